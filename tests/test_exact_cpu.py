"""The exact-integer cases of tests/_exact_case.py, checked without a GPU:

  * the integer reference agrees, exactly, with independent code (the oracle's float32 MLP and feature concatenation,
    torch's float64 autograd);
  * an ideal kernel -- a numpy emulation of each operand format that splits the operands as the kernels store them, sums
    products in float64 and rounds once to fp32 per split -- reproduces the reference bit for bit in any K-tile order and
    with split-K, for every admitted (class, precision) pair;
  * every deliberately broken emulation is caught (the count of differing elements is printed and recorded);
  * the builders' own assertions trip on an operand one bit too wide.
"""
import numpy as np
import pytest
import torch

import _exact_case as E
from oracle import list_oracle as O

F32, F64 = np.float32, np.float64
PAIRS = [(cls, p) for cls, precs in E.GEMM_CLASSES.items() for p in precs]
KT = 64


# ------------------------------------------------------------------------------------------ the emulated kernel
def emulate_gemm(a, w, precision, seed=None, splits=1, mutant=None):
    """out = a @ w.T as a kernel of `precision` would form it: planes, K-tiles of 64 in a (shuffled) order, `splits`
    partial sums each rounded to fp32 once, then added in fp32."""
    pad = -a.shape[1] % KT                                 # (the library pads K to its tile with zero columns too)
    a, w = np.pad(np.asarray(a, F32), ((0, 0), (0, pad))), np.pad(np.asarray(w, F32), ((0, 0), (0, pad)))
    (ah, al), (wh, wl) = E.planes(a, precision), E.planes(w, precision)
    ah, al, wh, wl = (t.astype(F64) for t in (ah, al, wh, wl))
    if mutant == "a_lo_dropped":
        al = np.zeros_like(al)
    if mutant == "w_lo_dropped":
        wl = np.zeros_like(wl)
    nk = a.shape[1] // KT
    tiles = [(t, t) for t in range(nk)]                   # (K-tile of A, K-tile of W)
    if mutant == "last_tile_skipped":
        tiles = tiles[:-1]
    if mutant == "tile_doubled":
        tiles.append(tiles[nk // 2])
    if mutant == "a_tiles_swapped" and nk > 1:
        tiles[0], tiles[nk - 1] = (nk - 1, 0), (0, nk - 1)
    if seed is not None:
        np.random.default_rng(seed).shuffle(tiles)
    out = np.zeros((a.shape[0], w.shape[0]), F32)
    per = -(-len(tiles) // splits)
    for s in range(0, len(tiles), per):
        acc = np.zeros(out.shape, F64)
        for ta, tw in tiles[s:s + per]:
            ka, kw = slice(ta * KT, (ta + 1) * KT), slice(tw * KT, (tw + 1) * KT)
            acc += ah[:, ka] @ wh[:, kw].T + ah[:, ka] @ wl[:, kw].T + al[:, ka] @ wh[:, kw].T
        out = (out + acc.astype(F32)).astype(F32)
    return out


def stored(x, precision):
    hi, lo = E.planes(np.asarray(x, F32), precision)
    return hi.astype(F64) + lo.astype(F64)


def emulate_chain(c, precision, mutant=None):
    """Forward and backward of the MLP case as the library lays them out: rows padded to the 256-row tile with X = 0,
    activations and gradient operands stored in `precision`, the fp16 gradient scale, weight gradients over all rows."""
    w = c["weights"]
    W = [np.asarray(w[f"fc_{i}.weight"], F32)[:, :, 0] for i in range(3)] + [np.asarray(w["fc_out.weight"], F32)[:, :, 0]]
    b = [np.asarray(w[f"fc_{i}.bias"], F64) for i in range(3)] + [np.asarray(w["fc_out.bias"], F64)]
    P = E.B * E.N
    rows = -(-P // 256) * 256
    X = np.zeros((rows, E.F), F32)
    X[:P] = np.transpose(c["X"], (0, 2, 1)).reshape(P, E.F)
    acts = [stored(X, precision)]
    for i in range(3):
        z = emulate_gemm(acts[i].astype(F32), W[i], precision).astype(F64) + b[i]
        acts.append(stored(np.maximum(z, 0).astype(F32), precision))
    out = {"sdf": ((acts[3] @ W[3].astype(F64).T)[:, 0] + b[3][0]).astype(F32)[:P]}
    s = E.FP16_GRAD_SCALE if precision == "fp16" else 1.0
    g = np.zeros((rows, 1), F64)
    g[:P, 0] = c["grad_sdf"].reshape(-1)
    out["d_fc_out.weight"] = (g.T @ acts[3]).astype(F32)[:, :, None]
    out["d_fc_out.bias"] = g.sum(0).astype(F32)
    if mutant == "padded_rows_leak":
        g[P:] = 1.0                                      # padded rows hold relu(bias) chains: only dZ = 0 keeps them out of dW
    dz = stored((s * g * W[3].astype(F64) * (acts[3] > 0)).astype(F32), precision)
    for i in (2, 1, 0):
        dw = emulate_gemm(dz.T.astype(F32), acts[i].T.astype(F32), precision, splits=3).astype(F64) / s
        out[f"d_fc_{i}.weight"] = dw.astype(F32)[:, :, None]
        out[f"d_fc_{i}.bias"] = (dz.sum(0) / s).astype(F32)
        dh = emulate_gemm(dz.astype(F32), W[i].T.copy(), precision).astype(F64)
        if i:
            dz = stored((dh * (acts[i] > 0)).astype(F32), precision)
    out["dX"] = (stored(dh.astype(F32), "fp16" if precision == "fp16" else "bf16x3") / s)[:P]
    if mutant == "wgrad_column_to_neighbour":
        dw0 = out["d_fc_0.weight"]
        col = int(np.argmax(np.abs(dw0[:, :, 0]).sum(0)))
        dw0[:, col + 1 if col + 1 < E.F else col - 1, 0] = dw0[:, col, 0]
        dw0[:, col, 0] = 0
    return out


def n_diff(a, b):
    return int((np.asarray(a, F64) != np.asarray(b, F64)).sum())


# ------------------------------------------------------------------------------------------ the reference is right
@pytest.mark.parametrize("variant,H1", [("narrow", 512), ("wide", 512), ("narrow", 768), ("zero_maps", 512)])
def test_reference_agrees_with_the_oracle_and_with_autograd(variant, H1):
    c = E.mlp_case(variant, H1)
    r = c["ref"]
    X32 = c["X"].astype(F32)
    assert np.array_equal(X32.astype(F64), c["X"])
    # the feature matrix: the oracle's own gathers on the zero / 1 x 1 x 1 pyramid (perm (0, 1, 2), scale 1: p = query)
    if H1 == 512:
        feats = O.concat_features(c["query"], c["vox_maps"], c["percep_feat"])
        assert feats.shape == (E.B, E.F, E.N)
        assert np.array_equal(feats.astype(F64), c["X"]), E.first_mismatch(feats.reshape(-1, E.N), c["X"].reshape(-1, E.N))
        nz = np.flatnonzero(np.abs(c["X"]).sum(axis=(0, 2)))
        if variant != "zero_maps":
            # the 1 x 1 x 1 level arrives as the 896 columns 1687 .. 2582 (a channel that is 0 in both images aside)
            assert E.LAST_LEVEL_COL == 1687 and nz.min() >= 1687 and nz.max() == E.F - 1
            assert (np.abs(c["X"][:, 1687:E.VOX_COLS]).sum(axis=(0, 2)) > 0).sum() > 800
    # forward: the oracle's float32 MLP (every sum is an integer multiple of the unit below 2^24: float32 is exact too)
    sdf, hidden = O.mlp(X32, c["weights"], return_hidden=True)
    assert np.array_equal(sdf.astype(F64), c["sdf"])
    for i, h in enumerate(hidden):
        assert np.array_equal(np.transpose(h, (0, 2, 1)).reshape(-1, h.shape[1]).astype(F64), r[f"H{i + 1}"])
    # backward: torch float64 autograd of the same MLP
    tw = {k: torch.from_numpy(np.asarray(v, F64)).requires_grad_(True) for k, v in c["weights"].items()}
    x = torch.from_numpy(c["X"].copy()).requires_grad_(True)
    h = x
    for name in ("fc_0", "fc_1", "fc_2", "fc_out"):
        h = torch.nn.functional.conv1d(h, tw[name + ".weight"], tw[name + ".bias"])
        if name != "fc_out":
            h = torch.relu(h)
    assert np.array_equal(h[:, 0].detach().numpy(), c["sdf"])
    h[:, 0].backward(torch.from_numpy(c["grad_sdf"].astype(F64)))
    for k in E.MLP_GRAD_KEYS:
        assert np.array_equal(tw[k[2:]].grad.numpy(), r[k].reshape(tw[k[2:]].shape)), k
    assert np.array_equal(x.grad.numpy()[:, E.VOX_COLS:E.VOX_COLS + E.IMG_C], c["d_percep_feat"])
    # the edge where masks matter is in the case: pre-activations that are exactly zero
    assert c["zero_preacts"] >= 1000
    # d fc_0.weight is exactly zero on the columns whose X is zero
    assert not r["d_fc_0.weight"][:, :E.LAST_LEVEL_COL].any() or variant == "zero_maps"


# ------------------------------------------------------------------------------------------ an ideal kernel passes
@pytest.mark.parametrize("cls,precision", PAIRS)
def test_ideal_emulation_reproduces_the_reference_in_any_order(cls, precision):
    g = E.gemm_case(cls, precision, 256, 264, 576)                      # 9 K-tiles: ragged under 2 and 4 splits
    want = g["ref"]
    assert np.abs(want).max() > 0
    for seed, splits in ((None, 1), (3, 1), (4, 2), (5, 4), (6, 9)):
        got = emulate_gemm(g["a"], g["w"], precision, seed=seed, splits=splits)
        assert got.dtype == F32 and np.array_equal(got.astype(F64), want), (seed, splits, E.first_mismatch(got, want))
    if cls != "d":                                # the true product and the three-term sum coincide when one lo is zero
        assert np.array_equal(want, E.gemm_reference(g["a"], g["w"], "d", "bf16x3"))


@pytest.mark.parametrize("variant,precision", [("narrow", "fp16"), ("narrow", "bf16x3"), ("narrow", "bf16"),
                                               ("wide", "fp16"), ("wide", "bf16x3")])
def test_ideal_chain_reproduces_the_reference(variant, precision):
    c = E.mlp_case(variant)
    got = emulate_chain(c, precision)
    assert np.array_equal(got["sdf"].astype(F64), c["ref"]["sdf"])
    for k in E.MLP_GRAD_KEYS:
        assert np.array_equal(got[k].astype(F64).reshape(c["ref"][k].shape), c["ref"][k]), (k, E.first_mismatch(
            got[k].reshape(got[k].shape[0], -1), c["ref"][k].reshape(got[k].shape[0], -1)))
    assert np.array_equal(got["dX"], c["ref"]["dX"])


# ------------------------------------------------------------------------------------------ a wrong kernel fails
LO_A = [(cls, p) for cls, p in PAIRS if p == "bf16x3" and cls in ("b7", "b12", "d")]
LO_W = [(cls, p) for cls, p in PAIRS if p == "bf16x3" and cls in ("c7", "c12", "d")]
GEMM_MUTANTS = ([("a_lo_dropped", c, p) for c, p in LO_A] + [("w_lo_dropped", c, p) for c, p in LO_W] +
                [(m, c, p) for m in ("last_tile_skipped", "tile_doubled", "a_tiles_swapped") for c, p in PAIRS])


@pytest.mark.parametrize("mutant,cls,precision", GEMM_MUTANTS)
def test_broken_gemm_emulations_are_caught(mutant, cls, precision, record_property):
    g = E.gemm_case(cls, precision, 256, 264, 576)
    got = emulate_gemm(g["a"], g["w"], precision, seed=11, splits=2, mutant=mutant)
    n = n_diff(got, g["ref"])
    record_property("differing_elements", n)
    print(f"mutant {mutant} on class {cls} / {precision}: {n} of {got.size} elements differ")
    assert n > 0 and not np.array_equal(got.astype(F64), g["ref"])


@pytest.mark.parametrize("precision", E.PRECISIONS)
def test_broken_chain_emulations_are_caught(precision, record_property):
    c = E.mlp_case("narrow")
    r = c["ref"]
    leak = emulate_chain(c, precision, "padded_rows_leak")
    n = sum(n_diff(leak[f"d_fc_{i}.weight"].reshape(r[f"d_fc_{i}.weight"].shape), r[f"d_fc_{i}.weight"]) for i in range(3))
    print(f"mutant padded_rows_leak / {precision}: {n} weight-gradient elements differ")
    record_property("padded_rows_leak", n)
    assert n > 0
    moved = emulate_chain(c, precision, "wgrad_column_to_neighbour")
    n = n_diff(moved["d_fc_0.weight"], r["d_fc_0.weight"])
    print(f"mutant wgrad_column_to_neighbour / {precision}: {n} elements of d fc_0.weight differ")
    record_property("wgrad_column_to_neighbour", n)
    assert n > 0


def test_mask_at_zero_is_seen(record_property):
    """h >= 0 instead of h > 0: differs only through the pre-activations that are exactly zero."""
    c = E.mlp_case("narrow")
    X = np.transpose(c["X"], (0, 2, 1)).reshape(-1, E.F)
    wrong = E.mlp_reference(X, c["weights"], c["grad_sdf"].reshape(-1), mask_ge=True)
    total = 0
    for k in E.MLP_GRAD_KEYS + ("dX",):
        n = n_diff(wrong[k], c["ref"][k])
        print(f"mutant mask h >= 0: {n} elements of {k} differ")
        total += n
    record_property("mask_ge", total)
    assert n_diff(wrong["d_fc_0.weight"], c["ref"]["d_fc_0.weight"]) > 0 and n_diff(wrong["dX"], c["ref"]["dX"]) > 0
    assert np.array_equal(wrong["sdf"], c["ref"]["sdf"])


# ------------------------------------------------------------------------------------------ the builder's own guards
def test_builder_refuses_operands_one_bit_too_wide():
    a, w = E.gemm_operands("a", 256, 256, 64)
    E.assert_exact_product(a, w, "bf16")
    # 8 / 11 significant bits fit bf16 / fp16, 9 / 12 do not; hi + lo holds 17 (lo's sign is the 17th), not 18
    for precision, fits, too_wide in (("bf16", 7.0 + 2.0 ** -5, 7.0 + 2.0 ** -6), ("fp16", 7.0 + 2.0 ** -8, 7.0 + 2.0 ** -9),
                                      ("bf16x3", 1.0 + 2.0 ** -8 + 2.0 ** -16, 1.0 + 2.0 ** -8 + 2.0 ** -17)):
        wide, ok = a.copy(), a.copy()
        wide[3, 5], ok[3, 5] = np.float32(too_wide), np.float32(fits)
        assert E.sig_bits(wide) == E.sig_bits(ok) + 1
        assert not E.exact_in(wide, precision) and E.exact_in(ok, precision)
        with pytest.raises(AssertionError, match="not stored exactly"):
            E.assert_exact_product(wide, w, precision)
    with pytest.raises(AssertionError, match="not admitted"):
        E.gemm_case("b12", "fp16", 256, 256, 64)
    b12, w12 = E.gemm_operands("b12", 256, 256, 64)
    assert not E.exact_in(b12, "fp16") and not E.exact_in(b12, "bf16") and E.exact_in(b12, "bf16x3")
    # the 2^24 bound: the same operands three times along K (a power-of-two factor would scale the unit with them)
    g = E.gemm_case("d", "bf16x3", 256, 256, 64)
    assert E.assert_exact_product(g["a"], g["w"], "bf16x3") * 3 >= E.LIMIT
    with pytest.raises(AssertionError, match="limit 2\\^24"):
        E.assert_exact_product(np.tile(g["a"], (1, 3)), np.tile(g["w"], (1, 3)), "bf16x3")
    assert E.sig_bits(np.array([0.0, 96.0, 257.0, 0.375])) == 9 and E.unit_of(np.array([6.0, 0.5]), np.array([4.0])) == 0.5
