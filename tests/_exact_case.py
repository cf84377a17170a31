"""Exact-integer operands for the MFMA GEMM family and the MLP chain, with their float64 references (numpy only).

The exactness lemma ("Exact-integer tests"): when every operand, AS THE KERNEL STORES IT, is an integer
multiple of one power of two (the unit), and sum_k |a_ik| |w_jk| stays below 2^24 units for every output, then every
partial sum any schedule can form is an integer below 2^24 units and fp32 holds it without rounding.  Tile order, MFMA
shape, split-K, the ping-pong stagger and the reduction tree cannot change a bit of the result, and fp16, bf16x3 and
bf16 must all return the one float64 answer.  The builders below ASSERT both conditions for every case they hand out,
so a test that compares with np.array_equal rests on nothing measured.
"""
import functools

import numpy as np

from oracle import cases, synth

F32, F64 = np.float32, np.float64
PRECISIONS = ("fp16", "bf16x3", "bf16")
LIMIT = float(1 << 24)
FP16_GRAD_SCALE = 32.0        # k_grad_scale_final: 2^k with max|grad_sdf| * 2^k in [32, 64); max|grad_sdf| = 1 here


# ------------------------------------------------------------------------------------------ storage emulation
def fp16_round(x):
    """float32 -> fp16 -> float32 (RNE)."""
    return np.asarray(x, F32).astype(np.float16).astype(F32)


def bf16_rne(x):
    """float32 -> bf16 (RNE on the bit pattern) -> float32."""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return r.view(F32).reshape(np.shape(x))


def planes(x, precision):
    """The operand as the kernels store it -> (hi, lo) float32 planes; lo is zero where the format has none."""
    x = np.asarray(x, F32)
    if precision == "fp16":
        return fp16_round(x), np.zeros_like(x)
    hi = bf16_rne(x)
    if precision == "bf16":
        return hi, np.zeros_like(x)
    return hi, bf16_rne((x - hi).astype(F32))


def exact_in(x, precision):
    """Stored without loss: the planes of `precision` add up to x (and x is a float32 to begin with)."""
    x64 = np.asarray(x, F64)
    hi, lo = planes(x64.astype(F32), precision)
    return bool(np.array_equal(hi.astype(F64) + lo.astype(F64), x64))


def _mantissa(x):
    m, e = np.frexp(np.abs(np.asarray(x, F64)))
    mi = (m * float(1 << 53)).astype(np.int64)            # exact: a double's 53-bit significand
    low = mi & -mi                                        # lowest set bit (0 for x == 0)
    tz = np.where(mi == 0, 53, np.frexp(np.maximum(low, 1).astype(F64))[1] - 1)
    return mi, e, tz


def sig_bits(x):
    """Largest number of significant bits (first to last set bit) of any entry; 0 for an all-zero array."""
    mi, _, tz = _mantissa(x)
    return int(np.where(mi == 0, 0, 53 - tz).max()) if mi.size else 0


def unit_of(*arrays):
    """The largest power of two that divides every entry of every array (1.0 when all are zero)."""
    best = None
    for x in arrays:
        mi, e, tz = _mantissa(x)
        if (mi != 0).any():
            lo = int((e - 53 + tz)[mi != 0].min())
            best = lo if best is None else min(best, lo)
    return 1.0 if best is None else float(np.ldexp(1.0, best))


def partial_sum_units(a, w, *more):
    """max_ij sum_k |a_ik| |w_jk| in units of unit_of(a) * unit_of(w); `more` (biases) must be multiples of that unit."""
    unit = unit_of(a) * unit_of(w)
    for b in more:
        assert unit_of(b) >= unit or not np.any(b), "a bias is no multiple of the product unit"
    worst = float((np.abs(np.asarray(a, F64)) @ np.abs(np.asarray(w, F64)).T).max()) if np.size(a) and np.size(w) else 0.0
    extra = max([float(np.abs(b).max()) for b in more if np.size(b)] or [0.0])
    return (worst + extra) / unit


def assert_exact_product(a, w, precision, *biases, what=""):
    """The lemma's two conditions for out = a @ w.T (+ bias) in `precision`.  For bf16x3 the bound is taken over the
    planes, whose lo parts have the finer unit."""
    assert exact_in(a, precision), f"{what}: A is not stored exactly in {precision}"
    assert exact_in(w, precision), f"{what}: W is not stored exactly in {precision}"
    if precision == "bf16x3":
        (ah, al), (wh, wl) = planes(a, precision), planes(w, precision)
        unit = unit_of(ah, al) * unit_of(wh, wl)
        for b in biases:
            assert not np.any(b) or unit_of(b) >= unit, f"{what}: bias below the product unit"
        absa, absw = np.abs(ah.astype(F64)) + np.abs(al.astype(F64)), np.abs(wh.astype(F64)) + np.abs(wl.astype(F64))
        units = (float((absa @ absw.T).max()) + max([float(np.abs(b).max()) for b in biases] or [0.0])) / unit
    else:
        units = partial_sum_units(a, w, *biases)
    assert units < LIMIT, f"{what}: partial sums reach {units:.0f} units (limit 2^24)"
    return units


# ------------------------------------------------------------------------------------------ GEMM operand classes
# class -> precisions admitted.  b* carry a lo part in A only (isolates A_lo . W_hi), c* in W only (A_hi . W_lo), d in both.
GEMM_CLASSES = {
    "a": ("fp16", "bf16x3", "bf16"),       # integers in [-7, 7], dense
    "b7": ("fp16", "bf16x3"),              # A = m + j 2^-7 (<= 11 significant bits), W integers
    "b12": ("bf16x3",),                    # A = m + j 2^-12 (<= 16 significant bits), W in {-1, 0, 1}
    "c7": ("fp16", "bf16x3"),              # mirrors of b
    "c12": ("bf16x3",),
    "d": ("bf16x3",),                      # both operands m + j 2^-9, m in {-1, 0, 1}, j in {-1, 0, 1}: three-term reference
}


def _ints(seed, shape, lo, hi):
    """Integers in [lo, hi] from the package's integer hash (platform independent)."""
    n = int(np.prod(shape))
    return ((synth._bits(seed, n) >> np.uint64(11)) % np.uint64(hi - lo + 1)).astype(np.int64).reshape(shape) + lo


def _wide(seed, shape, frac_bits, m_max):
    return (_ints(seed, shape, -m_max, m_max) + _ints(seed + 1, shape, 0, (1 << frac_bits) - 1) / float(1 << frac_bits)).astype(F32)


def _narrow_for(seed, shape, frac_bits):
    if frac_bits == 7:
        return _ints(seed, shape, -3, 3).astype(F32)                 # 3648 * 8 * 2^7 * 3 < 2^24
    z = _ints(seed, shape, -1, 1) * (_ints(seed + 1, shape, 0, 3) == 0)     # {-1, 0, 1}, a quarter of the slots taken
    return z.astype(F32)


def _class_d(seed, shape, K):
    # m + j 2^-9: for m = +-1 the bf16 hi plane is +-1 and lo = j 2^-9; the unit of a product is 2^-18, so at most
    # ~2^6 products of magnitude 1 may meet in one output: the density falls with K
    keep = _ints(seed + 2, shape, 0, (1 << 20) - 1) < int((1 << 20) * min(1.0, (32.0 / K) ** 0.5))
    x = _ints(seed, shape, -1, 1) + _ints(seed + 1, shape, -1, 1) / 512.0
    return (x * keep).astype(F32)


@functools.lru_cache(maxsize=8)
def gemm_operands(cls, rows_a, rows_w, K, seed=1):
    """A [rows_a, K], W [rows_w, K] of one operand class (float32).  Cached: treat the arrays as read-only."""
    sa, sw = 1000 * seed + 17, 1000 * seed + 59
    if cls == "a":
        return _ints(sa, (rows_a, K), -7, 7).astype(F32), _ints(sw, (rows_w, K), -7, 7).astype(F32)
    if cls in ("b7", "b12"):
        fb = 7 if cls == "b7" else 12
        return _wide(sa, (rows_a, K), fb, 7 if fb == 7 else 3), _narrow_for(sw, (rows_w, K), fb)
    if cls in ("c7", "c12"):
        fb = 7 if cls == "c7" else 12
        return _narrow_for(sa, (rows_a, K), fb), _wide(sw, (rows_w, K), fb, 7 if fb == 7 else 3)
    if cls == "d":
        return _class_d(sa, (rows_a, K), K), _class_d(sw, (rows_w, K), K)
    raise KeyError(cls)


def gemm_reference(a, w, cls, precision):
    """float64 a @ w.T: exact (every term is a multiple of the unit and the sums stay far below 2^53).  Class d: the
    kernels' documented three-term sum A_hi W_hi + A_hi W_lo + A_lo W_hi of the emulated planes (A_lo W_lo is dropped by
    design), not the true product."""
    if cls != "d":
        return np.asarray(a, F64) @ np.asarray(w, F64).T
    (ah, al), (wh, wl) = planes(a, precision), planes(w, precision)
    ah, al, wh, wl = (t.astype(F64) for t in (ah, al, wh, wl))
    return ah @ wh.T + ah @ wl.T + al @ wh.T


def gemm_case(cls, precision, rows_a, rows_w, K, seed=1):
    """-> dict(a, w, bias, ref, ref_bias, units): operands, an integer bias over W's rows, the references without and
    with it.  Asserts representability and the 2^24 bound."""
    assert precision in GEMM_CLASSES[cls], f"class {cls} is not admitted for {precision}"
    a, w = gemm_operands(cls, rows_a, rows_w, K, seed)
    bias = _ints(7000 + seed, (rows_w,), -7, 7).astype(F32)
    units = assert_exact_product(a, w, precision, bias, what=f"class {cls} {precision} K={K}")
    ref = gemm_reference(a, w, cls, precision)
    return dict(a=a, w=w, bias=bias, ref=ref, ref_bias=ref + bias.astype(F64)[None, :], units=units)


def first_mismatch(got, want, tile=256):
    """'' when equal, else the first differing (row, col), its tile and got / want -- for assertion messages."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    idx = tuple(int(i) for i in bad[0])
    where = f"tile {tuple(i // tile for i in idx)}" if len(idx) == 2 else ""
    return f"{len(bad)} of {got.size} differ; first at {idx} {where}: got {float(got[idx])!r}, want {float(want[idx])!r}"


# ------------------------------------------------------------------------------------------ the MLP case
B, N = 2, 300                              # B * N = 600: three 256-row tiles, the last one ragged
F = 3610
VOX_COLS = 2583                            # [2583 voxel | 1024 perceptual | 3 coordinates]
LAST_LEVEL_COL = 7 * sum(synth.VOX_CHANNELS[:5])      # 1687: first column of the 1 x 1 x 1 level
IMG_C = 1024
_MULTS = (5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61)


def shifted_perms(rows, cols, n_terms, salt):
    """Sum of n_terms signed shifted permutations r -> (mult_t r + shift_t) mod cols: entries in {-1, 0, 1}, row degree
    n_terms, column degree <= n_terms * ceil(rows / cols)."""
    w = np.zeros((rows, cols), np.int64)
    r = np.arange(rows)
    mult = _MULTS[salt % len(_MULTS)]           # one permutation per matrix, shifted: two patterns never meet
    for t in range(n_terms):
        shift = (t * (cols // n_terms) + 31 * salt + (t * t) % 5) % cols
        sign = np.where(((r + t) * (2 * t + 3) // 7 + salt) % 2 == 0, 1, -1)
        assert (w[r, (mult * r + shift) % cols] == 0).all(), "two patterns meet: choose other shifts"
        w[r, (mult * r + shift) % cols] = sign
    assert int((w != 0).sum()) == rows * n_terms
    return w


def _mlp_weights(H1, zero_maps=False):
    H2 = H3 = 256
    w0 = np.zeros((H1, F), np.int64)
    # the columns whose X is zero: dense small integers, so that a K-tile taken from the wrong place shows
    w0[:, :LAST_LEVEL_COL] = _ints(4100, (H1, LAST_LEVEL_COL), -2, 2)
    if zero_maps:
        w0[:, LAST_LEVEL_COL:F - 3] = _ints(4101, (H1, F - 3 - LAST_LEVEL_COL), -2, 2)
        r = np.arange(H1)                      # two of the three coordinate columns per row, +-1: xyz does reach H1
        w0[r, F - 3 + r % 3] = np.where(r % 2 == 0, 1, -1)
        w0[r, F - 3 + (r + 1) % 3] = np.where(r % 5 < 2, -1, 1)
    else:
        w0[:, LAST_LEVEL_COL:] = shifted_perms(H1, F - LAST_LEVEL_COL, 12, 0)
    w1 = shifted_perms(H2, H1, 6, 3)
    w2 = shifted_perms(H3, H2, 4, 5)
    c = np.arange(H3)
    w3 = np.where(c % 8 == 1, np.where((c // 8) % 3 == 0, -1, 1), 0)[None, :]
    wt = {"fc_0.weight": w0, "fc_1.weight": w1, "fc_2.weight": w2, "fc_out.weight": w3,
          "fc_0.bias": (np.arange(H1) * 3) % 5 - 2, "fc_1.bias": (np.arange(H2) * 7) % 5 - 3,
          "fc_2.bias": (np.arange(H3) * 5) % 7 - 4, "fc_out.bias": np.array([2])}
    return {k: (v[:, :, None] if k.endswith("weight") else v).astype(F32) for k, v in wt.items()}


def mlp_reference(X, weights, grad_sdf=None, mask_ge=False):
    """float64 forward (and, with grad_sdf, backward) of the four-layer MLP on X [P, F]; masks are h > 0.
    -> dict(sdf, H1..H3, Z1..Z3 and, with grad_sdf, the eight gradients, dZ1..dZ3, dX)."""
    W = [np.asarray(weights[f"{n}.weight"], F64)[:, :, 0] for n in ("fc_0", "fc_1", "fc_2", "fc_out")]
    b = [np.asarray(weights[f"{n}.bias"], F64) for n in ("fc_0", "fc_1", "fc_2", "fc_out")]
    out, h = {}, np.asarray(X, F64)
    acts = [h]
    for i in range(3):
        z = h @ W[i].T + b[i]
        h = np.maximum(z, 0.0)
        out[f"Z{i + 1}"], out[f"H{i + 1}"] = z, h
        acts.append(h)
    out["sdf"] = (h @ W[3].T + b[3])[:, 0]
    if grad_sdf is None:
        return out
    g = np.asarray(grad_sdf, F64).reshape(-1, 1)
    out["d_fc_out.weight"], out["d_fc_out.bias"] = (g.T @ acts[3])[:, :, None], g.sum(0)
    dh = g @ W[3]
    for i in (2, 1, 0):
        z = out[f"Z{i + 1}"]
        dz = dh * ((z >= 0) if mask_ge else (z > 0))
        out[f"dZ{i + 1}"] = dz
        name = f"fc_{i}"
        out[f"d_{name}.weight"], out[f"d_{name}.bias"] = (dz.T @ acts[i])[:, :, None], dz.sum(0)
        dh = dz @ W[i]
    out["dX"] = dh
    return out


MLP_GRAD_KEYS = tuple(f"d_{n}.{p}" for n in ("fc_0", "fc_1", "fc_2", "fc_out") for p in ("weight", "bias"))


@functools.lru_cache(maxsize=None)
def mlp_case(variant="narrow", H1=512):
    """variant 'narrow': percep_feat integers in [-3, 3] (every precision); 'wide': percep_feat = m + j / 16 (fp16 and
    bf16x3); 'zero_maps': image AND voxel maps all zero, the chain driven by the coordinates and the biases (forward).
    Cached: treat the arrays as read-only."""
    assert variant in ("narrow", "wide", "zero_maps")
    tiny = cases.build_case("tiny")
    query = (_ints(5100, (B, N, 3), -1, 1) * 0.5).astype(F32)
    vox = [np.zeros_like(m) for m in tiny["vox_maps"]]
    assert vox[5].shape == (B, 128, 1, 1, 1)
    c = dict(variant=variant, H1=H1, query=query, trans_mat=tiny["trans_mat"], precisions=PRECISIONS)
    if variant == "zero_maps":
        c["img_maps"] = [np.zeros_like(m) for m in tiny["img_maps"]]
        pf = np.zeros((B, IMG_C, N), F32)
    else:
        vox[5][:] = _ints(5200, vox[5].shape, -3, 3).astype(F32)
        if variant == "narrow":
            pf = _ints(5300, (B, IMG_C, N), -3, 3).astype(F32)
        else:
            pf = _wide(5400, (B, IMG_C, N), 4, 1)
            c["precisions"] = ("fp16", "bf16x3")
    c["vox_maps"], c["percep_feat"] = vox, pf
    c["weights"] = w = _mlp_weights(H1, zero_maps=variant == "zero_maps")
    c["grad_sdf"] = _ints(5500, (B, N), -1, 1).astype(F32)

    # the integer X: [voxel | perceptual | coordinates]; the 1 x 1 x 1 level gives each of its 128 channels to all
    # seven stencil samples of every point of its image (columns 1687 .. 2582)
    X = np.zeros((B, F, N), F64)
    X[:, LAST_LEVEL_COL:VOX_COLS, :] = np.repeat(vox[5].reshape(B, 128).astype(F64), 7, axis=1)[:, :, None]
    X[:, VOX_COLS:VOX_COLS + IMG_C, :] = pf
    X[:, VOX_COLS + IMG_C:, :] = np.transpose(query, (0, 2, 1))
    c["X"] = X
    rows = np.transpose(X, (0, 2, 1)).reshape(B * N, F)
    r = mlp_reference(rows, w, c["grad_sdf"].reshape(-1))
    c["ref"] = r
    c["sdf"] = r["sdf"].reshape(B, N)
    c["d_percep_feat"] = np.transpose(r["dX"].reshape(B, N, F)[:, :, VOX_COLS:VOX_COLS + IMG_C], (0, 2, 1))

    # ---- what the lemma needs, for every precision the case is admitted for
    act_bits = 8 if variant != "wide" else 11
    for k in ("H1", "H2", "H3"):
        assert sig_bits(r[k]) <= act_bits, (k, sig_bits(r[k]))
    assert sig_bits(rows) <= (8 if variant != "wide" else 11)
    for k in ("dZ3", "dZ2", "dZ1", "dX"):
        assert sig_bits(r[k]) <= 8, (k, sig_bits(r[k]))                 # hi-only in every format
    assert np.abs(r["dX"]).max() * FP16_GRAD_SCALE < 65504.0
    acts = [rows, r["H1"], r["H2"], r["H3"]]
    Ws = [np.asarray(w[f"{n}.weight"], F64)[:, :, 0] for n in ("fc_0", "fc_1", "fc_2", "fc_out")]
    bs = [np.asarray(w[f"{n}.bias"], F64) for n in ("fc_0", "fc_1", "fc_2", "fc_out")]
    worst = 0.0
    for p in c["precisions"]:
        for i in range(4):
            assert exact_in(acts[i], p) and exact_in(Ws[i], p), (p, i)
        for k in ("dZ3", "dZ2", "dZ1"):
            assert exact_in(r[k] * (FP16_GRAD_SCALE if p == "fp16" else 1.0), p), (p, k)
    for i in range(4):
        worst = max(worst, partial_sum_units(acts[i], Ws[i], bs[i]))                       # forward products
    for i in (2, 1, 0):
        dz = r[f"dZ{i + 1}"] * FP16_GRAD_SCALE
        worst = max(worst, partial_sum_units(dz, Ws[i].T), partial_sum_units(dz.T, acts[i].T))   # data / weight gradients
    worst = max(worst, partial_sum_units(c["grad_sdf"].reshape(1, -1).astype(F64), r["H3"].T))
    assert worst < LIMIT, worst
    c["units"] = worst
    c["zero_preacts"] = int(sum((r[k] == 0).sum() for k in ("Z1", "Z2", "Z3")))
    return c
