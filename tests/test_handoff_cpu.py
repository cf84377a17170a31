"""CPU: the checker of the hand-off kernels (tests/_handoff_check.py) checked itself.  The fp32 restatements -- the
oracle's resize, a numpy adjoint, a numpy projection on the device's operand formats -- meet every bound on every
case's shapes, and deliberately wrong restatements are rejected."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import list_oracle as O, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _handoff_check as hc  # noqa: E402

F32 = np.float32


# ---- fp32 restatements (and their wrong variants) ---------------------------------------------------------------------
def resize_f32(x, ms, shift=0, swap=False, clamp=True):
    """k_prep_img in numpy fp32, channels-last.  shift: taps moved by one pixel; swap: wx0 and wx1 exchanged; clamp=False:
    i1 = i0 + 1 without the edge test, reading on into the next row (the last pixel: the first one) as the device would."""
    x = np.asarray(x, F32)
    B, C, H, W = x.shape
    y0, y1, wy0, wy1 = hc.axis(H, ms)
    x0, x1, wx0, wx1 = hc.axis(W, ms)
    if not clamp:
        x1 = x0 + 1
    if swap:
        wx0, wx1 = wx1, wx0
    flat = x.reshape(B, C, H * W)

    def tap(yy, xx):
        i = (yy[:, None] * W + xx[None, :] + shift) % (H * W)
        return flat[:, :, i]
    with np.errstate(invalid="ignore", over="ignore"):
        top = tap(y0, x0) * wx0 + tap(y0, x1) * wx1
        bot = tap(y1, x0) * wx0 + tap(y1, x1) * wx1
        out = top * wy0[:, None] + bot * wy1[:, None]
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1).astype(F32))


def adjoint_f32(G, C, H, W, coff, dirty_row=None):
    """The adjoint in fp32 matrix products; dirty_row: a value left in the first source row no map row touches."""
    G = np.asarray(G, F32)
    ms = G.shape[1]
    My, ny = hc._adj_matrix(H, ms)
    Mx, _ = hc._adj_matrix(W, ms)
    g = G[..., coff:coff + C]
    r = np.einsum("oy,bopc->bypc", My.astype(F32), g).astype(F32)
    out = np.einsum("px,bypc->bcyx", Mx.astype(F32), r).astype(F32)
    if dirty_row is not None:
        out[:, :, np.flatnonzero(ny == 0)[0]] = dirty_row
    return out


def proj_f32(levels, wp, ms, n_kept, precision, skip=None, shift_block=0):
    """list_prep_img_proj's projected channels in numpy fp32 on the device's operand formats.  skip: a level left out of
    the sum; shift_block: every level takes the column block that many channels further on."""
    half = precision == "fp16"
    coff = sum(m.shape[1] for m in levels[:n_kept])
    out = 0
    for i, m in enumerate(levels[n_kept:]):
        C = m.shape[1]
        a = hc.level_rows(m)
        c0 = (coff + shift_block) % (wp.shape[1] - C + 1)
        w = wp[:, c0:c0 + C]
        if half:
            P = hc.sat_half(hc.sat_half(a).astype(F32) @ hc.sat_half(w).astype(F32).T).astype(F32)
        else:
            (ah, al), (wh, wl) = hc.split_bf16(a), hc.split_bf16(w)
            P = (ah @ wh.T + ah @ wl.T + al @ wh.T).astype(F32)
        coff += C
        if i == skip:
            continue
        out = out + O.resize_bilinear_align_corners(P.transpose(0, 3, 1, 2), ms).transpose(0, 2, 3, 1)
    out = out.astype(F32)
    return hc.sat_half(out) if half else out


def resize_worst(name, fn):
    """(worst error / bound of fn's fp32 result, of its saturating half) over the levels of a named case."""
    levels, ms = hc.resize_case(name)
    w32 = w16 = 0.0
    for i, m in enumerate(levels):
        ref, bound = hc.resize_case_reference(name, i)
        got = fn(m, ms)
        w32, w16 = max(w32, hc.worst(got, ref, bound)), max(w16, hc.worst(hc.sat_half(got), ref, bound, True))
    return w32, w16


def oracle_resize(m, ms):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.ascontiguousarray(O.resize_bilinear_align_corners(m, ms).transpose(0, 2, 3, 1))


# ---- the formats ------------------------------------------------------------------------------------------------------
def test_saturating_half_and_bf16_split():
    x = np.array([np.nan, np.inf, -np.inf, 70000.0, -70000.0, 65520.0, 65519.996, 65504.0, 1.0 + 2.0 ** -11,
                  1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 2.0 ** -149], F32)
    h = hc.sat_half(x)
    want = np.array([np.nan, 65504, -65504, 65504, -65504, 65504, 65504, 65504, 1.0, 1.0 + 2.0 ** -9, 0.0, 0.0], np.float16)
    assert hc.same_bits(h, want), (h, want)
    v = synth.normalish(3, (4096,), 3.0)
    hi, lo = hc.split_bf16(v)
    assert np.array_equal(hi, torch.from_numpy(v).bfloat16().float().numpy())
    assert np.array_equal(lo, torch.from_numpy(v - hi).bfloat16().float().numpy())
    assert np.abs(hi.astype(np.float64) + lo - v).max() <= np.abs(v).max() * 2.0 ** -16


def test_footprints_are_atens():
    """hc.axis against torch's own upsample on the CPU: an impulse response recovers every index and weight."""
    for S, ms in [(14, 137), (224, 137), (512, 137), (3, 320), (1, 7), (7, 2), (137, 137)]:
        i0, i1, w0, w1 = hc.axis(S, ms)
        eye = torch.eye(S, dtype=torch.float32).reshape(1, S, S, 1)
        M = torch.nn.functional.interpolate(eye, size=(ms, 1), mode="bilinear", align_corners=True)[0, :, :, 0].numpy().T
        mine = np.zeros((ms, S), F32)
        np.add.at(mine, (np.arange(ms), i0), w0)
        np.add.at(mine, (np.arange(ms), i1), w1)
        assert np.abs(mine - M).max() <= 2.0 ** -22, (S, ms)
        assert (i1 <= S - 1).all() and (i0 >= 0).all() and (w1 >= 0).all() and (w0 >= 0).all()


# ---- part 1: the resize -----------------------------------------------------------------------------------------------
SMALL_RESIZE = ["R1", "R3b", "R6"]


@pytest.mark.parametrize("name", list(hc.RESIZE_CASES))
def test_oracle_resize_meets_the_bound(name):
    w32, w16 = resize_worst(name, oracle_resize)
    print(f"{name}: oracle fp32 resize, worst error / bound fp32 {w32:.3f}, fp16 {w16:.3f}")
    assert w32 <= 1.0 and w16 <= 1.0
    if name in SMALL_RESIZE:                                   # (the restatement the wrong variants are made from)
        assert max(resize_worst(name, resize_f32)) <= 1.0


def rejected(fn, names):
    return [n for n in names if resize_worst(n, fn)[0] > 1.0]


def test_wrong_resizes_are_rejected():
    assert rejected(lambda m, ms: resize_f32(m, ms, shift=1), SMALL_RESIZE) == SMALL_RESIZE
    assert rejected(lambda m, ms: resize_f32(m, ms, swap=True), SMALL_RESIZE)
    assert rejected(lambda m, ms: resize_f32(m, ms, clamp=False), SMALL_RESIZE)
    # plain RNE instead of the saturating conversion: 70000 and the infinities become infinities
    levels, ms = hc.resize_case("R1")
    ref, bound = hc.resize_case_reference("R1", 4)
    with np.errstate(over="ignore"):
        assert hc.worst(resize_f32(levels[4], ms).astype(np.float16), ref, bound, True) == np.inf
    assert hc.worst(hc.sat_half(resize_f32(levels[4], ms)), ref, bound, True) <= 1.0


def test_special_values_reach_every_class():
    """R8: the planted values give NaN (inf * 0 at a grid-aligned tap), infinities, saturated and subnormal references."""
    ref = np.concatenate([hc.resize_case_reference("R1", i)[0].ravel() for i in range(5)])
    assert np.isnan(ref).any() and (ref == np.inf).any() and (ref == -np.inf).any()
    fin = ref[np.isfinite(ref)]
    assert (fin > 65504 * 1.01).any() and (fin < -65504 * 1.01).any()
    assert ((np.abs(fin) > 0) & (np.abs(fin) < 2.0 ** -126)).any()
    assert np.isfinite(ref).mean() > 0.8


# ---- part 2: the adjoint ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hc.ADJOINT_CASES))
def test_numpy_adjoint_meets_the_bound(name):
    G, shapes = hc.adjoint_case(name)
    coff = 0
    for (C, H, W) in shapes:
        ref, bound = hc.adjoint_reference(G, C, H, W, coff)
        assert hc.worst(adjoint_f32(G, C, H, W, coff), ref, bound) <= 1.0, (name, C, H, W)
        # <resize(x), g> == <x, adjoint(g)>: the reference is the transpose of the forward's reference
        x = synth.normalish(5, (G.shape[0], C, H, W))
        y, _ = hc.resize_reference(x, G.shape[1])
        lhs, rhs = float((y * G[..., coff:coff + C]).sum()), float((x * ref).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, float((np.abs(x) * np.abs(ref)).sum()))
        coff += C


def test_wrong_adjoints_are_rejected():
    G, shapes = hc.adjoint_case("A_ms137")
    C, H, W = shapes[2]                                        # 512 -> 137: 272 rows touched
    coff = sum(s[0] for s in shapes[:2])
    ref, bound = hc.adjoint_reference(G, C, H, W, coff)
    assert int((bound[0, 0, :, 0] > 0).sum()) == 272
    assert hc.worst(adjoint_f32(G, C, H, W, coff, dirty_row=1e-30), ref, bound) == np.inf
    assert hc.worst(np.full(ref.shape, np.nan, F32), ref, bound) == np.inf          # a workgroup that did not write
    assert hc.worst(np.roll(adjoint_f32(G, C, H, W, coff), 1, axis=3), ref, bound) > 1.0


# ---- part 3: the transposes -------------------------------------------------------------------------------------------
def test_wrong_transposes_are_rejected():
    src = synth.normalish(9, (2, 16, 3, 5, 7))
    src[0, :9, 1, 2, 3] = hc.SPECIALS
    for f16 in (False, True):
        want = hc.vox_expected(src, f16)
        assert hc.same_bits(want.copy(), want)
        assert not hc.same_bits(np.roll(want, 1, axis=-1), want)
    with np.errstate(over="ignore"):
        plain = np.transpose(src, (0, 2, 3, 4, 1)).astype(np.float16)
    assert not hc.same_bits(np.ascontiguousarray(plain), hc.vox_expected(src, True))
    assert hc.vox_expected(synth.normalish(9, (2, 16, 3, 5, 7)).astype(np.float16), False).dtype == F32


# ---- part 4: the projection -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proj_case():
    levels = hc.make_levels(8500, hc.PROJ_B, hc.PROJ_SHAPES)
    img_C = sum(s[0] for s in hc.PROJ_SHAPES)
    wp = hc.percep_columns(hc.proj_weights(8600, img_C, hc.PROJ_H1)["fc_0.weight"], img_C)
    assert wp.shape == (hc.PROJ_H1, img_C)
    return levels, wp


@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
def test_numpy_projection_meets_the_bound_and_wrong_ones_do_not(proj_case, precision):
    levels, wp = proj_case
    half = precision == "fp16"
    for k in range(5):
        ref, bound = hc.proj_reference(levels, wp, hc.PROJ_MS, k, precision)
        w = hc.worst(proj_f32(levels, wp, hc.PROJ_MS, k, precision), ref, bound, half)
        print(f"{precision} n_kept={k}: numpy restatement, worst error / bound {w:.3f}")
        assert w <= 1.0
        if k < 4:
            assert hc.worst(proj_f32(levels, wp, hc.PROJ_MS, k, precision, skip=4 - k - 1), ref, bound, half) > 1.0
        assert hc.worst(proj_f32(levels, wp, hc.PROJ_MS, k, precision, shift_block=64), ref, bound, half) > 1.0


def test_gemm_reference_on_the_prepared_map():
    """list_prep_percep_proj's check: one product on its own input, no resize."""
    a = synth.normalish(31, (50, 384))
    w = synth.uniform(32, (256, 384), -0.05, 0.05)
    for precision in ("fp16", "bf16x3"):
        half = precision == "fp16"
        P, e = hc.gemm_reference(a, w, precision, half)
        if half:
            got = hc.sat_half(hc.sat_half(a).astype(F32) @ hc.sat_half(w).astype(F32).T)
        else:
            (ah, al), (wh, wl) = hc.split_bf16(a), hc.split_bf16(w)
            got = (ah @ wh.T + ah @ wl.T + al @ wh.T).astype(F32)
        assert hc.worst(got, P, e) <= 1.0
        assert hc.worst(np.roll(np.asarray(got, F32), 1, axis=1), P, e) > 1.0
