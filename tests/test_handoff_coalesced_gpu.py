"""GPU: the lane-along-x form of the row-streaming resize (prep_kernels.hip: k_prep_img_rows<F16, 1>) -- a wave is one
channel octet of 64 neighbouring output columns -- on x-contiguous levels with sx = (W - 1) / (ms - 1) >= 0.5, and the
dispatch around it: launch_prep_img sends every other level of the same pyramid to the 8-columns-by-8-octets form in a
launch of its own; and the projection of the low-resolution levels straight from their NCHW sources (k_proj_level_nchw,
fp16 operands), launched behind the kept levels' resize without a barrier (list_prep_img_proj).

Every element meets the float64 reference within the derived bound of tests/_handoff_check.py (error / bound <= 1), and
agrees bit for bit with the same data sent through kernels this form does not touch: a channels-last copy (the `vec`
loads of k_prep_img_rows<F16, 0>) and a pyramid whose last level is cut to 32 channels (rows_eligible fails: the
per-level kernels k_prep_img_tile / k_prep_img).  Each test prints its worst error / bound (a record, not a tolerance)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _handoff_check as hc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2
XL_MIN_SX = 0.5               # kRowsXlMinSx
XL_PX = 64                    # kRowsPxXl: output columns of a workgroup

# name -> (ms, level shapes (C, H, W)); what each level is there for:
PYRAMIDS = {
    # 31 x 29: sx = 28 / 18 > 1, 19 columns in one ragged 64-column tile; 16 x 12, C = 128: 0.5 <= sx = 11 / 18 < 1, two
    # channel groups; 12 x 9: sx = 8 / 18 just below the threshold -> the old form; 7 x 10: sx = 9 / 18 = 0.5 exactly ->
    # the new one; 5 x 4: up-sampled, old form
    "ms19": (19, [(64, 31, 29), (128, 16, 12), (64, 12, 9), (64, 7, 10), (64, 5, 4)]),
    # 64 x 64: ms = 70 = 64 + 6 columns, two column tiles, the right-edge x1 clamp (x0 = W - 1 at the last column) in the
    # second; 40 x 36: sx = 35 / 69 = 0.507 new; 30 x 35: sx = 34 / 69 = 0.493 old
    "ms70": (70, [(64, 64, 64), (64, 40, 36), (64, 30, 35), (64, 8, 8), (64, 3, 2)]),
    # the smallest accepted case: 2 x 2 -> 3 (sx = 0.5); beside it W = 3 (sx = 1), W = 1 (no pair loads: old form),
    # H = 1 with W = 2
    "ms3": (3, [(64, 2, 2), (128, 2, 3), (64, 3, 1), (64, 1, 2), (64, 2, 2)]),
}
# levels that must take the lane-along-x form when dense NCHW (restated from rows_lane_along_x, prep_kernels.hip)
EXPECT_XL = {"ms19": [True, True, False, True, False], "ms70": [True, True, False, False, False],
             "ms3": [True, True, False, True, True]}
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pyramid(name):
    """(levels with planted specials, ms, [(ref, bound)] per level), built once and left unchanged."""
    if name not in _cache:
        ms, shapes = PYRAMIDS[name]
        levels = hc.make_levels(9700 + 100 * list(PYRAMIDS).index(name), B, shapes, specials=True)
        refs = [hc.resize_reference(m, ms) for m in levels]
        for r in refs:
            r[0].setflags(write=False)
            r[1].setflags(write=False)
        _cache[name] = (levels, ms, refs)
    return _cache[name]


def padded_nchw(m):
    """Dense [C,H,W] images with a batch stride larger than C * H * W (sb = C * H * W + 20 floats)."""
    b, n = m.shape[0], m[0].size
    base = torch.full((b, n + 20), float("nan"), device=DEV)
    base[:, :n] = dev(m).reshape(b, n)
    t = base[:, :n].view(m.shape)
    assert t.stride(0) == n + 20 and t.stride(3) == 1 and not t.is_contiguous()
    return t


def takes_xl(t, ms):
    """rows_lane_along_x of launch_prep_img: not `vec`, x-contiguous with a pair to load, sx >= 0.5 (in fp32 as there)."""
    vec = t.stride(1) == 1 and all(t.stride(d) % 4 == 0 for d in (0, 2, 3)) and t.data_ptr() % 16 == 0
    sx = np.float32(t.shape[3] - 1) / np.float32(ms - 1)
    return (not vec) and t.stride(3) == 1 and t.shape[3] >= 2 and bool(sx >= np.float32(XL_MIN_SX))


def channels_last(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date
    from list_amd import hip as h
    h.load()
    return h


@pytest.mark.parametrize("md", ["f32", "f16"])
@pytest.mark.parametrize("name", list(PYRAMIDS))
def test_lane_along_x_resize_per_element_and_bit_for_bit(hip, name, md):
    levels, ms, refs = pyramid(name)
    ts = [padded_nchw(m) for m in levels]
    assert [takes_xl(t, ms) for t in ts] == EXPECT_XL[name]
    if name == "ms70":
        assert ms > XL_PX                                       # more than one 64-column tile
    got_t = hip.prep_img_maps(ts, ms, md).data
    got = got_t.cpu().numpy()
    half = md == "f16"
    coff = 0
    for i, (m, (ref, bound)) in enumerate(zip(levels, refs)):
        C = m.shape[1]
        w = hc.worst(got[..., coff:coff + C], ref, bound, half)
        print(f"resize {name} {md} level {i} {m.shape[1:]} {'lane-along-x' if EXPECT_XL[name][i] else 'old form'}: "
              f"worst error / bound {w:.3f}")
        assert w <= 1.0, (name, md, i, w)
        coff += C
    assert coff == got.shape[-1]
    # the same data through kernels the new form does not touch
    bits = torch.int16 if half else torch.int32
    cl = [channels_last(dev(m)) for m in levels]
    assert not any(takes_xl(t, ms) for t in cl)
    other = hip.prep_img_maps(cl, ms, md).data
    diff = int((got_t.view(bits) != other.view(bits)).sum())
    print(f"resize {name} {md}: {diff} of {got_t.numel()} elements differ from the channels-last run")
    assert diff == 0, (name, md, diff)
    cut = [dev(m) for m in levels]
    cut[-1] = cut[-1][:, :32]                                   # rows_eligible fails: every level takes a per-level kernel
    other = hip.prep_img_maps(cut, ms, md).data
    n = other.shape[-1]
    diff = int((got_t[..., :n].contiguous().view(bits) != other.view(bits)).sum())
    print(f"resize {name} {md}: {diff} of {other.numel()} elements differ from the per-level kernels")
    assert diff == 0, (name, md, diff)


@pytest.fixture(scope="module")
def proj_levels():
    return hc.make_levels(9900, B, hc.PROJ_SHAPES, specials=False)


@pytest.fixture(scope="module")
def proj_weights(hip):
    img_C = sum(s[0] for s in hc.PROJ_SHAPES)
    w = hc.proj_weights(9950, img_C, hc.PROJ_H1)
    packed = {prec: hip.prep_mlp_weights({k: dev(v) for k, v in w.items()}, hc.VOX_C, img_C, prec)
              for prec in ("fp16", "bf16x3")}
    return packed, hc.percep_columns(w["fc_0.weight"], img_C)


def from_source(ts, n_kept, precision):
    """list_prep_img_proj's test for k_proj_level_nchw: fp16 operands, every projected level x-contiguous."""
    return precision == "fp16" and all(t.stride(3) == 1 for t in ts[n_kept:])


def check_img_proj(hip, ts, levels, packed, wp, precision, n_kept, tag):
    half = precision == "fp16"
    img = hip.prep_img_proj(ts, packed[precision], hc.PROJ_MS, precision, n_kept_levels=n_kept)
    kept = sum(s[0] for s in hc.PROJ_SHAPES[:n_kept])
    assert img.kept_C == kept
    if kept:                              # the kept channels: prep_img_maps' bit for bit
        plain = hip.prep_img_maps(ts, hc.PROJ_MS, "f16" if half else "f32").data
        bits = torch.int16 if half else torch.int32
        a = img.data[..., :kept].contiguous().view(bits)
        b = plain[..., :kept].contiguous().view(bits)
        assert int((a != b).sum()) == 0, (tag, precision, n_kept)
    ref, bound = hc.proj_reference(levels, wp, hc.PROJ_MS, n_kept, precision)
    wq = hc.worst(img.data[..., kept:].cpu().numpy(), ref, bound, half)
    print(f"img_proj {tag} {precision} n_kept={n_kept}: projected worst error / bound {wq:.3f}")
    assert wq <= 1.0, (tag, precision, n_kept, wq)


@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
@pytest.mark.parametrize("n_kept", [0, 1, 2, 3, 4])
def test_img_proj_from_the_nchw_sources(hip, proj_levels, proj_weights, precision, n_kept):
    """hc.PROJ_SHAPES, B = 2, H1 = 256, ms = 33: 1024 / 256 / 64 / 15 / 4 pixels per image -- 64-pixel tiles that are
    full, partial (15 of 64) and smaller than one 16-row MFMA block (4), K = 64 beside K = 128.  fp16: k_proj_level_nchw,
    launched behind the kept levels' resize without a barrier (the 32 x 32 level in the lane-along-x form, sx = 31 / 32);
    bf16x3: the retained launches (fp32 rows, split, grouped GEMM).  Every projected element meets
    hc.proj_reference's bound, the kept channels are prep_img_maps' bit for bit."""
    packed, wp = proj_weights
    ts = [padded_nchw(m) for m in proj_levels]
    assert [takes_xl(t, hc.PROJ_MS) for t in ts] == [True, False, False, False, False]
    assert from_source(ts, n_kept, precision) == (precision == "fp16")
    check_img_proj(hip, ts, proj_levels, packed, wp, precision, n_kept, "nchw")


def test_img_proj_channels_last_level_keeps_the_two_launches(hip, proj_levels, proj_weights):
    """One channels-last level among the projected ones (the 8 x 8, K = 128 level): list_prep_img_proj keeps
    k_img_level_rows and the grouped GEMM for the whole call; the same bound."""
    packed, wp = proj_weights
    ts = [padded_nchw(m) for m in proj_levels]
    ts[2] = channels_last(dev(proj_levels[2]))
    assert not from_source(ts, 2, "fp16") and from_source(ts, 3, "fp16")
    check_img_proj(hip, ts, proj_levels, packed, wp, "fp16", 2, "level 2 channels-last")
