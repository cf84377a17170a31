"""GPU: the layout hand-off kernels on every dispatch branch, element by element against the float64 references and the
derived bounds of tests/_handoff_check.py -- the 2-D resize (prep_kernels.hip: k_prep_img, k_prep_img_tile<0/1>,
k_prep_img_nhwc<0/1>, k_prep_img_rows<0/1> in its three load forms), the adjoint resize (bwd_img_kernels.hip:
k_img_grad_level<0>), the voxel transposes (k_transpose_vox, the fused tile launch, the elementwise conversion) and the
projected perceptual map (k_img_level_rows<0/1>, the grouped projection, k_proj_resize_sum for one to five levels).
Every element of every output is compared; every test prints its worst error / bound (a record, not a tolerance)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _handoff_check as hc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date
    from list_amd import hip as h
    h.load()
    return h


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def as_form(t, form):
    """nchw: dense; nhwc: channels-last (sc == 1); wh: a [B,C,W,H].transpose(2,3) view (sw == H, sc == W * H)."""
    if form == "nchw":
        return t.contiguous()
    if form == "nhwc":
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert form == "wh"
    if t.shape[2] == 1 and t.shape[3] > 1:                      # (the transposed view of one row is dense: every other column)
        return torch.repeat_interleave(t, 2, dim=3)[..., ::2]
    return t.transpose(2, 3).contiguous().transpose(2, 3)


# ---------------------------------------------------------------------------------------------- 1. the 2-D resize
# run -> (case of _handoff_check.RESIZE_CASES, source form, channels the last level is cut to).  The branch each run takes,
# read from launch_prep_img's conditions (prep_kernels.hip):
RESIZE_RUNS = {
    # every level C % 64 == 0 -> k_prep_img_rows in ONE launch; dense NCHW: sw == 1, W >= 2, sc != 1 -> `pair` loads.
    # 224 -> 137 down-samples (RY = 2), 14 -> 137 up-samples (RY = 32), 28 x 20 and 14 x 9 are not square, 137 % 16 = 9
    "R1": ("R1", "nchw", None),
    # channels-last: sc == 1, sw = C, sh, sb multiples of 4, 16-byte aligned -> `vec` loads
    "R2": ("R1", "nhwc", None),
    # transposed views: sw = H != 1 and sc = W * H != 1 -> neither vec nor pair: the plain strided loads
    "R3": ("R1", "wh", None),
    # the same with (64, 5, 1), (64, 1, 7), (64, 1, 1) levels: H == 1, W == 1
    "R3b": ("R3b", "wh", None),
    # last level 32 channels: rows_eligible fails -> no level takes the rows kernel; NCHW, C % 32 == 0, sw == 1 ->
    # k_prep_img_tile on every level (RY = 8 at 14 px; XS = 4, RY = 1 at 224 px); fp32 output <0>, fp16 output <1>
    "R4": ("R1", "nchw", 32),
    # the same channels-last: sc == 1, C % 8 == 0 -> k_prep_img_nhwc<0/1> on every level
    "R5": ("R1", "nhwc", 32),
    # channels (24, 40, 8, 36, 20): no C % 32 == 0, NCHW -> the generic k_prep_img, partial channel groups (40 = 32 + 8)
    "R6": ("R6", "nchw", None),
    # channels-last: fp32 output k_prep_img_nhwc<0> (C % 4 == 0); fp16 output: the nhwc kernel declines 36 and 20
    # (C % 8 != 0), the tile kernel too (sw != 1) -> generic k_prep_img on strided channels-last sources
    "R6cl": ("R6", "nhwc", None),
    # map-size limits: ms = 2 (rows kernel; generic kernel), ms = 320 = kResizeMaxMs (rows kernel with a 320^2 identity
    # level; generic kernel with its LDS tile full), ms = 274 with a (64, 512, 300) level
    "R7_ms2": ("R7_ms2", "nchw", None),
    "R7_ms2_generic": ("R7_ms2_generic", "nchw", None),
    "R7_ms320": ("R7_ms320", "nchw", None),
    "R7_ms320_generic": ("R7_ms320_generic", "nchw", None),
    "R7_ms274": ("R7_ms274", "nchw", None),
    # ... and a 32-channel neighbour: per-level fallback, the 512 x 300 level fails the tile kernel's 32 KB LDS test at
    # every XS (3 rows x 78 columns x 36 floats at XS = 4) and reaches the generic k_prep_img
    "R7_ms274_fallback": ("R7_ms274", "nchw", 32),
}


def resize_sources(run):
    case, form, cut = RESIZE_RUNS[run]
    levels, ms = hc.resize_case(case)
    ts = [dev(m) for m in levels]
    if cut is not None:
        ts[-1] = ts[-1][:, :cut]
    ts = [as_form(t, form) for t in ts]
    if form == "wh":                                          # launch_prep_img's `vec` and the kernel's `pair`, both false
        for t in ts:
            vec = t.stride(1) == 1 and all(t.stride(d) % 4 == 0 for d in (0, 2, 3))
            assert not vec and not (t.stride(3) == 1 and t.shape[3] >= 2), (t.shape, t.stride())
    if form == "nhwc":
        assert all(t.stride(1) == 1 for t in ts)
    return ts, ms


def resize_run(hip, run, md):
    ts, ms = resize_sources(run)
    return hip.prep_img_maps(ts, ms, md).data


def judge_resize(got, run, half):
    """Worst error / bound over every element of a prep_img_maps output."""
    case, _, cut = RESIZE_RUNS[run]
    levels, _ = hc.resize_case(case)
    coff, w = 0, 0.0
    for i, m in enumerate(levels):
        ref, bound = hc.resize_case_reference(case, i)
        Cl = m.shape[1] if (cut is None or i < len(levels) - 1) else cut
        w = max(w, hc.worst(got[..., coff:coff + Cl], ref[..., :Cl], bound[..., :Cl], half))
        coff += Cl
    assert coff == got.shape[-1]
    return w


@pytest.mark.parametrize("md", ["f32", "f16"])
@pytest.mark.parametrize("run", list(RESIZE_RUNS))
def test_resize_meets_the_bound_per_element(hip, run, md):
    got = resize_run(hip, run, md).cpu().numpy()
    w = judge_resize(got, run, md == "f16")
    print(f"resize {run} {md}: worst error / bound {w:.3f}")
    assert w <= 1.0, (run, md, w)


@pytest.mark.parametrize("md", ["f32", "f16"])
def test_resize_kernels_agree_bit_for_bit(hip, md):
    """The slice of a level in the output does not depend on the other levels, and every kernel evaluates ATen's form
    in the same order op by op ("same bits as k_prep_img"): levels 0 to 3 of R1 .. R5 are identical bit for bit, the
    planted NaN, infinities and saturating values included."""
    bits = torch.int32 if md == "f32" else torch.int16
    kept = sum(s[0] for s in hc.R1_SHAPES[:4])
    base = resize_run(hip, "R1", md)[..., :kept].contiguous().view(bits)
    for run in ("R2", "R3", "R4", "R5"):
        other = resize_run(hip, run, md)[..., :kept].contiguous().view(bits)
        diff = int((base != other).sum())
        print(f"resize {run} against R1, {md}: {diff} of {base.numel()} elements differ")
        assert diff == 0, (run, md, diff)


# ---------------------------------------------------------------------------------------------- 2. the adjoint resize
def adjoint_run(hip, G, shapes, form, null_level=None):
    """list_img_map_grad_to_levels through ctypes into NaN-filled destinations (a workgroup that does not write shows)."""
    B, ms = G.shape[0], G.shape[1]
    outs = [as_form(torch.full((B, Cl, H, W), float("nan"), device=DEV), form) for (Cl, H, W) in shapes]
    maps = hip._map2d_descriptors(outs)
    if null_level is not None:
        maps[null_level].data = None
    with torch.cuda.device(G.device):
        rc = hip.load().list_img_map_grad_to_levels(G.data_ptr(), B, ms, maps, hip._stream())
    assert rc == 0, hip._last_error()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("form", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(hc.ADJOINT_CASES))
def test_adjoint_resize_meets_the_bound_per_element(hip, name, form):
    """k_img_grad_level<0>: every level of every case (see _handoff_check.ADJOINT_CASES for what each one reaches),
    dense and channels-last destinations; untouched source rows and columns hold exact zeros (bound 0)."""
    G, shapes = hc.adjoint_case(name)
    outs = adjoint_run(hip, dev(G), shapes, form)
    coff = 0
    for (Cl, H, W), got in zip(shapes, outs):
        ref, bound = hc.adjoint_reference(G, Cl, H, W, coff)
        w = hc.worst(got, ref, bound)
        zeros = int((bound == 0).sum())
        print(f"adjoint {name} {form} ({Cl}, {H}, {W}): worst error / bound {w:.3f}, {zeros} exact zeros demanded")
        assert w <= 1.0, (name, form, Cl, H, W, w)
        coff += Cl


def test_adjoint_leaves_a_null_level_out(hip):
    """A descriptor with data = NULL is skipped: its (NaN-filled) tensor is untouched, the others are unchanged."""
    G, shapes = hc.adjoint_case("A_ms137")
    Gd = dev(G)
    full = adjoint_run(hip, Gd, shapes, "nchw")
    part = adjoint_run(hip, Gd, shapes, "nchw", null_level=1)
    for i, (a, b) in enumerate(zip(full, part)):
        if i == 1:
            assert np.isnan(b).all()
        else:
            assert np.array_equal(a, b), i


# ---------------------------------------------------------------------------------------------- 3. the voxel hand-off
def vox_sources(shapes, B, seed, specials):
    out = []
    for i, (Cl, D, H, W) in enumerate(shapes):
        m = synth.uniform(seed, (B, Cl, D, H, W)) if Cl == 1 else synth.normalish(seed + i, (B, Cl, D, H, W))
        if specials:
            n = min(Cl, len(hc.SPECIALS))
            m[B - 1, :n, D // 2, H - 1, W // 2] = hc.SPECIALS[:n]
            m[0, Cl - 1, 0, 0, 0] = np.float32(-70000.0)
        out.append(m)
    return out


def check_vox_pack(hip, vox, sources, srcs_np, md, in_place=()):
    """Read the pack back (offsets aligned to 256 bytes, levels used in place take no room) and compare bit for bit."""
    pack = vox._keep[0]
    raw = pack.view(torch.uint8).cpu().numpy()
    off = 0
    for l, (t, m) in enumerate(zip(sources, srcs_np)):
        lv = vox.levels[l]
        B, Cl, D, H, W = m.shape
        assert (lv.C, lv.D, lv.H, lv.W) == (Cl, D, H, W)
        if l in in_place:
            assert lv.data == t.data_ptr() and lv.image_stride == t.stride(0), l
            continue
        f16 = md == "f16" and Cl != 1 and Cl % 8 == 0             # the scalar level (and C % 8 != 0) stays fp32
        assert lv.dtype == (hip.MAP_F16 if f16 else hip.MAP_F32), l
        assert lv.data == pack.data_ptr() + off, l
        n = B * Cl * D * H * W
        nbytes = n * (2 if f16 else 4)
        got = raw[off:off + nbytes].view(np.float16 if f16 else np.float32).reshape(B, D, H, W, Cl)
        assert hc.same_bits(got, hc.vox_expected(m, f16)), (l, m.shape, md)
        off += (nbytes + 255) // 256 * 256


FUSED_SHAPES = [(c, 8, 8, 8) for c in hc.VOX_C]
GENERIC_SHAPES = [(c, 3, 5, 7) for c in (1, 8, 24, 136, 16, 260)]


@pytest.mark.parametrize("md", ["f32", "f16"])
def test_vox_fused_tile_launch(hip, md):
    """Channels (1, 16, 32, 64, 128, 128) at 8^3, B = 3: dense fp32, C in {16, 32, 64, 128}, 512 % (2048 / C) == 0 -> all
    five vector levels are tile-eligible: ONE k_transpose_vox_fused launch with every transpose_vox_tile<C> width, its
    fp32 and its fp16 store; the dense scalar level is used in place."""
    src = vox_sources(FUSED_SHAPES, 3, 9100, specials=True)
    ts = [dev(m) for m in src]
    check_vox_pack(hip, hip.prep_vox_maps(ts, md), ts, src, md, in_place=(0,))


@pytest.mark.parametrize("md", ["f32", "f16"])
@pytest.mark.parametrize("half_source", [False, True])
def test_vox_generic_kernel(hip, md, half_source):
    """3 x 5 x 7 levels (nvox = 105, not a multiple of 64) of channels (1, 8, 24, 136, 16, 260): not tile-eligible ->
    k_transpose_vox, C > 128 in c_begin chunks (136 = 128 + 8, 260 = 128 + 128 + 4); fp32 and fp16 sources (a scalar
    fp16 level is converted, not used in place); put_map's fp32 and saturating fp16 store."""
    src = vox_sources(GENERIC_SHAPES, 2, 9200, specials=not half_source)
    if half_source:
        src = [m.astype(np.float16) for m in src]
        for m in src:
            m[1, 0, 1, 2, 3], m[0, 0, 2, 4, 6], m[1, -1, 0, 0, 0] = np.inf, -np.inf, np.nan
    ts = [dev(m) for m in src]
    check_vox_pack(hip, hip.prep_vox_maps(ts, md), ts, src, md, in_place=() if half_source else (0,))


@pytest.mark.parametrize("md", ["f32", "f16"])
def test_vox_strided_sources(hip, md):
    """Batch- and channel-sliced sources (the strides of test_odd_shapes_take_the_general_paths): at 8^3 the channel
    slices stay tile-eligible with sc != D*H*W's dense sb (fused launch on strided bases), at 3 x 5 x 7 they take
    k_transpose_vox; the batch-sliced scalar level is still dense per image and used in place."""
    for shapes, seed in ((FUSED_SHAPES, 9300), (GENERIC_SHAPES[:5] + [(128, 3, 5, 7)], 9400)):
        src = vox_sources(shapes, 2, seed, specials=True)
        ts = [torch.cat([dev(m), dev(m)], 0)[:2] if m.shape[1] == 1 else torch.cat([dev(m), dev(m)], 1)[:, :m.shape[1]]
              for m in src]
        assert all(not t.is_contiguous() for t in ts[1:])
        check_vox_pack(hip, hip.prep_vox_maps(ts, md), ts, src, md, in_place=(0,))


def test_vox_channels_last_sources(hip):
    """Dense channels-last fp32 levels.  fp32 maps: used in place (pointer equality).  fp16 maps: the 128-channel levels
    (at most 31 voxels a side) are CONVERTED elementwise (launch_split, FMT_FP16), the others stay in place in fp32.
    A channels-last 128-channel level whose images are not dense (a batch slice: sb != vol * C) is refused by the
    elementwise conversion and transposed with sc == 1 by k_transpose_vox."""
    src = vox_sources(GENERIC_SHAPES[:4] + [(128, 3, 5, 7), (128, 2, 3, 1)], 2, 9500, specials=True)
    cl = [dev(m).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3) for m in src]
    cl[0] = dev(src[0])
    vox = hip.prep_vox_maps(cl, "f32")
    check_vox_pack(hip, vox, cl, src, "f32", in_place=range(6))
    vox = hip.prep_vox_maps(cl, "f16")
    assert all(vox.levels[l].dtype == hip.MAP_F32 for l in range(4))
    check_vox_pack(hip, vox, cl, src, "f16", in_place=range(4))
    # (B * vol * C % 4 != 0 cannot occur in that branch: fp16 levels have C % 8 == 0; the reachable refusal is sb)
    gap = [t for t in cl]
    big = torch.cat([cl[4].permute(0, 2, 3, 4, 1), cl[4].permute(0, 2, 3, 4, 1)], 1).contiguous()   # [B, 2D, H, W, C]
    gap[4] = big[:, :3].permute(0, 4, 1, 2, 3)
    assert gap[4].stride(1) == 1 and gap[4].stride(0) == 2 * 105 * 128
    vox = hip.prep_vox_maps(gap, "f16")
    check_vox_pack(hip, vox, gap, src, "f16", in_place=range(4))


# ---------------------------------------------------------------------------------------------- 4. the projected map
def judge_proj(got, levels, wp, ms, n_kept, precision, tag):
    half = precision == "fp16"
    coff, wk = 0, 0.0
    for m in levels[:n_kept]:                                  # channels [0, kept_C): the plain resize, as in part 1
        ref, bound = hc.resize_reference(m, ms)
        wk = max(wk, hc.worst(got[..., coff:coff + m.shape[1]], ref, bound, half))
        coff += m.shape[1]
    ref, bound = hc.proj_reference(levels, wp, ms, n_kept, precision)
    assert got.shape[-1] == coff + ref.shape[-1]
    wp_ = hc.worst(got[..., coff:], ref, bound, half)
    print(f"img_proj {tag} {precision} n_kept={n_kept}: worst error / bound kept {wk:.3f}, projected {wp_:.3f}")
    assert wk <= 1.0 and wp_ <= 1.0, (tag, precision, n_kept, wk, wp_)


def proj_setup(hip, levels, H1, precision, seed):
    img_C = sum(m.shape[1] for m in levels)
    w = hc.proj_weights(seed, img_C, H1)
    packed = hip.prep_mlp_weights({k: dev(v) for k, v in w.items()}, hc.VOX_C, img_C, precision)
    return packed, hc.percep_columns(w["fc_0.weight"], img_C)


@pytest.fixture(scope="module")
def proj_levels():
    return hc.make_levels(8500, hc.PROJ_B, hc.PROJ_SHAPES)


@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
@pytest.mark.parametrize("n_kept", [0, 1, 2, 3, 4])
def test_img_proj_every_number_of_kept_levels(hip, proj_levels, precision, n_kept):
    """H1 = 256, channels (64, 64, 128, 64, 64) at 32^2 .. 2^2, ms = 33, B = 3: k_proj_resize_sum<F16, NL, SRC16> for
    NL = 5 - n_kept, k_img_level_rows<0/1>, the grouped ping-pong GEMM with K = 64 groups beside K = 128 and partial last
    256-row tiles (3 * 64, 3 * 15, 3 * 4 rows), k_prep_img_rows on the kept levels (all C % 64 == 0)."""
    packed, wp = proj_setup(hip, proj_levels, hc.PROJ_H1, precision, 8600)
    img = hip.prep_img_proj([dev(m) for m in proj_levels], packed, hc.PROJ_MS, precision, n_kept_levels=n_kept)
    assert img.kept_C == sum(s[0] for s in hc.PROJ_SHAPES[:n_kept])
    judge_proj(img.data.cpu().numpy(), proj_levels, wp, hc.PROJ_MS, n_kept, precision, "small")


@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
def test_img_proj_channels_last_levels(hip, proj_levels, precision):
    """Channels-last sources: k_img_level_rows reads along the channels, the kept levels take the rows kernel's vec loads;
    the result is the NCHW one bit for bit (the same operands reach the same kernels)."""
    packed, wp = proj_setup(hip, proj_levels, hc.PROJ_H1, precision, 8600)
    cl = [as_form(dev(m), "nhwc") for m in proj_levels]
    img = hip.prep_img_proj(cl, packed, hc.PROJ_MS, precision, n_kept_levels=2)
    judge_proj(img.data.cpu().numpy(), proj_levels, wp, hc.PROJ_MS, 2, precision, "channels-last")
    ref = hip.prep_img_proj([dev(m) for m in proj_levels], packed, hc.PROJ_MS, precision, n_kept_levels=2)
    bits = torch.int16 if precision == "fp16" else torch.int32
    assert torch.equal(img.data.view(bits), ref.data.view(bits))


@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
def test_img_proj_default_encoder_channels(hip, precision):
    """The encoder's channels (64, 64, 128, 256, 512) at 64 px, H1 = 512, ms = 137, the default number of kept levels
    (0: every level is enlarged at least 2 x 2): K up to 512, five source levels."""
    levels = synth.make_img_maps(8700, 1, 64)
    packed, wp = proj_setup(hip, levels, 512, precision, 8800)
    ts = [dev(m) for m in levels]
    n_kept = hip.img_proj_kept_levels(ts, 137)
    img = hip.prep_img_proj(ts, packed, 137, precision)
    assert img.data.shape[-1] == sum(m.shape[1] for m in levels[:n_kept]) + 512
    judge_proj(img.data.cpu().numpy(), levels, wp, 137, n_kept, precision, "default")


@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
def test_percep_proj_is_one_product_on_the_prepared_map(hip, proj_levels, precision):
    """list_prep_percep_proj: out[pixel][n] = sum_c map[pixel][c] W0[n][c] on the prepared map the device itself made
    (own-input rule), K = 384, 3 * 33^2 = 3267 rows (a partial last 256-row tile)."""
    half = precision == "fp16"
    packed, wp = proj_setup(hip, proj_levels, hc.PROJ_H1, precision, 8600)
    img = hip.prep_img_maps([dev(m) for m in proj_levels], hc.PROJ_MS, hip.map_dtype_for(precision))
    out = hip.prep_percep_proj(img, packed, precision).data
    px = hc.PROJ_B * hc.PROJ_MS * hc.PROJ_MS
    got = out.view(torch.float16 if half else torch.float32)[:px * hc.PROJ_H1].reshape(px, hc.PROJ_H1).cpu().numpy()
    a = img.data.cpu().numpy().reshape(px, -1).astype(np.float32)
    P, e = hc.gemm_reference(a, wp, precision, half)
    w = hc.worst(got, P, e)
    print(f"percep_proj {precision}: worst error / bound {w:.3f}")
    assert w <= 1.0, (precision, w)
