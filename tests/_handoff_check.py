"""The per-element check of the layout hand-off kernels (prep_kernels.hip: the 2-D resize, the voxel transposes, the
projected perceptual map; bwd_img_kernels.hip: the adjoint resize), shared by test_handoff_cpu.py (which applies it to
numpy fp32 restatements and to deliberately wrong ones) and test_handoff_gpu.py (which applies it to every dispatch branch
of the device).  Plain numpy; no GPU here.

Indices and weights are ATen's (upsample_bilinear2d, align_corners), evaluated in numpy float32 exactly as adj_footprint
and k_prep_img write them, every step one IEEE operation:
    sc = f32(S-1) / f32(ms-1);  f = sc * f32(o);  i0 = min(int(f), S-1);  i1 = i0 + (i0 < S-1);
    w1 = f - f32(i0);  w0 = f32(1) - w1.
The interpolation itself is evaluated in float64 from those fp32 weights in the FOUR-TAP GATHER form (a dense weight
matrix would multiply an infinity by the zeros of the taps it does not use).  With u = 2^-24, the library being built
with -ffp-contract=off (device fp32 arithmetic is op by op):

  resize        every tap passes through at most four fp32 roundings (product, sum, product, sum):
                4.5 u S with S = sum |v_ij| wx_i wy_j, + 4 * 2^-149 for subnormal products.
  fp16 output   + half an fp16 ulp of the reference: 2^-11 |ref|, at least 2^-25 (the subnormal halfs).  Where
                |ref| - bound > 65504 the result must be exactly +-65504 (the library's saturating conversion, sat_h).
                A NaN meets a NaN; in fp32 an infinity meets the same infinity, in fp16 an infinity is +-65504.
  adjoint       out[ys,xs] = sum_oy sum_ox wy(oy,ys) wx(ox,xs) G[oy,ox]; a tap with i0 == i1 carries w0 + w1.  The kernel
                runs two explicit fmaf chains, of n_y(ys) map rows and n_x(xs) map columns that touch the source row and
                column: (n_y + n_x + 2) u sum |wy| |wx| |G| (the 2: the fp32 sums w0 + w1).  A source row or column that
                no map pixel touches has bound 0: exact zeros.
  transposes    exact: bit for bit in fp32; the saturating RNE half of the value in fp16 (NaN stays NaN, +-inf and
                +-70000 become +-65504, 65520 becomes 65504).
  projection    P_l = rows_l W0[:, cols_l]^T on the device's own operands (own-input rule):
                fp16    operands = the saturating RNE halfs of the levels and of fc_0.weight; their products are exact in
                        fp32; accumulation (K_l + 2) c u sum |a| |w| with c = 2, the allowance _voxenc_check.py fixes for
                        the matrix cores' internal order; P_l is stored as a half: + max(2^-11 |P_l|, 2^-25).
                bf16x3  operands = hi + lo (hi the RNE bf16, lo the RNE bf16 of the remainder); the three products drop
                        lo * lo: + sum |lo_a| |lo_w|; accumulation (3 K_l + 2) c u sum |a| |w|; P_l is fp32.
                The error of P_l is carried through the resize's (non-negative) weights; the resize and the level sum add
                (4.5 + NL) u S with S = sum_l sum |P_l| wx wy (NL levels: four roundings per tap and one per added level);
                the final half rounding follows as for the plain resize.
No measured tolerance anywhere."""
import numpy as np

from oracle import synth

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
F16_MAX = 65504.0
TINY = 4 * 2.0 ** -149
MXU_C = 2                     # tests/_voxenc_check.py's allowance for the matrix cores' internal order


# ---------------------------------------------------------------------------------------------- formats
def sat_half(x):
    """The library's fp32 -> fp16 store (sat_h + v_cvt_f16_f32): clamp to +-65504, round to nearest even, NaN stays."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        return np.clip(x, F32(-F16_MAX), F32(F16_MAX)).astype(np.float16)       # (np.clip propagates a NaN)


def bf16_rne(x):
    """fp32 -> the fp32 value of its round-to-nearest-even bf16 (finite input)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return (r & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(F32).reshape(np.shape(x))


def split_bf16(x):
    """(hi, lo) of the library's split4: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32)."""
    x = np.asarray(x, F32)
    hi = bf16_rne(x)
    return hi, bf16_rne((x - hi).astype(F32))


# ---------------------------------------------------------------------------------------------- footprints
def axis(S, ms):
    """(i0, i1, w0, w1) of the ms map indices on a source axis of S pixels: fp32, one IEEE operation per step."""
    sc = F32(S - 1) / F32(ms - 1) if ms > 1 else F32(0)
    f = (sc * np.arange(ms, dtype=F32)).astype(F32)
    i0 = np.minimum(f.astype(np.int64), S - 1)
    i1 = i0 + (i0 < S - 1)
    w1 = (f - i0.astype(F32)).astype(F32)
    w0 = (F32(1) - w1).astype(F32)
    return i0, i1, w0, w1


def _gather4(v, ms):
    """v [B,C,H,W] float64 -> [B,C,ms,ms]: the four-tap form in float64 from the fp32 weights."""
    y0, y1, wy0, wy1 = axis(v.shape[2], ms)
    x0, x1, wx0, wx1 = axis(v.shape[3], ms)
    wy0, wy1 = wy0.astype(F64)[:, None], wy1.astype(F64)[:, None]
    wx0, wx1 = wx0.astype(F64), wx1.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        r0, r1 = v[:, :, y0], v[:, :, y1]
        top = r0[..., x0] * wx0 + r0[..., x1] * wx1
        bot = r1[..., x0] * wx0 + r1[..., x1] * wx1
        return top * wy0 + bot * wy1


def resize_reference(x, ms):
    """x [B,C,H,W] fp32 (NaN, infinities allowed) -> (ref, bound) float64, channels-last [B,ms,ms,C]: the fp32 bound
    4.5 u S + 4 * 2^-149 (0 where S is not finite: there ref is a NaN or an infinity and must meet its like)."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 4
    v = x.astype(F64)
    ref = _gather4(v, ms)
    S = _gather4(np.abs(v), ms)
    bound = np.where(np.isfinite(S), 4.5 * U24 * np.where(np.isfinite(S), S, 0.0) + TINY, 0.0)
    return np.ascontiguousarray(ref.transpose(0, 2, 3, 1)), np.ascontiguousarray(bound.transpose(0, 2, 3, 1))


def ratios(got, ref, bound, half):
    """error / bound of every element (float64).  half: the output is fp16 -- `bound` is the fp32 bound, the half
    rounding and the saturation rule are added here.  inf where a NaN, an infinity or a saturated value does not meet
    what it must."""
    got = np.asarray(got).astype(F64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fin = np.isfinite(ref)
        b = np.where(np.isfinite(bound), bound, 0.0)
        if half:
            b = b + np.maximum(2.0 ** -11 * np.where(fin, np.abs(ref), 0.0), 2.0 ** -25)
        err = np.abs(got - ref)
        q = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
        q = np.where(fin & np.isfinite(got), q, np.inf)
        q = np.where(np.isnan(ref), np.where(np.isnan(got), 0.0, np.inf), q)
        if half:
            sat = np.isinf(ref) | (fin & (np.abs(ref) - b > F16_MAX))
            q = np.where(sat, np.where(got == np.sign(ref) * F16_MAX, 0.0, np.inf), q)
        else:
            q = np.where(np.isinf(ref), np.where(got == ref, 0.0, np.inf), q)
    return q


def worst(got, ref, bound, half=False):
    q = ratios(got, ref, bound, half)
    return float(q.max()) if q.size else 0.0


# ---------------------------------------------------------------------------------------------- adjoint resize
def _adj_matrix(S, ms):
    """[ms,S] float64: map index o carries w0 on i0 and w1 on i1 (w0 + w1 where they coincide); n [S]: map indices
    that touch each source index."""
    i0, i1, w0, w1 = axis(S, ms)
    M = np.zeros((ms, S), F64)
    o = np.arange(ms)
    np.add.at(M, (o, i0), w0.astype(F64))
    np.add.at(M, (o, i1), w1.astype(F64))
    hit = np.zeros((ms, S), bool)
    hit[o, i0] = True
    hit[o, i1] = True
    return M, hit.sum(0)


def adjoint_reference(G, C, H, W, coff):
    """G [B,ms,ms,Ct] fp32 (finite) -> (ref, bound) float64 [B,C,H,W] of the level at channel offset coff."""
    G = np.asarray(G)
    B, ms = G.shape[0], G.shape[1]
    g = G[..., coff:coff + C].astype(F64)
    My, ny = _adj_matrix(H, ms)
    Mx, nx = _adj_matrix(W, ms)

    def apply(a, my, mx):
        r = np.einsum("oy,bopc->bypc", my, a, optimize=True)
        return np.einsum("px,bypc->bcyx", mx, r, optimize=True)
    ref = apply(g, My, Mx)
    A = apply(np.abs(g), np.abs(My), np.abs(Mx))
    n = (ny[:, None] + nx[None, :] + 2).astype(F64)
    touched = (ny[:, None] > 0) & (nx[None, :] > 0)
    return ref, np.where(touched, n * U24 * A, 0.0)


# ---------------------------------------------------------------------------------------------- voxel transposes
def vox_expected(src, as_f16):
    """src [B,C,D,H,W] fp32 or fp16 -> the channels-last level the library must hold, bit for bit."""
    t = np.ascontiguousarray(np.transpose(np.asarray(src), (0, 2, 3, 4, 1)))
    return sat_half(t.astype(F32)) if as_f16 else t.astype(F32)


def same_bits(got, want):
    """Bit for bit, any NaN meeting any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    nan = np.isnan(got) & np.isnan(want)
    return bool(np.all((np.ascontiguousarray(got).view(bits) == np.ascontiguousarray(want).view(bits)) | nan))


# ---------------------------------------------------------------------------------------------- projected map
def percep_columns(w0, img_C):
    """The perceptual block of fc_0.weight [H1,F(,1)]: the reference's feature order is voxels | image | xyz."""
    w0 = np.asarray(w0, F32).reshape(w0.shape[0], -1)
    F = w0.shape[1]
    return np.ascontiguousarray(w0[:, F - 3 - img_C:F - 3])


def level_rows(m):
    """[B,C,H,W] -> [B,H,W,C]"""
    return np.ascontiguousarray(np.transpose(m, (0, 2, 3, 1)))


def gemm_reference(a, w, precision, out_half):
    """a [..,K], w [N,K] fp32: the device's own operands of `precision` -> (P, e) float64: the product and its bound,
    the half store of the result included when out_half."""
    K = a.shape[-1]
    if precision == "fp16":
        ao, wo = sat_half(a).astype(F64), sat_half(w).astype(F64)
        drop, terms = 0.0, 1
    else:
        (ah, al), (wh, wl) = split_bf16(a), split_bf16(w)
        ao, wo = ah.astype(F64) + al.astype(F64), wh.astype(F64) + wl.astype(F64)
        drop, terms = np.abs(al.astype(F64)) @ np.abs(wl.astype(F64)).T, 3
    P = ao @ wo.T
    e = (terms * K + 2) * MXU_C * U24 * (np.abs(ao) @ np.abs(wo).T) + drop
    if out_half:
        e = e + np.maximum(2.0 ** -11 * np.abs(P), 2.0 ** -25)
    return P, e


def proj_reference(levels, wp, ms, n_kept, precision):
    """levels: five [B,C,H,W] fp32 (finite); wp: percep_columns(fc_0.weight) [H1,img_C] -> (ref, bound) float64
    [B,ms,ms,H1] of the projected channels, before the output's own half rounding (ratios(half=True) adds it)."""
    half = precision == "fp16"
    coff = sum(m.shape[1] for m in levels[:n_kept])
    ref = E = S = 0.0
    NL = len(levels) - n_kept
    for m in levels[n_kept:]:
        C = m.shape[1]
        P, e = gemm_reference(level_rows(m), wp[:, coff:coff + C], precision, half)      # [B,H,W,H1]
        P, e = P.transpose(0, 3, 1, 2), e.transpose(0, 3, 1, 2)
        ref = ref + _gather4(P, ms)
        E = E + _gather4(e, ms)
        S = S + _gather4(np.abs(P), ms)
        coff += C
    bound = E + (4.5 + NL) * U24 * S + TINY
    return np.ascontiguousarray(ref.transpose(0, 2, 3, 1)), np.ascontiguousarray(bound.transpose(0, 2, 3, 1))


# ---------------------------------------------------------------------------------------------- the cases
# values no finite-arithmetic test sees: NaN, infinities, beyond the fp16 range, the RNE overflow threshold, subnormals
SPECIALS = np.array([np.nan, np.inf, -np.inf, 70000.0, -70000.0, 65520.0, 2.0 ** -149, -2.0 ** -130, 1.5 * 2.0 ** -127], F32)


def plant_specials(x):
    """Every channel of x [B,C,H,W] gets one special value: at the weight-0 tap of map pixel (0, 0) (a grid-aligned
    pixel), at the bottom-right corner and on the bottom edge (i1 == i0), or at an interior tap."""
    B, C, H, W = x.shape
    pos = [(0, min(1, W - 1)), (H - 1, W - 1), (H // 2, W // 2), (H - 1, W // 3)]
    for b in range(B):
        for c in range(C):
            k = c + 4 * b
            y, xx = pos[(k // len(SPECIALS)) % len(pos)]
            x[b, c, y, xx] = SPECIALS[k % len(SPECIALS)]
    return x


def make_levels(seed, B, shapes, specials=False):
    out = []
    for i, (C, H, W) in enumerate(shapes):
        m = synth.normalish(seed + 7 * i, (B, C, H, W))
        out.append(plant_specials(m) if specials else m)
    return out


R1_SHAPES = [(64, 224, 224), (64, 112, 112), (128, 56, 56), (64, 28, 20), (64, 14, 9)]
R6_SHAPES = [(24, 50, 46), (40, 25, 23), (8, 224, 224), (36, 7, 6), (20, 4, 3)]
# name -> (B, ms, level shapes (C,H,W), special values planted)
RESIZE_CASES = {
    "R1": (2, 137, R1_SHAPES, True),
    "R3b": (2, 137, [(64, 5, 1), (64, 1, 7), (64, 1, 1), (64, 2, 9), (64, 9, 2)], False),
    "R6": (2, 137, R6_SHAPES, True),
    "R7_ms2": (1, 2, [(64, 224, 224), (64, 5, 1), (64, 1, 7), (64, 2, 2), (64, 14, 9)], False),
    "R7_ms2_generic": (1, 2, R6_SHAPES, False),
    "R7_ms320": (1, 320, [(64, 320, 320), (64, 2, 3), (64, 14, 9), (64, 5, 1), (64, 1, 7)], False),
    "R7_ms320_generic": (1, 320, [(24, 2, 3), (40, 50, 46), (8, 320, 320), (36, 7, 6), (20, 1, 1)], False),
    "R7_ms274": (1, 274, [(64, 512, 300), (64, 2, 2), (64, 14, 9), (64, 28, 20), (64, 5, 5)], False),
}
_SEEDS = {n: 7000 + 100 * i for i, n in enumerate(RESIZE_CASES)}
_levels, _refs = {}, {}


def resize_case(name):
    """(levels, ms) of a named case, built once."""
    if name not in _levels:
        B, ms, shapes, specials = RESIZE_CASES[name]
        _levels[name] = (make_levels(_SEEDS[name], B, shapes, specials), ms)
    return _levels[name]


def resize_case_reference(name, level):
    """(ref, bound) of one level of a named case, computed once and shared (read-only)."""
    key = (name, level)
    if key not in _refs:
        levels, ms = resize_case(name)
        r, b = resize_reference(levels[level], ms)
        r.setflags(write=False)
        b.setflags(write=False)
        _refs[key] = (r, b)
    return _refs[key]


# adjoint: name -> (B, ms, level shapes).  Channels (8, 36, 4, 64, 12): partial 32-channel groups (8, 36 = 32 + 4, 4, 12)
ADJOINT_CASES = {
    # 224 -> 137 (down-sampled, W > 128: two passes), 14 -> 137, 512 -> 137 (272 of 512 rows touched, four passes),
    # 137 -> 137, (C, 5, 1)
    "A_ms137": (2, 137, [(8, 224, 224), (36, 14, 14), (4, 512, 512), (64, 137, 137), (12, 5, 1)]),
    # 512 x 300 -> 274 (three passes), (C, 1, 7), (C, 5, 1), up-sampling by 20
    "B_ms274": (1, 274, [(8, 512, 300), (36, 1, 7), (4, 5, 1), (64, 14, 14), (12, 3, 2)]),
    # 3 x 2 -> 320: 319 columns land on one source column, maxper is capped at ms; 320 -> 320 (more than 64 KB of LDS)
    "C_ms320": (1, 320, [(8, 3, 2), (36, 2, 3), (4, 320, 320), (64, 14, 9), (12, 1, 1)]),
    # ms = 2: only the first and the last source row / column are touched
    "D_ms2": (2, 2, [(8, 3, 2), (36, 1, 7), (4, 5, 1), (64, 2, 2), (12, 14, 14)]),
}


def adjoint_case(name):
    B, ms, shapes = ADJOINT_CASES[name]
    Ct = sum(s[0] for s in shapes)
    return synth.normalish(8100 + 10 * list(ADJOINT_CASES).index(name), (B, ms, ms, Ct)), shapes


# projected map: H1 = 256, ms = 33, B = 3: the projected levels' rows (3 * 64, 3 * 15, 3 * 4 ...) leave the last 256-row
# tile partial, a K = 64 group sits beside K = 128
PROJ_SHAPES = [(64, 32, 32), (64, 16, 16), (128, 8, 8), (64, 5, 3), (64, 2, 2)]
PROJ_B, PROJ_MS, PROJ_H1 = 3, 33, 256
VOX_C = (1, 16, 32, 64, 128, 128)


def proj_weights(seed, img_C, H1):
    """synth.make_mlp_weights for a feature vector with img_C perceptual channels; H1 = 256: fc_0 cut to its first 256
    rows and fc_1 to its first 256 columns (the library wants H3 = 256 and H1, H2 multiples of 256)."""
    F = 7 * sum(VOX_C) + img_C + 3
    w = synth.make_mlp_weights(seed, F, 256)
    if H1 == 256:
        w["fc_0.weight"] = np.ascontiguousarray(w["fc_0.weight"][:256])
        w["fc_0.bias"] = np.ascontiguousarray(w["fc_0.bias"][:256])
        w["fc_1.weight"] = np.ascontiguousarray(w["fc_1.weight"][:, :256])
    else:
        assert H1 == 512
    return w
