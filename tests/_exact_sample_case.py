"""Grid-aligned sample points for the voxel and image gathers and their adjoints, with float64 references (numpy only).

The exactness lemma of tests/_exact_case.py with an interpolation weight as the second operand ("Exact-integer
tests", "Grid-aligned samples"): a coordinate whose un-normalised value v = ((c + 1) * 0.5) * (S - 1) is exactly a half
integer m / 2 has the weights w1 = v - floor(v) and w0 = (floor(v) + 1) - v in {0, 1/2, 1} without rounding, so every trilinear
weight is a multiple of 1/8 and every bilinear one a multiple of 1/4.  With small-integer maps and a small-integer dX every
product and every partial sum of a gather, a scatter, an LDS window, an MFMA fragment or a flush is a small multiple of one
power of two: no order can change a bit, and np.array_equal against float64 is the whole comparison.

The stencil displacement 0.0722 is not dyadic, so only ONE of the seven samples of a point can be aligned: a case aligns
sample j_star and gives fc_0 zero weights on the columns of the other six, whose X then reaches no sum and whose dX is 0.

The fp32 restatements below (load_point, the stencil add, axis_setup, project: csrc/point_math.h) CHOOSE the coordinates and
are asserted on every coordinate handed out; the reference weights come from the target m alone, never from them.
"""
import functools

import numpy as np

import _exact_case as E
from _exact_case import F32, F64, _ints

KDISP = F32(0.0722)                         # kDisp, csrc/vox_adjoint_plan.h
WIN_PK_SCALE = 0.0625                       # kWinPkScale: a window level's fp16 image is kept at the gradient scale times this
VOX_CHANNELS = (1, 16, 32, 64, 128, 128)
CALLS = {"model": ((2, 1, 0), 2.0), "plain": ((0, 1, 2), 1.0)}      # network/models.py:91-92, and the identity
AXIS_VARIANTS = ("c", "-d", "+d")
IMG_C = 1024
H1 = 512


# ------------------------------------------------------------------------------------------ fp32 restatements
def restate_load_point(query, perm, scale):
    """load_point: p = query[..., perm] * scale in fp32 (scale is a power of two here: a contracted fma changes nothing)."""
    return (np.asarray(query, F32)[..., list(perm)] * F32(scale)).astype(F32)


def stencil_offset(j):
    """stencil_point<J>: what is ADDED to (x, y, z) -- centre, then (-d, +d) along x, y, z."""
    off = np.zeros(3, F32)
    if j:
        off[(j - 1) // 2] = -KDISP if j % 2 else KDISP
    return off


def restate_axis(c, size):
    """axis_setup: the clamped un-normalised coordinate v, fp32 step by step."""
    c = np.asarray(c, F32)
    hi = F32(size - 1)
    v = ((c + F32(1.0)) * F32(0.5)) * hi
    return np.where(v != v, hi, np.minimum(hi, np.maximum(v, F32(0.0)))).astype(F32)


def restate_weights(v):
    """axis_setup's i0, w0, w1 of a clamped v (used by the emulation of tests/test_exact_sample_cpu.py only)."""
    f = np.floor(v).astype(F32)
    return f.astype(np.int64), ((f + F32(1.0)) - v).astype(F32), (v - f).astype(F32)


def restate_project(T, px, py, pz, ms, clamp_hi):
    """project: (ix, iy) of one camera T[12], fp32 with the fma chain of the kernel (numpy has no fma: the chain is exact in
    float64 for the cameras used here -- products of a power of two and sums of two terms -- and rounded once)."""
    T = np.asarray(T, F32).reshape(12).astype(F64)
    px, py, pz = (np.asarray(t, F32).astype(F64) for t in (px, py, pz))
    assert T[3] == 0 and T[6] == 0 and T[1] == 0 and T[7] == 0 and not T[[2, 5, 8]].any(), "restated for diagonal cameras only"
    X = (px * T[0]).astype(F32) + F32(T[9])
    Y = (py * T[4]).astype(F32) + F32(T[10])
    Z = np.zeros_like(X) + F32(T[11])
    den = (Z + F32(1e-8)).astype(F32)
    half = F32(F32(ms - 1) * F32(0.5))
    out = []
    for r in (X, Y):
        u = np.minimum(np.maximum((r / den).astype(F32), F32(0.0)), F32(clamp_hi)).astype(F32)
        g = ((u - half).astype(F32) / half).astype(F32)
        out.append(((g + F32(1.0)).astype(F32) * half).astype(F32))
    return out[0], out[1]


def _neighbours(x, n=4):
    """The fp32 value x and its n neighbours on either side, nearest first."""
    x = F32(x)
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.array(out, F32)


# ------------------------------------------------------------------------------------------ aligned coordinates
@functools.lru_cache(maxsize=None)
def aligned_coords(size, variant):
    """Coordinates p (BEFORE the stencil add) of one axis of a level of `size` voxels whose sample -- the centre ('c'), the
    one displaced by -kDisp ('-d') or by +kDisp ('+d') -- lands exactly on a half integer.
    -> dict(p [K] float32, m [K] int (v = m / 2), inside [K] bool, targets: how many half-integer targets there are,
    found: how many of them the search reached).  Asserts the restated v of every coordinate handed out."""
    assert variant in AXIS_VARIANTS and size >= 2
    off = F32(0.0) if variant == "c" else (-KDISP if variant == "-d" else KDISP)
    ps, ms = [], []
    n_targets = 2 * (size - 1) + 1
    for m in range(n_targets):
        t = F32(m) * F32(0.5)
        got = None
        for c in _neighbours(F32(2.0 * float(t) / (size - 1) - 1.0)):
            for p in (_neighbours(F32(c - off)) if variant != "c" else [c]):
                if restate_axis(F32(p + off), size) == t and F32(p * F32(0.5)) * F32(2.0) == p:
                    got = p
                    break
            if got is not None:
                break
        if got is not None:
            ps.append(got)
            ms.append(m)
    found = len(ps)
    inside = [True] * found
    for p, m in ((-1.5, 0), (-1.25, 0), (1.25, n_targets - 1), (1.5, n_targets - 1)):      # beyond the box: clamped, aligned for free
        ps.append(F32(p)); ms.append(m); inside.append(False)
    p, m, inside = np.array(ps, F32), np.array(ms, np.int64), np.array(inside)
    assert np.array_equal(restate_axis((p + off).astype(F32), size).astype(F64), m / 2.0), (size, variant)
    mi = m[inside]
    assert 3 * found >= 2 * n_targets, f"S={size} {variant}: {found} of {n_targets} targets"
    assert 0 in mi and n_targets - 1 in mi, f"S={size} {variant}: a border is missing"
    assert any(0 < k < n_targets - 1 and k % 2 == 0 for k in mi) or size == 2, f"S={size} {variant}: no interior integer"
    assert any(k % 2 == 1 for k in mi), f"S={size} {variant}: no interior half"
    return dict(p=p, m=m, inside=inside, targets=n_targets, found=found)


def axis_variants(j_star):
    """The variant of the x, y, z axis when stencil sample j_star is the aligned one."""
    v = ["c", "c", "c"]
    if j_star:
        v[(j_star - 1) // 2] = "-d" if j_star % 2 else "+d"
    return v


def reference_axis(m, size):
    """From the target alone: i0, the weight of tap i0, the weight of tap i0 + 1 and whether that tap exists."""
    i0 = m // 2
    f = (m % 2) / 2.0
    return i0, 1.0 - f, f, (i0 + 1) < size


def trilinear_taps(m, dims):
    """m [P, 3] (x, y, z targets), dims (D, H, W) -> list of 8 (z, y, x index arrays, weight [P]); a tap beyond the border
    is skipped (weight 0, index kept inside)."""
    D, H, W = dims
    ax = [reference_axis(m[:, a], s) for a, s in ((0, W), (1, H), (2, D))]
    taps = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = np.ones(len(m), F64)
                idx = []
                for (i0, w0, w1, has1), d in zip(ax, (dx, dy, dz)):
                    w = w * (np.where(has1, w1, 0.0) if d else w0)
                    idx.append(np.where(has1, i0 + d, i0))
                taps.append((idx[2], idx[1], idx[0], w))
    return taps


def scatter_add(shape, indices, weights, dx):
    """out[cell] = sum over taps and points of w dx[point, :], and the same sum of |w dx| -- np.add.at's result, formed by
    sorting the contributions by cell and summing each run (float64: exact for these operands, in any order).
    shape: the cells' grid; indices: per tap a tuple of index arrays [P]; weights: per tap [P]; dx [P, C]."""
    flat = np.concatenate([np.ravel_multi_index(i, shape) for i in indices])
    contrib = np.concatenate([w[:, None] * dx for w in weights])
    order = np.argsort(flat, kind="stable")
    flat, contrib = flat[order], contrib[order]
    starts = np.flatnonzero(np.r_[True, flat[1:] != flat[:-1]])
    n_cells = int(np.prod(shape))
    out, mass = np.zeros((n_cells, dx.shape[1]), F64), np.zeros((n_cells, dx.shape[1]), F64)
    out[flat[starts]] = np.add.reduceat(contrib, starts, axis=0)
    mass[flat[starts]] = np.add.reduceat(np.abs(contrib), starts, axis=0)
    return out.reshape(tuple(shape) + (dx.shape[1],)), mass.reshape(tuple(shape) + (dx.shape[1],))


# ------------------------------------------------------------------------------------------ the voxel case
def _level_cols(channels, l, j):
    """Reference feature indices (c_base + c) * 7 + j of level l's sample j."""
    base = sum(channels[:l])
    return (base + np.arange(channels[l])) * 7 + j


def _half_flush_units(sum_abs):
    """Largest per-voxel sum |w dX| in units of 1/8: the packed-half flushes hold 2^11 of them exactly at any scale."""
    return float(sum_abs.max()) * 8.0


@functools.lru_cache(maxsize=2)
def vox_case(sizes, channels=VOX_CHANNELS, j_star=0, variant="model", B=2, N=300, align=None, pile=0):
    """sizes: six (D, H, W); align: the (D, H, W) whose levels are aligned in this run (default: level 1's).  Extends
    mlp_case: integer voxel maps in [-3, 3] (level 0 in {0, 1}), percep_feat in [-3, 3], fc_0.weight non-zero only on the
    columns c * 7 + j_star of the aligned levels and on the perceptual block, grad_sdf in {-1, 0, 1} thinned until the
    packed-half bound holds.  pile: the first `pile` points of image 0 are one point -- on a half integer along every axis,
    with one column of percep_feat and one grad_sdf -- so that their dX adds up with one sign in eight voxels (a heavy
    voxel: many atomics on one address, a flush of eleven bits).  (fc_0 is zero on xyz too: the aligned coordinates are 24-bit numbers no 16-bit format holds.)
    -> dict with query, vox_maps, percep_feat, weights, grad_sdf, aligned (levels), cols (reference feature indices of the
    aligned and perceptual columns), X_cols [B, len(cols), N], sdf [B, N], d_vox {l: [B, D, H, W, C]}, precisions, units.
    Cached: treat the arrays as read-only."""
    sizes, channels = tuple(tuple(s) for s in sizes), tuple(channels)
    perm, scale = CALLS[variant]
    align = tuple(align) if align is not None else sizes[1]
    aligned = [l for l in range(6) if sizes[l] == align]
    assert aligned, "no level has the aligned size"
    D, H, W = align
    seed = 9000 + 37 * j_star + 1000 * (D + 3 * H + 7 * W) + N
    P = B * N
    # ---- coordinates: every point draws one aligned coordinate per axis
    off = stencil_offset(j_star)
    p = np.zeros((B, N, 3), F32)
    m = np.zeros((B, N, 3), np.int64)
    yields = {}
    for a, (s, v) in enumerate(zip((W, H, D), axis_variants(j_star))):
        ac = aligned_coords(s, v)
        pick = _ints(seed + a, (B, N), 0, len(ac["p"]) - 1)
        if pile:
            odd = np.flatnonzero(ac["m"] % 2 == 1)
            pick[0, :pile] = odd[len(odd) // 2]
        p[:, :, a], m[:, :, a] = ac["p"][pick], ac["m"][pick]
        yields[(s, v)] = (ac["found"], ac["targets"])
    query = np.zeros((B, N, 3), F32)
    for a in range(3):
        query[:, :, perm[a]] = p[:, :, a] / F32(scale)
    sample = (restate_load_point(query, perm, scale) + off).astype(F32)
    for a, s in enumerate((W, H, D)):
        assert np.array_equal(restate_axis(sample[:, :, a], s).astype(F64), m[:, :, a] / 2.0), "a coordinate is not aligned"
    # ---- maps
    vox = []
    for l, (c, s) in enumerate(zip(channels, sizes)):
        lo, hi = (0, 1) if l == 0 else (-3, 3)
        vox.append(_ints(seed + 10 + l, (B, c) + s, lo, hi).astype(F32))
    pf = _ints(seed + 20, (B, IMG_C, N), -3, 3).astype(F32)
    if pile:
        assert 0 < pile <= N
        pf[0, :, :pile] = pf[0, :, :1]
    # ---- reference gather of the aligned columns
    mm = m.reshape(P, 3)
    b_of = np.repeat(np.arange(B), N)
    taps = trilinear_taps(mm, align)
    cols, Xa = [], []
    for l in aligned:
        x = np.zeros((P, channels[l]), F64)
        for z, y, xx, w in taps:
            x += w[:, None] * vox[l][b_of, :, z, y, xx].astype(F64)
        cols.append(_level_cols(channels, l, j_star))
        Xa.append(x)
    n_vox_cols = 7 * sum(channels)
    cols.append(n_vox_cols + np.arange(IMG_C))
    Xa.append(np.transpose(pf, (0, 2, 1)).reshape(P, IMG_C).astype(F64))
    cols, Xa = np.concatenate(cols), np.concatenate(Xa, axis=1)
    n_act = len(cols)
    Fdim = n_vox_cols + IMG_C + 3
    # ---- weights: fc_0 is a sum of six signed shifted permutations over the active columns, zero elsewhere
    wts = E._mlp_weights(H1)
    w0a = E.shifted_perms(H1, n_act, 6, 0)
    w0 = np.zeros((H1, Fdim), F32)
    w0[:, cols] = w0a
    wts["fc_0.weight"] = w0[:, :, None]
    ref_w = dict(wts, **{"fc_0.weight": w0a.astype(F32)[:, :, None]})
    # ---- grad_sdf, thinned until every packed-half flush is exact
    dens = 1.0
    keep_rank = _ints(seed + 30, (P,), 0, (1 << 20) - 1)
    sign = _ints(seed + 31, (P,), 0, 1) * 2 - 1
    keep_rank[:pile], sign[:pile] = 0, sign[0]
    while True:
        g = np.where(keep_rank < dens * (1 << 20), sign, 0).astype(F64)
        r = E.mlp_reference(Xa, ref_w, g)
        d_vox, worst = {}, 0.0
        for i, l in enumerate(aligned):
            dx = r["dX"][:, sum(channels[k] for k in aligned[:i]):][:, :channels[l]]
            grad, mass = scatter_add((B,) + align, [(b_of, z, y, xx) for z, y, xx, _ in taps], [t[3] for t in taps], dx)
            d_vox[l] = grad
            worst = max(worst, _half_flush_units(mass))
        if worst < 2048.0:
            break
        dens *= 0.85
        assert dens > 0.01, "grad_sdf thinned away"
    assert np.count_nonzero(g) >= 32
    # ---- the lemma's conditions
    c = dict(sizes=sizes, channels=channels, j_star=j_star, variant=variant, perm=perm, scale=scale, B=B, N=N, align=align,
             aligned=aligned, query=query, vox_maps=vox, percep_feat=pf, weights=wts, grad_sdf=g.reshape(B, N).astype(F32),
             cols=cols, X_cols=np.transpose(Xa.reshape(B, N, n_act), (0, 2, 1)), sdf=r["sdf"].reshape(B, N), d_vox=d_vox,
             precisions=("fp16", "bf16x3"), F=Fdim, density=dens, yields=yields, m=m, ref=r, pile=pile)
    bits = {"fp16": 11, "bf16x3": 16}
    values = {k: np.unique(a) for k, a in (("X", Xa), ("H1", r["H1"]), ("H2", r["H2"]), ("H3", r["H3"]))}      # (few distinct numbers)
    grads = {k: np.unique(r[k]) for k in ("dZ3", "dZ2", "dZ1", "dX")}
    for prec in c["precisions"]:
        for k, a in values.items():
            assert E.sig_bits(a) <= bits[prec] and E.exact_in(a, prec), (prec, k, E.sig_bits(a))
        for k, a in grads.items():
            assert E.sig_bits(a) <= 8, (k, E.sig_bits(a))
            assert E.exact_in(a * (E.FP16_GRAD_SCALE if prec == "fp16" else 1.0), prec), (prec, k)
    assert np.abs(r["dX"]).max() * E.FP16_GRAD_SCALE < 65504.0
    acts = [Xa, r["H1"], r["H2"], r["H3"]]
    Ws = [np.asarray(ref_w[f"{n}.weight"], F64)[:, :, 0] for n in ("fc_0", "fc_1", "fc_2", "fc_out")]
    bs = [np.asarray(ref_w[f"{n}.bias"], F64) for n in ("fc_0", "fc_1", "fc_2", "fc_out")]
    units = max(E.partial_sum_units(acts[i], Ws[i], bs[i]) for i in range(4))
    for i in (2, 1, 0):
        units = max(units, E.partial_sum_units(r[f"dZ{i + 1}"] * E.FP16_GRAD_SCALE, Ws[i].T))
    assert units < E.LIMIT, units
    # fp32 atomics and LDS windows: per voxel sum |w dX| in units of 1/8 (times the fp16 scale) far below 2^24; the packed
    # halfs, at the gradient scale (times kWinPkScale for window levels): below 2^11 units, and inside fp16's range
    assert worst * E.FP16_GRAD_SCALE < E.LIMIT and worst < 2048.0
    assert worst / 8.0 * E.FP16_GRAD_SCALE < 65504.0 and E.FP16_GRAD_SCALE * WIN_PK_SCALE / 8.0 >= 2.0 ** -14
    c["units"], c["flush_units"] = units, worst
    return c


def cubic(s, channels=VOX_CHANNELS):
    return tuple((s, s, s) for _ in channels)


# ------------------------------------------------------------------------------------------ the 2-D case
CAMERA_A = 64.0


def camera(ms, B):
    h = (ms - 1) / 2.0
    T = np.array([[CAMERA_A, 0, 0], [0, CAMERA_A, 0], [0, 0, 0], [h, h, 1]], F32)
    return np.repeat(T[None], B, axis=0)


@functools.lru_cache(maxsize=None)
def aligned_pixels(ms, clamp_hi):
    """Point coordinates px (one axis; both axes of the camera above are alike) whose projected pixel coordinate is exactly
    m / 2.  -> dict(p, m, targets, found); m / 2 >= ms lies wholly outside the map (zeros padding: no weight is read)."""
    T = camera(ms, 1)[0]
    top = int(clamp_hi)
    assert top == clamp_hi
    ps, mk = [], []
    n_targets = 2 * top + 1
    for m in range(n_targets):
        for px in _neighbours(F32((m - (ms - 1)) / (2.0 * CAMERA_A))):
            ix, _ = restate_project(T, px, px, F32(0), ms, clamp_hi)
            if ix == F32(m / 2.0) or (m / 2.0 >= ms and ix >= F32(ms)):
                ps.append(px); mk.append(m)
                break
    found = len(ps)
    for px, m in ((-2.0, 0), (-1.5, 0), (2.0, 2 * top), (1.75, 2 * top)):       # beyond both clamps
        ix, _ = restate_project(T, F32(px), F32(px), F32(0), ms, clamp_hi)
        if ix == F32(m / 2.0) or (m / 2.0 >= ms and ix >= F32(ms)):
            ps.append(F32(px)); mk.append(m)
    p, m = np.array(ps, F32), np.array(mk, np.int64)
    ix, iy = restate_project(T, p, p, np.zeros_like(p), ms, clamp_hi)
    ok = np.where(m / 2.0 >= ms, ix >= F32(ms), ix.astype(F64) == m / 2.0)
    assert ok.all() and np.array_equal(ix, iy)
    assert 3 * found >= 2 * n_targets, f"ms={ms}: {found} of {n_targets} targets"
    assert 0 in m[:found] and 2 * min(top, ms - 1) in m[:found] and (m[:found] % 2 == 1).any()
    assert (p[found:] < 0).any() and (p[found:] > 0).any(), "a clamp cannot be piled on"
    return dict(p=p, m=m, targets=n_targets, found=found)


def bilinear_taps(m, ms):
    """m [P, 2] (x, y targets) -> list of 4 (y, x, weight); a tap outside the map has weight 0 (zeros padding)."""
    ax = []
    for a in (0, 1):
        i0, f = m[:, a] // 2, (m[:, a] % 2) / 2.0
        ax.append((i0, np.where(i0 <= ms - 1, 1.0 - f, 0.0), np.where(i0 + 1 <= ms - 1, f, 0.0)))
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            (x0, wx0, wx1), (y0, wy0, wy1) = ax
            taps.append((np.minimum(y0 + dy, ms - 1), np.minimum(x0 + dx, ms - 1), (wx1 if dx else wx0) * (wy1 if dy else wy0)))
    return taps


@functools.lru_cache(maxsize=2)
def img_case(ms, B=2, N=300, clamp_hi=None, variant="plain", pile=0):
    """An integer map [B, ms, ms, 1024] in [-3, 3] (to be handed over as a PreparedImage), the camera above, zero voxel maps.
    pile: that many points of image 0 on the pixel (0, 0) -- both coordinates below the low clamp.
    -> dict with query, trans_mat, img_map, vox_maps, weights, grad_sdf, X_percep [B, 1024, N], sdf, d_img_map
    [B, ms, ms, 1024], d_percep (the gradient of the pooled features, [B, 1024, N]), precisions."""
    clamp_hi = float(ms - 1 if clamp_hi is None else clamp_hi)
    perm, scale = CALLS[variant]
    P = B * N
    seed = 7000 + ms + N
    ap = aligned_pixels(ms, clamp_hi)
    pick = _ints(seed, (B, N, 2), 0, len(ap["p"]) - 1)
    reach = np.flatnonzero(ap["m"] / 2.0 < ms)
    if len(reach) < len(ap["p"]):               # a clamp beyond the map: three coordinates of four still reach it
        pick = np.where(_ints(seed + 5, (B, N, 2), 0, 3) > 0, reach[pick % len(reach)], pick)
    lows, highs = np.flatnonzero(ap["p"] < -1.2), np.flatnonzero(ap["p"] > 1.2)
    pick[:, -4:, :] = highs[0]                    # piled on the high clamp, on the low one, and on one of each
    pick[:, -8:-4, :] = lows[0]
    pick[:, -12:-8, 0], pick[:, -12:-8, 1] = lows[-1], highs[-1]
    if pile:
        assert pile <= N and len(lows)
        pick[0, :pile, :] = lows[0]
    p = np.zeros((B, N, 3), F32)
    p[:, :, :2] = ap["p"][pick]
    p[:, :, 2] = (_ints(seed + 1, (B, N), -4, 4) * 0.25).astype(F32)        # z reaches neither X nor Y nor the denominator
    m = ap["m"][pick]
    query = np.zeros((B, N, 3), F32)
    for a in range(3):
        query[:, :, perm[a]] = p[:, :, a] / F32(scale)
    T = camera(ms, B)
    pp = restate_load_point(query, perm, scale)
    ix, iy = restate_project(T[0], pp[:, :, 0], pp[:, :, 1], pp[:, :, 2], ms, clamp_hi)
    for a, got in enumerate((ix, iy)):
        t = m[:, :, a] / 2.0
        assert np.where(t >= ms, got >= F32(ms), got.astype(F64) == t).all(), "a projection is not aligned"
    img = _ints(seed + 2, (B, ms, ms, IMG_C), -3, 3).astype(F32)
    tiny = E.cases.build_case("tiny")
    vox = [np.zeros((B,) + v.shape[1:], F32) for v in tiny["vox_maps"]]
    mm = m.reshape(P, 2)
    b_of = np.repeat(np.arange(B), N)
    taps = bilinear_taps(mm, ms)
    Xp = np.zeros((P, IMG_C), F64)
    for y, x, w in taps:
        Xp += w[:, None] * img[b_of, y, x, :].astype(F64)
    wts = E._mlp_weights(H1)
    w0 = np.array(wts["fc_0.weight"][:, :, 0])
    w0a = E.shifted_perms(H1, IMG_C, 6, 0)
    w0[:, E.VOX_COLS:E.VOX_COLS + IMG_C] = w0a
    w0[:, E.VOX_COLS + IMG_C:] = 0                  # xyz: see vox_case
    wts["fc_0.weight"] = w0[:, :, None]
    ref_w = dict(wts, **{"fc_0.weight": w0a.astype(F32)[:, :, None]})
    g = (_ints(seed + 3, (P,), -1, 1)).astype(F64)
    r = E.mlp_reference(Xp, ref_w, g)
    d_map, mass = scatter_add((B, ms, ms), [(b_of, y, x) for y, x, _ in taps], [t[2] for t in taps], r["dX"])
    c = dict(ms=ms, B=B, N=N, clamp_hi=clamp_hi, variant=variant, perm=perm, scale=scale, query=query, trans_mat=T, img_map=img,
             vox_maps=vox, weights=wts, grad_sdf=g.reshape(B, N).astype(F32), m=m,
             X_percep=np.transpose(Xp.reshape(B, N, IMG_C), (0, 2, 1)), sdf=r["sdf"].reshape(B, N), d_img_map=d_map,
             d_percep=np.transpose(r["dX"].reshape(B, N, IMG_C), (0, 2, 1)), precisions=("fp16", "bf16x3"), ref=r,
             yields=(ap["found"], ap["targets"]), pile=pile)
    values = {k: np.unique(a) for k, a in (("X", Xp), ("H1", r["H1"]), ("H2", r["H2"]), ("H3", r["H3"]))}
    grads = {k: np.unique(r[k]) for k in ("dZ3", "dZ2", "dZ1", "dX")}
    for prec, nb in (("fp16", 11), ("bf16x3", 16)):
        for k, a in values.items():
            assert E.sig_bits(a) <= nb and E.exact_in(a, prec), (prec, k, E.sig_bits(a))
        for k, a in grads.items():
            assert E.sig_bits(a) <= 8 and E.exact_in(a * (E.FP16_GRAD_SCALE if prec == "fp16" else 1.0), prec), (prec, k)
    # the projected map of prep_percep_proj: map . fc_0's perceptual block, per pixel -- integers of at most 18
    assert np.abs(w0a).sum(axis=1).max() * 3 < 2048
    # per pixel sum |w dX| in units of 1/4 (times the fp16 scale): fp32 partial rows, atomics and heavy partials are exact
    c["flush_units"] = float(mass.max()) * 4.0 * E.FP16_GRAD_SCALE
    assert c["flush_units"] < E.LIMIT
    return c
