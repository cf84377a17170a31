"""What the grid-aligned exact tests can see (CPU, numpy): a float32 emulation of gather and scatter -- the restated
coordinate arithmetic, fp32 products and sums, points and taps in shuffled order -- reproduces the float64 reference of
tests/_exact_sample_case.py bit for bit, and each of eight small mistakes moves at least one number."""
import numpy as np
import pytest

import _exact_sample_case as S
from _exact_case import F32, F64

SIZES_USED = (8, 16, 32, 6, 10, 14)
MAPS_USED = ((137, 136.0), (50, 49.0), (50, 136.0))


def test_aligned_coordinates_reach_two_thirds_of_the_targets_with_borders_integers_and_halves():
    for s in SIZES_USED:
        for v in S.AXIS_VARIANTS:
            a = S.aligned_coords(s, v)                     # asserts the conditions itself
            print(f"S={s:3d} {v:>2}: {a['found']} of {a['targets']} half-integer targets, {int((~a['inside']).sum())} points beyond the box")
            assert 3 * a["found"] >= 2 * a["targets"]
            mi = a["m"][a["inside"]]
            assert mi.min() == 0 and mi.max() == 2 * (s - 1) and (mi % 2 == 1).any()
            assert ((mi % 2 == 0) & (mi > 0) & (mi < 2 * (s - 1))).any()
            out = a["p"][~a["inside"]]
            assert (out < -1).any() and (out > 1).any()
    for ms, hi in MAPS_USED:
        a = S.aligned_pixels(ms, hi)
        print(f"ms={ms} clamp_hi={hi}: {a['found']} of {a['targets']} half-pixel targets")
        assert 3 * a["found"] >= 2 * a["targets"]


# ------------------------------------------------------------------------------------------ the emulation
def _axes(c, mutate):
    j = c["j_star"]
    if mutate == "swap_d" and j:
        j = j + 1 if j % 2 else j - 1
    xyz = (S.restate_load_point(c["query"], c["perm"], c["scale"]) + S.stencil_offset(j)).astype(F32).reshape(-1, 3)
    D, H, W = c["align"]
    axes = []
    for a, size in enumerate((W, H, D)):
        if mutate == "border" and a == 0:                # the high clamp one voxel too far: the skipped tap is read
            v = ((xyz[:, a] + F32(1)) * F32(0.5)) * F32(size - 1)
            v = np.minimum(F32(size), np.maximum(v, F32(0))).astype(F32)
        else:
            v = S.restate_axis(xyz[:, a], size)
        i0, w0, w1 = S.restate_weights(v)
        has1 = i0 + 1 < size
        if mutate == "stride0":
            has1 = np.zeros_like(has1)
        if mutate == "swap_w" and a == 1:
            w0, w1 = w1, w0
        axes.append((i0, w0, w1, has1))
    return axes


def _taps(c, mutate, rng):
    """The 8 taps in a shuffled order: flat voxel index within the image [P] and fp32 weight [P]."""
    D, H, W = c["align"]
    (x0, wx0, wx1, hx), (y0, wy0, wy1, hy), (z0, wz0, wz1, hz) = _axes(c, mutate)
    out = []
    for k in rng.permutation(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        w = ((wx1 if dx else wx0) * (wy1 if dy else wy0)).astype(F32) * (wz1 if dz else wz0)
        flat = ((z0 + dz * hz) * H + (y0 + dy * hy)) * W + (x0 + dx * hx)
        out.append((flat % (D * H * W), w.astype(F32)))   # (a tap past the last voxel wraps: only the 'border' mistake makes one)
    return out


def emulate_gather(c, l, rng, mutate=None):
    """-> the reference-order voxel block of X [P, 7 * sum(C)], float32, with level l's aligned sample written."""
    B, N, C = c["B"], c["N"], c["channels"][l]
    D, H, W = c["align"]
    vmap = np.transpose(c["vox_maps"][l], (0, 2, 3, 4, 1)).reshape(B, D * H * W, C)
    b_of = np.repeat(np.arange(B), N)
    acc = np.zeros((B * N, C), F32)
    for flat, w in _taps(c, mutate, rng):
        acc = (acc + w[:, None] * vmap[b_of, flat, :]).astype(F32)
    X = np.zeros((B * N, 7 * sum(c["channels"])), F32)
    X[:, S._level_cols(c["channels"], l, c["j_star"] + (1 if mutate == "col_shift" else 0))] = acc
    return X


def reference_gather(c, l):
    cols = S._level_cols(c["channels"], l, c["j_star"])
    at = np.searchsorted(c["cols"], cols)
    assert np.array_equal(c["cols"][at], cols)
    return cols, np.transpose(c["X_cols"][:, at, :], (0, 2, 1)).reshape(c["B"] * c["N"], len(cols))


def _dx_of(c, l):
    before = sum(c["channels"][k] for k in c["aligned"] if k < l)
    return c["ref"]["dX"][:, before:before + c["channels"][l]].astype(F32)


def round_bits(x, bits):
    m, e = np.frexp(np.asarray(x, F64))
    return np.ldexp(np.round(m * (1 << bits)) / (1 << bits), e)


def emulate_scatter(c, l, rng, mutate=None):
    B, N, C = c["B"], c["N"], c["channels"][l]
    D, H, W = c["align"]
    P = B * N
    dx = _dx_of(c, l)
    rows = rng.permutation(P)
    if mutate == "twice":
        rows = np.append(rows, np.flatnonzero(np.abs(dx).sum(axis=1))[0])
    if mutate == "drop_block":
        rows = rows[rows < (P - 1) // 64 * 64]
    b_of = np.repeat(np.arange(B), N)
    grad = np.zeros((B, D * H * W, C), F32)
    for flat, w in _taps(c, None, rng):
        np.add.at(grad, (b_of[rows], flat[rows]), (w[rows, None] * dx[rows]).astype(F32))      # fp32 adds, one after the other
    if mutate == "flush10":
        scale = S.E.FP16_GRAD_SCALE * S.WIN_PK_SCALE
        grad = (round_bits(grad.astype(F64) * scale, 10) / scale).astype(F32)
    return grad.reshape(B, D, H, W, C)


def moved(got, want):
    return int((np.asarray(got, F64) != np.asarray(want, F64)).sum())


# ------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("j_star", [0, 1, 4])
def test_the_emulated_gather_is_the_reference_and_every_mistake_shows(j_star):
    c = S.vox_case(S.cubic(8), j_star=j_star)
    rng = np.random.default_rng(7 + j_star)
    for l in (0, 2, 5):
        cols, want = reference_gather(c, l)
        for _ in range(2):                               # two orders of the taps
            assert moved(emulate_gather(c, l, rng)[:, cols], want) == 0
        for mistake in ("swap_w", "swap_d", "col_shift", "border", "stride0"):
            if mistake == "swap_d" and j_star == 0:
                continue                                 # the centre has no displacement to exchange
            n = moved(emulate_gather(c, l, rng, mistake)[:, cols], want)
            print(f"gather j*={j_star} level {l} {mistake}: {n} of {want.size} numbers move")
            assert n > 0, (mistake, l)


def test_the_emulated_scatter_is_the_reference_and_every_mistake_shows():
    # 4 096 points of one image, 701 of them one point: eight voxels whose sums need all eleven bits of a packed-half flush
    c = S.vox_case(S.cubic(8), j_star=2, B=1, N=4096, pile=701)
    print(f"density of grad_sdf {c['density']:.3f}, heaviest voxel {c['flush_units']:.0f} units of 1/8 (limit 2048)")
    assert 1024 <= c["flush_units"] < 2048
    rng = np.random.default_rng(11)
    for l in (0, 3, 5):
        want = c["d_vox"][l]
        for _ in range(2):                               # two orders of the points and the taps
            assert moved(emulate_scatter(c, l, rng), want) == 0
        for mistake in ("twice", "drop_block", "flush10"):
            if mistake == "flush10" and c["channels"][l] == 1:
                continue                                 # the scalar level has no packed-half form
            n = moved(emulate_scatter(c, l, rng, mistake), want)
            print(f"scatter level {l} {mistake}: {n} of {want.size} numbers move")
            assert n > 0, (mistake, l)
    for mistake in ("swap_w", "swap_d", "stride0"):      # a wrong tap or weight shows in the adjoint as in the gather
        grad = np.zeros((1, 512, c["channels"][3]), F32)
        dx = _dx_of(c, 3)
        for flat, w in _taps(c, mistake, rng):
            np.add.at(grad, (np.zeros(len(flat), np.int64), flat), (w[:, None] * dx).astype(F32))
        n = moved(grad.reshape(c["d_vox"][3].shape), c["d_vox"][3])
        print(f"scatter level 3 {mistake}: {n} numbers move")
        assert n > 0, mistake


def test_the_image_case_holds_its_conditions_and_reaches_the_clamps():
    for ms, hi in ((50, None), (50, 136.0)):
        c = S.img_case(ms, clamp_hi=hi)
        t = c["m"] / 2.0
        print(f"ms={ms} clamp_hi={c['clamp_hi']}: yield {c['yields']}, heaviest pixel {c['flush_units']:.0f} units")
        assert (t == 0).any() and (t == min(c["clamp_hi"], ms - 1)).any() and (c["m"] % 2 == 1).any()
        assert (t == c["clamp_hi"]).any()
        if c["clamp_hi"] > ms - 1:
            assert (t >= ms).any() and ((t > ms - 1) & (t < ms)).any()          # wholly outside, and half outside
        assert np.abs(c["d_img_map"]).max() > 0 and np.abs(c["X_percep"]).max() > 0
