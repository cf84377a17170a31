"""Coarse-to-fine SDF grid for meshing: the network is queried on a coarse lattice of the R^3 grid and then only at the
fine points near the surface (the MISE idea of Occupancy Networks, one level).

Marching cubes reads the field's sign everywhere and its values only in the cells the surface cuts.  With stride s:

  1. the lattice c_m = min(m * s, R - 1), m = 0 .. K - 1, K = ceil((R - 1) / s) + 1, is queried (K^3 points at
     exactly the dense grid's coordinates);
  2. a brick (the fine points between neighbouring lattice indices) is active iff a corner is not finite, its corners
     straddle `level`, or a corner lies within `band` of it; the active set is dilated by one brick;
  3. the fine points that are no lattice points and lie in a dilated brick (on faces: in any brick holding them) are
     listed in raster order and queried;
  4. the [R,R,R] volume takes the lattice values, the refined values and, everywhere else, the trilinear
     interpolation of the 8 corners of the point's brick.

Guarantee: if the dense volume has no sign change (w.r.t. `level`) within the closed extent of any inactive brick,
marching cubes of the filled volume is marching cubes of the dense one, vertices and faces bit for bit -- every cut
cell then has 8 exact corners, every other cell has all corners on one side (an inactive brick's corners are finite,
on one side and at least `band` from `level`, so is its interpolation).  A feature thinner than the band that no
lattice point sees can be missed: then the result is an approximation.  The default band is a brick's diagonal, twice
the strict bound for a 1-Lipschitz SDF.

The steps run on the device through liblist_hip.so (include/list_refine.h); classify_cpu, refined_points_cpu and
fill_cpu restate them in numpy, bit for bit: the test oracle and the CPU path of predict_grid_refined.
"""
import ctypes as C

import numpy as np

from . import hip, parallel

MAX_R = 1290                           # R^3 <= INT32_MAX: bricks and fine points are int32-indexed
STRIDES = (2, 4, 8)

REFINE_EXPORTS = {
    "list_refine_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "list_refine_mask_offset": (C.c_size_t, [C.c_int32, C.c_int32]),
    "list_refine_count": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p]),
    "list_refine_emit": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_void_p]),
    "list_refine_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_void_p]),
    "list_refine_last_error": (C.c_char_p, []),
}

_section = hip.Section(REFINE_EXPORTS, "list_refine_last_error")    # include/list_refine.h on hip.load()'s handle
load, _check = _section.load, _section.check


# ---- geometry -------------------------------------------------------------------------------------------------------
def check_args(R, s):
    if s not in STRIDES:
        raise hip.ListError("refine", hip.ERR_SHAPE, f"stride s = {s}: must be 2, 4 or 8")
    if R < 2:
        raise hip.ListError("refine", hip.ERR_SHAPE, f"R = {R}: the grid needs at least 2 points per axis")
    if R > MAX_R:
        raise hip.ListError("refine", hip.ERR_SHAPE, f"R = {R}: R^3 exceeds INT32_MAX (at most R = {MAX_R})")


def dims(R, s):
    """(K, NB): lattice points and bricks per axis."""
    check_args(R, s)
    K = -(-(R - 1) // s) + 1
    return K, K - 1


def lattice_indices(R, s):
    """Fine index of every lattice index, per axis: int64 [K]."""
    K, _ = dims(R, s)
    return np.minimum(np.arange(K, dtype=np.int64) * s, R - 1)


def default_band(R, s, lo=-0.5, hi=0.5):
    """The diagonal of a full brick in world units."""
    check_args(R, s)
    return float(np.sqrt(3.0) * min(s, R - 1) * (hi - lo) / (R - 1))


def lattice_points(R, s, device, begin=0, end=None, lo=-0.5, hi=0.5):
    """float32 coordinates [end - begin, 3] of the lattice points [begin, end) in raster order: the dense grid's
    coordinates at those indices, bit for bit (utils.grid_axis_coord)."""
    import torch
    from . import utils
    K, _ = dims(R, s)
    end = K ** 3 if end is None else end
    m = torch.arange(begin, end, device=device, dtype=torch.int64)
    axes = (m // (K * K), (m // K) % K, m % K)
    return torch.stack([utils.grid_axis_coord(torch.clamp(a * s, max=R - 1), lo, hi, R) for a in axes], dim=1)


# ---- host restatement -----------------------------------------------------------------------------------------------
def classify_cpu(lattice, level=0.0, band=None, R=None, s=None):
    """lattice float32 [K,K,K] -> (active, dilated) bool [NB,NB,NB].  band=None: default_band(R, s)."""
    v = np.ascontiguousarray(lattice, dtype=np.float32)
    if band is None:
        band = default_band(R, s)
    lv, bd = np.float32(level), np.float32(band)
    n = v.shape[0] - 1
    bad = np.zeros((n, n, n), dtype=bool)
    any_in = np.zeros_like(bad)
    any_out = np.zeros_like(bad)
    near = np.zeros_like(bad)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            w = v[dx:dx + n, dy:dy + n, dz:dz + n]
            inside = w > lv
            bad |= ~np.isfinite(w)
            any_in |= inside
            any_out |= ~inside
            near |= np.abs(w - lv) < bd
    active = bad | (any_in & any_out) | near
    pad = np.pad(active, 1)
    dilated = np.zeros_like(active)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                dilated |= pad[dx:dx + n, dy:dy + n, dz:dz + n]
    return active, dilated


def _axis_tables(R, s):
    """Per fine index: lattice index or -1, the range [lo, hi] of bricks holding it, the interpolating brick and t."""
    K, NB = dims(R, s)
    i = np.arange(R, dtype=np.int64)
    lat = np.where(i == R - 1, K - 1, np.where(i % s == 0, i // s, -1))
    b_lo = np.where(lat < 0, i // s, np.maximum(lat - 1, 0))
    b_hi = np.where(lat < 0, i // s, np.minimum(lat, NB - 1))
    b = np.minimum(i // s, NB - 1)
    c0, c1 = np.minimum(b * s, R - 1), np.minimum((b + 1) * s, R - 1)
    t = (i - c0).astype(np.float32) / (c1 - c0).astype(np.float32)
    return lat, b_lo, b_hi, b, t


def refined_mask_cpu(dilated, R, s):
    """bool [R,R,R]: the refined fine points."""
    lat, b_lo, b_hi, _, _ = _axis_tables(R, s)
    m = np.zeros((R, R, R), dtype=bool)
    for bx in (b_lo, b_hi):
        for by in (b_lo, b_hi):
            for bz in (b_lo, b_hi):
                m |= dilated[bx[:, None, None], by[None, :, None], bz[None, None, :]]
    on = lat >= 0
    m &= ~(on[:, None, None] & on[None, :, None] & on[None, None, :])
    return m


def refined_points_cpu(dilated, R, s, lo=-0.5, hi=0.5):
    """(coords float32 [n,3], flat fine indices int32 [n]) of the refined points, in raster order."""
    idx = np.flatnonzero(refined_mask_cpu(dilated, R, s).ravel())
    step = (hi - lo) / (R - 1)
    ijk = np.unravel_index(idx, (R, R, R))
    coords = np.empty((idx.size, 3), dtype=np.float32)
    for a in range(3):
        t = ijk[a]
        coords[:, a] = np.where(t == R - 1, float(hi), lo + t.astype(np.float64) * step).astype(np.float32)
    return coords, idx.astype(np.int32)


def fill_cpu(lattice, values, indices, R, s):
    """The filled float32 [R,R,R] volume: lattice values, values[n] at the flat fine indices[n], trilinear elsewhere."""
    v = np.ascontiguousarray(lattice, dtype=np.float32)
    lat, _, _, b, t = _axis_tables(R, s)

    def lerp(a, c, w):
        return a + w * (c - a)
    bx, by, bz = b[:, None, None], b[None, :, None], b[None, None, :]
    tz = t[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        c = [[lerp(v[bx + x, by + y, bz], v[bx + x, by + y, bz + 1], tz) for y in range(2)] for x in range(2)]
        ty, tx = t[None, :, None], t[:, None, None]
        out = lerp(lerp(c[0][0], c[0][1], ty), lerp(c[1][0], c[1][1], ty), tx).astype(np.float32)
    out = np.array(np.broadcast_to(out, (R, R, R)), dtype=np.float32)         # (a writable copy)
    out.reshape(-1)[np.asarray(indices, dtype=np.int64)] = np.asarray(values, dtype=np.float32).reshape(-1)
    li = np.flatnonzero(lat >= 0)
    out[np.ix_(li, li, li)] = v[np.ix_(lat[li], lat[li], lat[li])]
    return out


# ---- device ---------------------------------------------------------------------------------------------------------
class Plan:
    """What list_refine_count left for emit and fill: the workspace, the grid and the number of refined points."""

    def __init__(self, ws, R, s, n):
        self.ws, self.R, self.s, self.n = ws, R, s, n

    def masks(self):
        """(active, dilated) uint8 [NB,NB,NB] device views of the workspace."""
        _, NB = dims(self.R, self.s)
        off = load().list_refine_mask_offset(self.R, self.s)
        nb3 = NB ** 3
        return self.ws[:nb3].view(NB, NB, NB), self.ws[off:off + nb3].view(NB, NB, NB)


def _cuda_f32(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError(f"{what} must be a float32 CUDA/HIP tensor (got {type(t).__name__} "
                           f"{getattr(t, 'dtype', None)} {getattr(t, 'device', None)})")


def count(lattice, R, s, level=0.0, band=None):
    """Classify, dilate and count on the lattice's device and current stream -> Plan.  lattice: float32 [K,K,K]
    (or [K^3]).  The one host synchronisation reads the count back."""
    import torch
    _cuda_f32(lattice, "lattice")
    K, _ = dims(R, s)
    if lattice.numel() != K ** 3:
        raise hip.ListError("list_refine_count", hip.ERR_SHAPE, f"lattice of {lattice.numel()} values, need {K}^3")
    band = default_band(R, s) if band is None else float(band)
    lib = load()
    dev = lattice.device
    with torch.cuda.device(dev):
        need = _section.sized(lib.list_refine_workspace_bytes(R, s), "list_refine_workspace_bytes")
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        total = torch.empty((1,), dtype=torch.int64, device=dev)
        lat = lattice.contiguous()
        _check(lib.list_refine_count(lat.data_ptr(), R, s, float(level), band, ws.data_ptr(), need, total.data_ptr(),
                                     hip._stream()), "list_refine_count")
        n = int(total.item())
    return Plan(ws, R, s, n)


def emit(plan, lo=-0.5, hi=0.5):
    """-> (coords float32 [n,3], flat fine indices int32 [n]) of the refined points, in raster order."""
    import torch
    dev = plan.ws.device
    with torch.cuda.device(dev):
        coords = torch.empty((plan.n, 3), dtype=torch.float32, device=dev)
        idx = torch.empty((plan.n,), dtype=torch.int32, device=dev)
        _check(load().list_refine_emit(plan.R, plan.s, float(lo), float(hi), plan.ws.data_ptr(), plan.ws.numel(),
                                       coords.data_ptr() if plan.n else None, idx.data_ptr() if plan.n else None,
                                       plan.n, hip._stream()), "list_refine_emit")
    return coords, idx


def fill(plan, lattice, values):
    """-> the filled float32 [R,R,R] volume on the plan's device.  values: float32 [n], the field at emit's points."""
    import torch
    _cuda_f32(lattice, "lattice")
    _cuda_f32(values, "values")
    K, _ = dims(plan.R, plan.s)
    if lattice.numel() != K ** 3 or values.numel() != plan.n:
        raise hip.ListError("list_refine_fill", hip.ERR_SHAPE,
                            f"lattice of {lattice.numel()} values (need {K ** 3}), values of {values.numel()} "
                            f"(need {plan.n})")
    R = plan.R
    dev = plan.ws.device
    with torch.cuda.device(dev):
        lat, val = lattice.contiguous(), values.contiguous()
        vol = torch.empty((R, R, R), dtype=torch.float32, device=dev)
        _check(load().list_refine_fill(lat.data_ptr(), val.data_ptr() if plan.n else None, plan.n, R, plan.s,
                                       plan.ws.data_ptr(), plan.ws.numel(), vol.data_ptr(), hip._stream()),
               "list_refine_fill")
    return vol


# ---- driver ---------------------------------------------------------------------------------------------------------
def _query_all(query_fn, pts_of, total, step, device, shard):
    """query_fn over the points [0, total) in chunks of `step` (this rank's share when sharded, then gathered)."""
    import torch
    rank, world = parallel.world_info() if shard else (0, 1)
    begin, end = parallel.shard_range(total, rank, world)
    out = torch.empty((end - begin,), dtype=torch.float32, device=device)
    for b in range(begin, end, step):
        e = min(b + step, end)
        out[b - begin:e - begin] = torch.as_tensor(query_fn(pts_of(b, e).unsqueeze(0))).reshape(-1)
    if shard:
        out = parallel.gather_ragged_points(out, total)
    return out


def predict_grid_refined(query_fn, R, s, band=None, level=0.0, device=None, step=1 << 20, shard=False, lo=-0.5,
                         hi=0.5):
    """The filled [R,R,R] float32 volume of the coarse-to-fine grid, and a dict of counts (lattice, refined, queried
    points and the queried share of R^3).

    query_fn maps a [1,P,3] float32 coordinate chunk to the P field values (already divided by sdf_scale).  On a CUDA
    device the steps run in HIP; device "cpu" runs the numpy restatement, query_fn then gets and returns numpy arrays.
    shard=True with torch.distributed initialised: the lattice and the refined list are split over the ranks with
    parallel.shard_range and all-gathered (every rank derives the same refined list from the full lattice)."""
    import torch
    K, _ = dims(R, s)
    band = default_band(R, s, lo, hi) if band is None else float(band)
    if not np.isfinite(band) or band < 0 or not np.isfinite(level):
        raise ValueError(f"band = {band}, level = {level}: both must be finite, band >= 0")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.type == "cpu":
        lat_pts = lattice_points(R, s, "cpu", lo=lo, hi=hi).numpy()
        lattice = np.concatenate([np.asarray(query_fn(lat_pts[None, b:b + step]), dtype=np.float32).reshape(-1)
                                  for b in range(0, K ** 3, step)]).reshape(K, K, K)
        _, dilated = classify_cpu(lattice, level, band)
        coords, idx = refined_points_cpu(dilated, R, s, lo, hi)
        values = np.concatenate([np.zeros(0, np.float32)] + [
            np.asarray(query_fn(coords[None, b:b + step]), dtype=np.float32).reshape(-1)
            for b in range(0, len(idx), step)])
        vol = fill_cpu(lattice, values, idx, R, s)
        n = len(idx)
    else:
        lattice = _query_all(query_fn, lambda b, e: lattice_points(R, s, device, b, e, lo, hi), K ** 3, step, device,
                             shard)
        plan = count(lattice, R, s, level, band)
        coords, _ = emit(plan, lo, hi)
        values = _query_all(query_fn, lambda b, e: coords[b:e], plan.n, step, device, shard)
        vol = fill(plan, lattice, values)
        n = plan.n
    stats = {"lattice": K ** 3, "refined": n, "queried": K ** 3 + n, "fraction": (K ** 3 + n) / R ** 3}
    return vol, stats
