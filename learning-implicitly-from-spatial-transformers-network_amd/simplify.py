"""Simplify a triangle mesh by uniform-grid vertex clustering (Rossignac-Borrel): the marching-cubes mesh of a smooth
surface is almost all voxel-sized facets; this merges the vertices of one grid cell into one.

`simplify` runs on the tensors' device through liblist_hip.so (include/list_simplify.h) when it is given CUDA tensors;
`simplify_cpu` is the same rule in numpy -- the CPU fallback and the test oracle.  Both give, exactly:

  * inputs: verts float32 [V,3], faces int32 [F,3], 0 <= V, F <= INT32_MAX; cells = (R0,R1,R2), each 1 <= Ra <= 1024 (an
    int means the same on all axes); bounds lo[a] < hi[a], finite, float64 (scalars or one value per axis, default
    -0.5 / 0.5, as mesh.marching_cubes takes them).  inv[a] = Ra / (hi[a] - lo[a]) and cell[a] = (hi[a] - lo[a]) / Ra
    are computed here in float64 and handed to the device as doubles, so both sides hold the same bits;
  * per vertex and axis, in float64 with every operation rounded on its own (no fused multiply-add):
    t = (double)v - lo; u = clamp(t * inv, 0, R) (a vertex outside the box goes onto the box face);
    i = min((int64)floor(u), R - 1); q = rint((u - i) * 2^30), ties to even, 0 <= q <= 2^30;
    key = (i0 * R1 + i1) * R2 + i2 < 2^30;
  * a vertex with a non-finite coordinate is invalid: in no cluster.  A face with an index outside [0, V) or with an
    invalid corner is invalid: never in the output, its index never used as an address;
  * a cluster is the set of valid vertices with one key; clusters are numbered in ascending key (np.unique).  Per
    cluster and axis S = sum of q (int64) and n = count; its representative, every integer-to-double conversion exact:
    a = S // n, r = S % n; m = ((double)a + (double)r / (double)n) * 2^-30; p = (float)(lo + ((double)i + m) * cell);
  * a valid face whose three corners do not lie in three different clusters is degenerate and dropped; every other
    valid face is kept, in its order and orientation, with cluster numbers for corners.  Duplicate faces and opposite
    pairs (a,b,c) / (a,c,b) stay: a vertex map sends a closed surface to a mod-2 cycle, so every edge of the output of
    a closed input lies in an even number of faces (evaluate.mesh_contains' parity test stays meaningful);
  * clusters that no kept face uses are dropped, the rest renumbered in ascending key: V' vertices, F' faces;
  * info: n_verts (V'), n_faces (F'), clusters, invalid_verts, invalid_faces, degenerate_faces, and vertex_map int32 [V]
    (the output vertex of each input vertex, -1 if it is invalid or its cluster was dropped).

Every output is a function of the inputs alone, bit for bit, and does not depend on the order of the input vertices; the
faces follow the input face order."""
import ctypes as C

import numpy as np

from . import hip

INT32_MAX = 2 ** 31 - 1
MAX_CELLS = 1024                # LIST_SIMP_MAX_CELLS
TOTALS = ("n_verts", "n_faces", "clusters", "invalid_verts", "invalid_faces", "degenerate_faces")     # the int64[6]
Q_ONE = float(2 ** 30)

SIMPLIFY_EXPORTS = {
    "list_simp_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_void_p]),
    "list_simp_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "list_simp_emit": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "list_simp_last_error": (C.c_char_p, []),
}

_section = hip.Section(SIMPLIFY_EXPORTS, "list_simp_last_error")    # include/list_simplify.h on hip.load()'s handle
load, _check = _section.load, _section.check


# ---- the grid (host, both paths) ------------------------------------------------------------------------------------
def check_cells(cells):
    """cells as three ints in [1, 1024]; an int means the same on all axes."""
    c = np.asarray(cells)
    if c.dtype == bool or c.dtype.kind not in "iu" or c.shape not in ((), (3,)):
        raise ValueError(f"cells must be an integer or three integers (got {cells!r})")
    c = np.broadcast_to(c.astype(np.int64), (3,))
    if (c < 1).any() or (c > MAX_CELLS).any():
        raise ValueError(f"cells must be in [1, {MAX_CELLS}] on every axis (got {cells!r})")
    return tuple(int(x) for x in c)


def grid(cells, bb_min=-0.5, bb_max=0.5):
    """(R int64 [3], lo, inv, cell float64 [3]): the numbers both paths compute with."""
    R = np.array(check_cells(cells), dtype=np.int64)
    lo = np.broadcast_to(np.asarray(bb_min, dtype=np.float64), (3,)).copy()
    hi = np.broadcast_to(np.asarray(bb_max, dtype=np.float64), (3,)).copy()
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"bb_min and bb_max must be finite (got {bb_min!r}, {bb_max!r})")
    with np.errstate(over="ignore"):
        ext = hi - lo
    if not (lo < hi).all() or not np.isfinite(ext).all():
        raise ValueError(f"bb_min must be below bb_max on every axis, the box finite (got {bb_min!r}, {bb_max!r})")
    inv, cell = R.astype(np.float64) / ext, ext / R.astype(np.float64)
    if not (np.isfinite(inv).all() and (cell > 0).all()):
        raise ValueError(f"the box [{bb_min!r}, {bb_max!r}] is too thin for {cells!r} cells")
    return R, lo, inv, cell


def _info(totals, vertex_map):
    info = {k: int(x) for k, x in zip(TOTALS, totals)}
    info["vertex_map"] = vertex_map
    return info


# ---- device ---------------------------------------------------------------------------------------------------------
def _is_cuda(x):
    return hasattr(x, "is_cuda") and x.is_cuda


def _dev_inputs(verts, faces):
    import torch
    hip._f32_cuda(verts, "verts")
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or not faces.is_cuda:
        raise RuntimeError(f"faces must be an int32 CUDA/HIP tensor (got {type(faces).__name__} "
                           f"{getattr(faces, 'dtype', None)} {getattr(faces, 'device', None)})")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise hip.ListError("simplify", hip.ERR_SHAPE, f"verts of shape {tuple(verts.shape)}: need [V,3]")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise hip.ListError("simplify", hip.ERR_SHAPE, f"faces of shape {tuple(faces.shape)}: need [F,3]")
    if faces.device != verts.device:
        raise RuntimeError(f"verts on {verts.device}, faces on {faces.device}")
    if len(verts) > INT32_MAX or len(faces) > INT32_MAX:
        raise hip.ListError("simplify", hip.ERR_SHAPE, f"V = {len(verts)}, F = {len(faces)}: both must be in [0, INT32_MAX]")
    return verts.contiguous(), faces.contiguous()


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def simplify(verts, faces, cells, bb_min=-0.5, bb_max=0.5):
    """The mesh with the vertices of every grid cell merged into one (the module's rule) ->
    (verts' float32 [V',3], faces' int32 [F',3], info).

    CUDA tensors (verts float32 [V,3], faces int32 [F,3], one device) take the HIP path on their device and current
    stream and get tensors on that device (info's vertex_map too); another dtype is refused (RuntimeError), another
    shape is refused (hip.ListError, ERR_SHAPE), non-contiguous tensors are copied.  CPU tensors and array-likes go to
    simplify_cpu, which converts them and gives numpy arrays.  cells outside [1, 1024] and non-finite or empty bounds
    are refused (ValueError) on both paths.  The one host synchronisation reads the six totals back."""
    if not (_is_cuda(verts) and _is_cuda(faces)):
        if _is_cuda(verts) or _is_cuda(faces):
            raise RuntimeError("verts and faces must both be CUDA/HIP tensors, or neither")
        return simplify_cpu(verts, faces, cells, bb_min, bb_max)
    import torch
    R, lo, inv, cell = grid(cells, bb_min, bb_max)
    verts, faces = _dev_inputs(verts, faces)
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), verts.device
    lib = load()
    cR, clo = (C.c_int32 * 3)(*R.tolist()), (C.c_double * 3)(*lo.tolist())
    cinv, ccell = (C.c_double * 3)(*inv.tolist()), (C.c_double * 3)(*cell.tolist())
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_simp_workspace_bytes(V, F, cR), "list_simp_workspace_bytes")
        vmap = torch.empty((V,), dtype=torch.int32, device=dev)
        totals = torch.empty((len(TOTALS),), dtype=torch.int64, device=dev)
        stream = hip._stream()
        _check(lib.list_simp_count(_ptr(verts), _ptr(faces), V, F, cR, clo, cinv, ws.data_ptr(), ws.numel(), _ptr(vmap),
                                   totals.data_ptr(), stream), "list_simp_count")
        info = _info(totals.tolist(), vmap)                      # the read-back
        Vo, Fo = info["n_verts"], info["n_faces"]
        out_v = torch.empty((Vo, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((Fo, 3), dtype=torch.int32, device=dev)
        _check(lib.list_simp_emit(_ptr(faces), V, F, cR, clo, ccell, _ptr(vmap), ws.data_ptr(), ws.numel(), _ptr(out_v),
                                  Vo, _ptr(out_f), Fo, stream), "list_simp_emit")
    return out_v, out_f, info


# ---- host -----------------------------------------------------------------------------------------------------------
def vertex_cells(v, R, lo, inv):
    """The per-vertex rule on float32 [V,3] -> (valid bool [V], i int64 [V,3], q int64 [V,3], key int64 [V]); the rows
    of an invalid vertex hold what the origin would get."""
    valid = np.isfinite(v).all(axis=1)
    t = np.where(valid[:, None], v, np.float32(0)).astype(np.float64) - lo
    u = np.minimum(np.maximum(t * inv, 0.0), R.astype(np.float64))
    i = np.minimum(np.floor(u).astype(np.int64), R - 1)
    q = np.rint((u - i.astype(np.float64)) * Q_ONE).astype(np.int64)
    key = (i[:, 0] * R[1] + i[:, 1]) * R[2] + i[:, 2]
    return valid, i, q, key


def cluster_points(S, n, i, lo, cell):
    """The representatives of clusters with sums S int64 [K,3], counts n int64 [K] in cells i int64 [K,3] -> float32 [K,3]."""
    n = n[:, None]
    a, r = S // n, S % n
    m = (a.astype(np.float64) + r.astype(np.float64) / n.astype(np.float64)) * (1.0 / Q_ONE)
    return (lo + (i.astype(np.float64) + m) * cell).astype(np.float32)


def simplify_cpu(verts, faces, cells, bb_min=-0.5, bb_max=0.5):
    """simplify restated in numpy -> (verts' float32 [V',3], faces' int32 [F',3], info), all on the host.  verts:
    array-like [V,3] (converted to float32), faces: array-like [F,3] of any integer dtype; tensors are copied."""
    R, lo, inv, cell = grid(cells, bb_min, bb_max)
    if hasattr(verts, "detach"):
        verts = verts.detach().cpu().numpy()
    if hasattr(faces, "detach"):
        faces = faces.detach().cpu().numpy()
    v = np.asarray(verts)
    if v.size == 0:
        v = np.zeros((0, 3), dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"verts of shape {v.shape}: need [V,3]")
    v = np.ascontiguousarray(v, dtype=np.float32)
    f = np.asarray(faces)
    if f.size == 0:
        f = np.zeros((0, 3), dtype=np.int64)
    if f.dtype.kind not in "iu":
        raise TypeError(f"faces must hold integers (got {f.dtype})")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces of shape {f.shape}: need [F,3]")
    f = f.astype(np.int64)
    V = len(v)
    if V > INT32_MAX or len(f) > INT32_MAX:
        raise ValueError(f"V = {V}, F = {len(f)}: both must be in [0, INT32_MAX]")

    valid, i, q, key = vertex_cells(v, R, lo, inv)
    keys, inverse = np.unique(key[valid], return_inverse=True)           # ascending key: the cluster numbers
    K = len(keys)
    cluster = np.full(V, -1, dtype=np.int64)
    cluster[valid] = inverse.reshape(-1)
    order = np.argsort(cluster[valid], kind="stable")
    n = np.bincount(cluster[valid], minlength=K).astype(np.int64)
    S = (np.add.reduceat(q[valid][order], np.cumsum(n) - n, axis=0) if K else np.zeros((0, 3), dtype=np.int64))

    in_range = ((f >= 0) & (f < V)).all(axis=1)
    cf = np.full(f.shape, -1, dtype=np.int64)
    cf[in_range] = cluster[f[in_range]]
    fvalid = (cf >= 0).all(axis=1)
    distinct = (cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 0] != cf[:, 2])
    kept = cf[fvalid & distinct]
    used = np.zeros(K, dtype=bool)
    used[kept.ravel()] = True
    cmap = np.cumsum(used) - 1

    ci = np.stack([keys // (R[1] * R[2]), (keys // R[2]) % R[1], keys % R[2]], axis=1)
    out_v = cluster_points(S[used], n[used], ci[used], lo, cell).reshape(-1, 3)
    out_f = cmap[kept].astype(np.int32).reshape(-1, 3)
    vmap = np.full(V, -1, dtype=np.int32)
    mapped = valid.copy()
    mapped[valid] = used[cluster[valid]]
    vmap[mapped] = cmap[cluster[mapped]]
    totals = (len(out_v), len(out_f), K, int((~valid).sum()), int((~fvalid).sum()), int((fvalid & ~distinct).sum()))
    return out_v, out_f, _info(totals, vmap)
