"""Mesh evaluation: Chamfer-L2, precision / recall / F-score and volumetric IoU of a predicted mesh against the ground
truth (the reference's evaluation/eval_util.py:eval_mesh, implicit_waterproofing.py and libmesh/inside_mesh.py).

The device functions run through liblist_hip.so (include/list_eval.h) on the tensors' device; every `*_cpu` function is
the same computation in numpy -- the CPU fallback and the test oracle:

  * nn_distance: the nearest dst point of every src point (distance_p2p without normals).  The device computes the
    distance in float32 from explicit differences; nn_distance_cpu is scipy's cKDTree in float64.
  * sample_surface: area-weighted surface samples with counter-based uniforms (splitmix64 of the seed and the sample
    index, recipe in list_eval.h), so a (mesh, n, seed) gives the same points on both sides, bar faces whose cdf
    boundary lies within the rounding of the two scans.
  * mesh_contains / implicit_waterproofing: the reference's parity ray test on its 2-D triangle hash, in float64; the
    device reproduces the numpy restatement bit for bit.
  * eval_pointcloud / eval_mesh: the reference's dict, keys, formulas and quirks included.  eval_mesh samples the
    prediction with `seed`, the ground truth with `seed + 1`, and draws the IoU points in the box from `seed + 2`.
"""
import ctypes as C
import math
import os

import numpy as np

from . import hip
from .mesh import Mesh

EVAL_EXPORTS = {
    "list_eval_nn": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "list_eval_sample_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "list_eval_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p,
                                   C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "list_eval_contains_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "list_eval_contains": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "list_eval_last_error": (C.c_char_p, []),
}
INSIDE, HOLE, REFUSED = 1, 2, 128                         # enum ListEvalFlags
THRESHOLDS = (0.005, 0.01, 0.05)
# implicit_waterproofing.py:33: the Euler angles of the retries
EULER_RETRIES = ((0.0, math.pi / 2, 0.0), (math.pi / 2, 0.0, 0.0), (0.0, 0.0, math.pi / 2))

_section = hip.Section(EVAL_EXPORTS, "list_eval_last_error")    # include/list_eval.h on hip.load()'s handle
load, _check = _section.load, _section.check


# ---- counter-based uniforms (list_eval.h) ---------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def splitmix64(x):
    """splitmix64 of a Python int or a uint64 array (wrapping uint64 arithmetic)."""
    if isinstance(x, (int, np.integer)):
        z = (int(x) + 0x9E3779B97F4A7C15) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)
    z = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform_cpu(seed, counters):
    """u(counter) = (splitmix64(splitmix64(seed) ^ counter) >> 11) * 2^-53, float64 in [0, 1)."""
    key = np.uint64(splitmix64(int(seed) & _M64))
    z = splitmix64(np.asarray(counters, dtype=np.uint64) ^ key)
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _uniform_torch(seed, counters):
    """uniform_cpu on the device: the same uint64 arithmetic in wrapping int64 (shifts made logical by masking)."""
    import torch

    def s64(c):
        return c - (1 << 64) if c >= 1 << 63 else c

    def lsr(z, s):
        return (z >> s) & ((1 << (64 - s)) - 1)

    z = counters.to(torch.int64) ^ s64(splitmix64(int(seed) & _M64))
    z = z + s64(0x9E3779B97F4A7C15)
    z = (z ^ lsr(z, 30)) * s64(0xBF58476D1CE4E5B9)
    z = (z ^ lsr(z, 27)) * s64(0x94D049BB133111EB)
    z = z ^ lsr(z, 31)
    return lsr(z, 11).to(torch.float64) * 2.0 ** -53


def box_samples_cpu(n, bb_min, bb_max, seed):
    """n points uniform in the box (eval_util.py:43-44), float64 [n, 3]: u(3 i + k) * (bb_max - bb_min) + bb_min."""
    u = uniform_cpu(seed, np.arange(3 * n, dtype=np.uint64)).reshape(n, 3)
    lo, hi = np.asarray(bb_min, dtype=np.float64), np.asarray(bb_max, dtype=np.float64)
    return u * (hi - lo) + lo


def box_samples(n, bb_min, bb_max, seed, device):
    import torch
    u = _uniform_torch(seed, torch.arange(3 * n, dtype=torch.int64, device=device)).view(n, 3)
    lo = torch.as_tensor(np.broadcast_to(np.asarray(bb_min, dtype=np.float64), (3,)).copy(), device=device)
    hi = torch.as_tensor(np.broadcast_to(np.asarray(bb_max, dtype=np.float64), (3,)).copy(), device=device)
    return u * (hi - lo) + lo


# ---- mesh files -----------------------------------------------------------------------------------------------------
def _fan(polys):
    tris = []
    for p in polys:
        for k in range(1, len(p) - 1):
            tris.append((p[0], p[k], p[k + 1]))
    return np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def _load_obj(path):
    verts, polys = [], []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                nv = len(verts)
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    idx.append(i - 1 if i > 0 else nv + i)        # 1-based; negative: relative to the end
                polys.append(idx)
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), _fan(polys)


def _load_off(path):
    with open(path) as f:
        tokens = []
        for line in f:
            line = line.split("#")[0].strip()
            if line:
                tokens.extend(line.split())
    if not tokens or not tokens[0].endswith("OFF"):
        raise ValueError(f"{path}: not an OFF file")
    nv, nf = int(tokens[1]), int(tokens[2])
    pos = 4
    verts = np.asarray(tokens[pos:pos + 3 * nv], dtype=np.float64).reshape(nv, 3)
    pos += 3 * nv
    polys = []
    for _ in range(nf):
        k = int(tokens[pos])
        polys.append([int(t) for t in tokens[pos + 1:pos + 1 + k]])
        pos += 1 + k
    return verts, _fan(polys)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4",
              "float32": "f4", "double": "f8", "float64": "f8"}


def _load_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header")
    body = data.index(b"\n", end) + 1
    header = data[:end].decode("ascii").splitlines()
    fmt, elements = None, []
    for line in header:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], ("list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    verts = np.zeros((0, 3))
    if fmt == "ascii":
        rows = [r.split() for r in data[body:].decode("ascii").splitlines() if r.strip()]
        r, vlist, polys = 0, [], []
        for name, count, props in elements:
            names = [p[0] for p in props]
            for vals in rows[r:r + count]:
                if name == "vertex":
                    vlist.append([float(vals[names.index(a)]) for a in ("x", "y", "z")])
                elif name == "face":
                    polys.append([int(x) for x in vals[1:1 + int(vals[0])]])
            r += count
        return np.asarray(vlist, dtype=np.float64).reshape(-1, 3), _fan(polys)
    if fmt not in ("binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: PLY format {fmt} not supported")
    e = "<" if fmt == "binary_little_endian" else ">"
    pos = body
    faces = np.zeros((0, 3), dtype=np.int64)
    for name, count, props in elements:
        if all(not isinstance(t, tuple) for _, t in props):
            dt = np.dtype([(n, e + t) for n, t in props])
            arr = np.frombuffer(data, dtype=dt, count=count, offset=pos)
            pos += dt.itemsize * count
            if name == "vertex":
                verts = np.stack([arr["x"], arr["y"], arr["z"]], axis=1).astype(np.float64)
            continue
        if name != "face" or len(props) != 1:
            raise ValueError(f"{path}: PLY element {name} with list properties not supported")
        _, (_, ct, it) = props[0]
        ct, it = np.dtype(e + ct), np.dtype(e + it)
        k = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0]) if count else 3
        dt = np.dtype([("n", ct), ("i", it, (k,))])
        arr = np.frombuffer(data, dtype=dt, count=count, offset=pos) if count else np.zeros(0, dt)
        if np.all(arr["n"] == k):                                      # every face has the same size
            pos += dt.itemsize * count
            faces = _fan(arr["i"].astype(np.int64))
        else:
            polys = []
            for _ in range(count):
                k = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
                pos += ct.itemsize
                polys.append(np.frombuffer(data, dtype=it, count=k, offset=pos).astype(np.int64).tolist())
                pos += it.itemsize * k
            faces = _fan(polys)
    return verts, faces


def load_mesh(path):
    """A triangle mesh from .obj (v / f lines, `v/vt/vn` tokens, polygons fanned), .off or .ply (ascii or binary) ->
    mesh.Mesh (float32 vertices, int32 faces)."""
    ext = os.path.splitext(str(path))[1].lower()
    loader = {".obj": _load_obj, ".off": _load_off, ".ply": _load_ply}.get(ext)
    if loader is None:
        raise ValueError(f"{path}: load_mesh reads .obj, .off or .ply")
    verts, faces = loader(path)
    return Mesh(verts, faces)


def as_mesh(m, what="mesh"):
    if m is None:
        raise ValueError(f"{what} is None: evaluation needs a mesh or a path to one")
    if isinstance(m, Mesh):
        return m
    if isinstance(m, (str, os.PathLike)):
        return load_mesh(m)
    if hasattr(m, "vertices") and hasattr(m, "faces"):
        return Mesh(np.asarray(m.vertices), np.asarray(m.faces))
    raise ValueError(f"{what}: expected a Mesh or a path, got {type(m).__name__}")


# ---- device ---------------------------------------------------------------------------------------------------------
def _dev_tensor(t, dtype, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor (got {type(t).__name__} {getattr(t, 'device', None)})")
    return t.to(dtype).contiguous()


def nn_distance(src, dst):
    """For every src point (float32 [N,3] device tensor) the distance to its nearest dst point [M,3] and that point's
    index (smallest on ties) -> (dist float32 [N], idx int32 [N]) on the device."""
    import torch
    src, dst = _dev_tensor(src, torch.float32, "src").view(-1, 3), _dev_tensor(dst, torch.float32, "dst").view(-1, 3)
    N, M = src.shape[0], dst.shape[0]
    dist = torch.empty((N,), dtype=torch.float32, device=src.device)
    idx = torch.empty((N,), dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _check(load().list_eval_nn(src.data_ptr() if N else None, N, dst.data_ptr() if M else None, M,
                                   dist.data_ptr() if N else None, idx.data_ptr() if N else None, hip._stream()),
               "list_eval_nn")
    return dist, idx


def _mesh_tensors(verts, faces):
    import torch
    v = _dev_tensor(verts, torch.float32, "verts").view(-1, 3)
    f = _dev_tensor(faces, torch.int32, "faces").view(-1, 3)
    return v, f


def sample_surface(verts, faces, n, seed=0):
    """n area-weighted samples on the surface of a device mesh -> (points float32 [n,3], face_idx int32 [n])."""
    import torch
    v, f = _mesh_tensors(verts, faces)
    lib, dev = load(), v.device
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_eval_sample_workspace_bytes(f.shape[0]), "list_eval_sample_workspace_bytes")
        points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        face_idx = torch.empty((n,), dtype=torch.int32, device=dev)
        _check(lib.list_eval_sample(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], n, int(seed) & _M64,
                                    ws.data_ptr(), ws.numel(), points.data_ptr() if n else None,
                                    face_idx.data_ptr() if n else None, hip._stream()), "list_eval_sample")
        if n and int(face_idx[0]) < 0:
            raise hip.ListError("list_eval_sample", hip.ERR_SHAPE, "the mesh has no positive, finite surface area")
    return points, face_idx


def _contains_flags(v, f, points, hash_res, rot):
    import torch
    lib, dev = load(), v.device
    p = _dev_tensor(points, torch.float64, "points").view(-1, 3)
    Q = p.shape[0]
    flags = torch.empty((Q,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_eval_contains_workspace_bytes(f.shape[0], int(hash_res)), "list_eval_contains_workspace_bytes")
        r = None if rot is None else torch.as_tensor(np.asarray(rot, dtype=np.float64).reshape(9), device=dev)
        _check(lib.list_eval_contains(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], p.data_ptr() if Q else None,
                                      Q, None if r is None else r.data_ptr(), int(hash_res), ws.data_ptr(), ws.numel(),
                                      flags.data_ptr() if Q else None, hip._stream()), "list_eval_contains")
        if Q and int(flags[0]) & REFUSED:
            raise hip.ListError("list_eval_contains", hip.ERR_SHAPE, "the triangles' bounding box has a zero extent")
    return flags


def mesh_contains(verts, faces, points, hash_res=512, rot=None):
    """MeshIntersector.query on the device: points float64 [Q,3] -> (contains bool [Q], hole bool [Q]).
    rot: optional 3x3 applied to the mesh and the points before the test."""
    v, f = _mesh_tensors(verts, faces)
    flags = _contains_flags(v, f, points, hash_res, rot)
    return (flags & INSIDE) != 0, (flags & HOLE) != 0


def implicit_waterproofing(verts, faces, points, hash_res=512):
    """implicit_waterproofing.py on the device: the inside test, retried under three rotations for the points whose
    two parities disagree (holes), until none is left -> (occupancy bool [Q], hole bool [Q]).  Counting the holes
    synchronises once per round."""
    import torch
    v, f = _mesh_tensors(verts, faces)
    points = _dev_tensor(points, torch.float64, "points").view(-1, 3)
    occ, hole = mesh_contains(v, f, points, hash_res)
    for euler in EULER_RETRIES:
        sel = torch.nonzero(hole).squeeze(1)
        if sel.numel() == 0:
            break
        o, h = mesh_contains(v, f, points[sel], hash_res, rot=rotation_matrix(euler))
        occ[sel] = o
        hole = torch.zeros_like(hole)
        hole[sel] = h
    return occ, hole


def eval_pointcloud(pointcloud_pred, pointcloud_gt):
    """eval_util.py:eval_pointcloud without normals, on the device: the reference's dict of Python floats."""
    import torch
    pred, gt = _dev_tensor(pointcloud_pred, torch.float32, "pred"), _dev_tensor(pointcloud_gt, torch.float32, "gt")
    completeness, _ = nn_distance(gt, pred)
    accuracy, _ = nn_distance(pred, gt)
    return _finish_pointcloud(*_pointcloud_stats(completeness, accuracy), len(pred))


def _pointcloud_stats(completeness, accuracy):
    import torch
    c, a = completeness.double(), accuracy.double()
    moments = torch.stack([c.mean(), a.mean(), (c * c).mean(), (a * a).mean()])
    counts = torch.stack([(c < p).sum() for p in THRESHOLDS] + [(a < p).sum() for p in THRESHOLDS])
    return moments, counts


def _finish_pointcloud(moments, counts, n_pred):
    if hasattr(moments, "tolist"):
        moments, counts = moments.tolist(), [int(x) for x in counts.tolist()]
    completeness, accuracy, completeness2, accuracy2 = (float(x) for x in moments)
    out = {"completeness": completeness, "accuracy": accuracy, "completeness2": completeness2,
           "accuracy2": accuracy2, "chamfer_l2": (0.5 * completeness2 + 0.5 * accuracy2) * 10000}
    precision = {"precision_" + str(p * 100): counts[i] / n_pred for i, p in enumerate(THRESHOLDS)}
    recall = {"recall_" + str(p * 100): counts[3 + i] / n_pred for i, p in enumerate(THRESHOLDS)}
    fscore = {}
    for p in THRESHOLDS:
        pr, rc = precision["precision_" + str(p * 100)], recall["recall_" + str(p * 100)]
        fscore["fscore_" + str(p * 100)] = 2 * (pr * rc) / (pr + rc + 1e-5)
    out.update(precision)
    out.update(recall)
    out.update(fscore)
    return out


def eval_mesh(mesh_pred, mesh_gt, bb_min, bb_max, n_points=100000, seed=0, device=None, hash_res=512):
    """eval_util.py:eval_mesh: the point-cloud metrics of n_points surface samples of each mesh, plus the IoU of the
    two occupancies over 10 * n_points uniform samples of the box.  Meshes: mesh.Mesh or paths.  device: a CUDA/HIP
    device runs everything there (Python floats come back); None or "cpu" runs the numpy restatement.
    Returns {} when the prediction has fewer than 10 vertices."""
    mesh_pred, mesh_gt = as_mesh(mesh_pred, "pred mesh"), as_mesh(mesh_gt, "gt mesh")
    if len(mesh_pred.vertices) < 10:
        return {}
    import torch
    if device is None or torch.device(device).type == "cpu":
        return eval_mesh_cpu(mesh_pred, mesh_gt, bb_min, bb_max, n_points, seed, hash_res)
    dev = torch.device(device)
    vp, fp = (torch.from_numpy(a).to(dev) for a in (mesh_pred.vertices, mesh_pred.faces))
    vg, fg = (torch.from_numpy(a).to(dev) for a in (mesh_gt.vertices, mesh_gt.faces))
    pc_pred, _ = sample_surface(vp, fp, n_points, seed)
    pc_gt, _ = sample_surface(vg, fg, n_points, seed + 1)
    completeness, _ = nn_distance(pc_gt, pc_pred)
    accuracy, _ = nn_distance(pc_pred, pc_gt)
    moments, counts = _pointcloud_stats(completeness, accuracy)
    samples = box_samples(10 * n_points, bb_min, bb_max, seed + 2, dev)
    occ_pred = implicit_waterproofing(vp, fp, samples, hash_res)[0]
    occ_gt = implicit_waterproofing(vg, fg, samples, hash_res)[0]
    areas = torch.stack([(occ_pred | occ_gt).sum(), (occ_pred & occ_gt).sum()]).tolist()
    out = _finish_pointcloud(moments, counts, n_points)
    out["iou"] = _iou(areas[1], areas[0])
    return out


def _iou(intersect, union):
    # (area_intersect / area_union) of two float32 sums: nan for an empty union, as numpy gives with a warning
    return float(np.float32(intersect) / np.float32(union)) if union else float("nan")


# ---- host -----------------------------------------------------------------------------------------------------------
def _host(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def nn_distance_cpu(src, dst):
    """distance_p2p: cKDTree in float64 -> (dist float64 [N], idx int64 [N])."""
    from scipy.spatial import cKDTree
    src, dst = _host(src, np.float64).reshape(-1, 3), _host(dst, np.float64).reshape(-1, 3)
    if len(dst) == 0:
        raise hip.ListError("nn_distance_cpu", hip.ERR_SHAPE, "M = 0 dst points")
    dist, idx = cKDTree(dst).query(src)
    return dist, idx


def _valid_faces(faces, n_verts):
    return np.all((faces >= 0) & (faces < n_verts), axis=1)


def sample_surface_cpu(verts, faces, n, seed=0):
    """sample_surface restated in numpy -> (points float32 [n,3], face_idx int32 [n])."""
    v, f = _host(verts, np.float32).reshape(-1, 3), _host(faces, np.int32).reshape(-1, 3)
    if len(f) == 0:
        raise hip.ListError("sample_surface_cpu", hip.ERR_SHAPE, "0 faces")
    ok = _valid_faces(f, len(v))
    fs = np.where(ok[:, None], f, 0)
    p = v.astype(np.float64)[fs]                                   # [F, 3 corners, 3 axes]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = np.where(ok, 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz), 0.0)
    cdf = np.cumsum(area)
    total = cdf[-1]
    if not (total > 0 and np.isfinite(total)):
        raise hip.ListError("sample_surface_cpu", hip.ERR_SHAPE, "the mesh has no positive, finite surface area")
    u = uniform_cpu(seed, np.arange(3 * n, dtype=np.uint64)).reshape(n, 3)
    face = np.searchsorted(cdf, u[:, 0] * total, side="right")
    face = np.where(face == len(f), np.searchsorted(cdf, total, side="left"), face)
    r = np.sqrt(u[:, 1])
    a, b, c = 1.0 - r, r * (1.0 - u[:, 2]), r * u[:, 2]
    t = p[face]
    points = (a[:, None] * t[:, 0] + b[:, None] * t[:, 1]) + c[:, None] * t[:, 2]
    return points.astype(np.float32), face.astype(np.int32)


def rotation_matrix(euler):
    """implicit_waterproofing.py:to_rotation_matrix: R = Rz . Ry . Rx (float64 3x3)."""
    ax, ay, az = euler
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return np.dot(rz, np.dot(ry, rx))


def _rotate(R, x, y, z):
    if R is None:
        return x, y, z
    return tuple((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z for r in range(3))


def _cell_clamp(x, res):
    return np.where(x >= 1.0, np.minimum(x, res - 1), 0.0).astype(np.int64)


def _hits(t, px, py, pz):
    """check_triangles and the depth test of (point, triangle) pairs: t [K, 9] float64 -> (parity-0 hit, parity-1 hit)."""
    a00, a01, a10, a11 = t[:, 0] - t[:, 6], t[:, 3] - t[:, 6], t[:, 1] - t[:, 7], t[:, 4] - t[:, 7]
    y0, y1 = px - t[:, 6], py - t[:, 7]
    det = a00 * a11 - a01 * a10
    s, ad = np.sign(det), np.abs(det)
    u = (a11 * y0 - a01 * y1) * s
    v = (-a10 * y0 + a00 * y1) * s
    uv = u + v
    inside = (ad != 0) & (0 < u) & (u < ad) & (0 < v) & (v < ad) & (0 < uv) & (uv < ad)
    v1x, v1y, v1z = t[:, 6] - t[:, 0], t[:, 7] - t[:, 1], t[:, 8] - t[:, 2]
    v2x, v2y, v2z = t[:, 3] - t[:, 0], t[:, 4] - t[:, 1], t[:, 5] - t[:, 2]
    n0, n1, n2 = v1y * v2z - v1z * v2y, v1z * v2x - v1x * v2z, v1x * v2y - v1y * v2x
    alpha = n0 * (t[:, 0] - px) + n1 * (t[:, 1] - py)
    an = np.abs(n2)
    depth = t[:, 2] * an + alpha * np.sign(n2)
    zc = pz * an
    ok = inside & (an != 0)
    return ok & (depth >= zc), ok & (depth < zc)


def mesh_contains_cpu(verts, faces, points, hash_res=512, rot=None, chunk=1 << 17):
    """mesh_contains restated in numpy (the same float64 operations in the same order) -> (contains, hole)."""
    v, f = _host(verts, np.float32).reshape(-1, 3), _host(faces, np.int32).reshape(-1, 3)
    pts = _host(points, np.float64).reshape(-1, 3)
    res = int(hash_res)
    if len(f) == 0:
        raise hip.ListError("mesh_contains_cpu", hip.ERR_SHAPE, "0 faces")
    if not 1 <= res <= 8192:
        raise hip.ListError("mesh_contains_cpu", hip.ERR_SHAPE, f"hash_res {res}")
    R = None if rot is None else np.asarray(rot, dtype=np.float64).reshape(3, 3)
    f = f[_valid_faces(f, len(v))]
    c = v.astype(np.float64)[f]                                    # [F, 3, 3]
    tri = np.stack(_rotate(R, c[..., 0], c[..., 1], c[..., 2]), axis=-1)
    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
    ext = hi - lo
    if len(f) == 0 or not np.all((ext > 0) & np.isfinite(ext)):
        raise hip.ListError("mesh_contains_cpu", hip.ERR_SHAPE, "the triangles' bounding box has a zero extent")
    scale = (res - 1) / ext
    translate = 0.5 - scale * lo
    tri = (scale * tri + translate).reshape(-1, 9)
    x0, x1 = _cell_clamp(tri[:, 0::3].min(axis=1), res), _cell_clamp(tri[:, 0::3].max(axis=1), res)
    y0, y1 = _cell_clamp(tri[:, 1::3].min(axis=1), res), _cell_clamp(tri[:, 1::3].max(axis=1), res)
    # the hash: (cell, triangle) for every cell of every triangle's bbox, sorted by cell
    w, h = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    n_cells = w * h
    tri_of = np.repeat(np.arange(len(tri)), n_cells)
    k = np.arange(len(tri_of)) - np.repeat(np.cumsum(n_cells) - n_cells, n_cells)
    cell = (x0[tri_of] + k // h[tri_of]) * res + (y0[tri_of] + k % h[tri_of])
    order = np.argsort(cell, kind="stable")
    cell, tri_of = cell[order], tri_of[order]

    contains = np.zeros(len(pts), dtype=bool)
    hole = np.zeros(len(pts), dtype=bool)
    for s in range(0, len(pts), chunk):
        x, y, z = _rotate(R, pts[s:s + chunk, 0], pts[s:s + chunk, 1], pts[s:s + chunk, 2])
        px, py, pz = scale[0] * x + translate[0], scale[1] * y + translate[1], scale[2] * z + translate[2]
        keep = (0 <= px) & (px <= res) & (0 <= py) & (py <= res) & (0 <= pz) & (pz <= res)
        q = np.flatnonzero(keep)
        cx, cy = px[q].astype(np.int64), py[q].astype(np.int64)
        good = (cx < res) & (cy < res)
        q, cx, cy = q[good], cx[good], cy[good]
        qc = cx * res + cy
        b, e = np.searchsorted(cell, qc, "left"), np.searchsorted(cell, qc, "right")
        cnt = e - b
        pq = np.repeat(q, cnt)
        j = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(b, cnt)
        h0, h1 = _hits(tri[tri_of[j]], px[pq], py[pq], pz[pq])
        n0 = np.bincount(pq[h0], minlength=len(px)) & 1
        n1 = np.bincount(pq[h1], minlength=len(px)) & 1
        contains[s:s + chunk] = (n0 == 1) & (n1 == 1)
        hole[s:s + chunk] = n0 != n1
    return contains, hole


def implicit_waterproofing_cpu(verts, faces, points, hash_res=512):
    """implicit_waterproofing restated in numpy -> (occupancy, hole)."""
    pts = _host(points, np.float64).reshape(-1, 3)
    occ, hole = mesh_contains_cpu(verts, faces, pts, hash_res)
    for euler in EULER_RETRIES:
        if not hole.any():
            break
        sel = np.flatnonzero(hole)
        o, h = mesh_contains_cpu(verts, faces, pts[sel], hash_res, rot=rotation_matrix(euler))
        occ[sel] = o
        hole = np.zeros_like(hole)
        hole[sel] = h
    return occ, hole


def eval_pointcloud_cpu(pointcloud_pred, pointcloud_gt):
    """eval_util.py:eval_pointcloud without normals, in numpy / cKDTree."""
    pred, gt = _host(pointcloud_pred, np.float32).reshape(-1, 3), _host(pointcloud_gt, np.float32).reshape(-1, 3)
    completeness, _ = nn_distance_cpu(gt, pred)
    accuracy, _ = nn_distance_cpu(pred, gt)
    moments = [completeness.mean(), accuracy.mean(), (completeness ** 2).mean(), (accuracy ** 2).mean()]
    counts = [int(np.count_nonzero(completeness < p)) for p in THRESHOLDS] + \
        [int(np.count_nonzero(accuracy < p)) for p in THRESHOLDS]
    return _finish_pointcloud(moments, counts, len(pred))


def eval_mesh_cpu(mesh_pred, mesh_gt, bb_min, bb_max, n_points=100000, seed=0, hash_res=512):
    """eval_mesh restated in numpy."""
    mesh_pred, mesh_gt = as_mesh(mesh_pred, "pred mesh"), as_mesh(mesh_gt, "gt mesh")
    if len(mesh_pred.vertices) < 10:
        return {}
    pc_pred, _ = sample_surface_cpu(mesh_pred.vertices, mesh_pred.faces, n_points, seed)
    pc_gt, _ = sample_surface_cpu(mesh_gt.vertices, mesh_gt.faces, n_points, seed + 1)
    out = eval_pointcloud_cpu(pc_pred, pc_gt)
    samples = box_samples_cpu(10 * n_points, bb_min, bb_max, seed + 2)
    occ_pred = implicit_waterproofing_cpu(mesh_pred.vertices, mesh_pred.faces, samples, hash_res)[0]
    occ_gt = implicit_waterproofing_cpu(mesh_gt.vertices, mesh_gt.faces, samples, hash_res)[0]
    out["iou"] = _iou(int(np.count_nonzero(occ_pred & occ_gt)), int(np.count_nonzero(occ_pred | occ_gt)))
    return out
