"""Training-data preparation: the files the file-backed datasets read, made from raw meshes (the reference's
preprocessing/preprocess.py and preprocessing/farthest_pointcloud.py, which need trimesh, igl, pytorch3d and h5py).

The device functions run through liblist_hip.so (include/list_data.h) on the tensors' device; every `*_cpu` function
is the same computation in numpy -- the CPU fallback and the test oracle:

  * signed_distance: the exact distance to the closest triangle (float32), negative where the generalised winding
    number is > 0.5.  The restatement computes the distance with the device's float32 operations and the winding
    number in float64.
  * boundary_samples: points + sigma * n, n standard normal from Box-Muller over the counter-based uniforms of
    list_eval.h, so that a (points, sigma, seed) gives the same samples on both sides.
  * farthest_points: pytorch3d.ops.sample_farthest_points(random_start_point=False), ties to the smallest index.
  * prepare_shape: isosurf_scaled.obj, sampled_points (grid_points, query_points_sigma_{s}) and farthest_pointclouds
    (points_{n_farthest}) for one mesh; `python -m list_amd.prepare` runs it over a tree of meshes.
"""
import argparse
import ctypes as C
import math
import os
import sys
import traceback
from glob import glob

import numpy as np

from . import evaluate as E
from . import hip
from .mesh import Mesh

DATA_EXPORTS = {
    "list_data_signed_distance_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "list_data_signed_distance": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "list_data_boundary_samples": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p]),
    "list_data_farthest_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "list_data_last_error": (C.c_char_p, []),
}
MAX_FPS_POINTS = 65536                                    # LIST_DATA_MAX_FPS_POINTS
SIGMAS = (0.003, 0.01, 0.07)                              # preprocess.py's --sigma default
_BOUNDARY_BASE = 1 << 63                                  # boundary_samples' counters: 2^63 + 6 i + 2 k (+1)

_section = hip.Section(DATA_EXPORTS, "list_data_last_error")    # include/list_data.h on hip.load()'s handle
load, _check = _section.load, _section.check


def _host(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


# ---- mesh normalisation -----------------------------------------------------------------------------------------------
def scale_mesh(verts, faces):
    """preprocess.py:scale_mesh: centre the bounding box of the referenced vertices at 0 and divide by its largest
    extent (float64, rounded to float32 once); vertex order and faces kept -> mesh.Mesh."""
    v, f = _host(verts, np.float64).reshape(-1, 3), _host(faces, np.int32).reshape(-1, 3)
    used = np.unique(f[E._valid_faces(f, len(v))]) if len(f) else np.arange(len(v))
    ref = v[used] if len(used) else v
    lo, hi = ref.min(axis=0), ref.max(axis=0)
    size = (hi - lo).max()
    if not (size > 0 and np.isfinite(size)):
        raise ValueError("the mesh's bounding box has no positive, finite extent")
    return Mesh(((v - (hi + lo) / 2) * (1.0 / size)).astype(np.float32), f)


# ---- device ---------------------------------------------------------------------------------------------------------
def signed_distance(verts, faces, points, with_winding=False):
    """Signed distance of device points [Q,3] to a device mesh -> (sdf float32 [Q], face_idx int32 [Q], winding
    float32 [Q] or None)."""
    import torch
    v, f = E._mesh_tensors(verts, faces)
    p = E._dev_tensor(points, torch.float32, "points").view(-1, 3)
    lib, dev, Q = load(), v.device, p.shape[0]
    sdf = torch.empty((Q,), dtype=torch.float32, device=dev)
    face_idx = torch.empty((Q,), dtype=torch.int32, device=dev)
    winding = torch.empty((Q,), dtype=torch.float32, device=dev) if with_winding else None
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_data_signed_distance_workspace_bytes(f.shape[0]), "list_data_signed_distance_workspace_bytes")
        _check(lib.list_data_signed_distance(
            v.data_ptr() if v.numel() else None, v.shape[0], f.data_ptr(), f.shape[0], p.data_ptr() if Q else None, Q,
            ws.data_ptr(), ws.numel(), sdf.data_ptr() if Q else None, face_idx.data_ptr() if Q else None,
            winding.data_ptr() if (Q and with_winding) else None, hip._stream()), "list_data_signed_distance")
    return sdf, face_idx, winding


def boundary_samples(points, sigma, seed=0):
    """points + sigma * n on the device (float32 [M,3]); sigma == 0 gives the points unchanged."""
    import torch
    p = E._dev_tensor(points, torch.float32, "points").view(-1, 3)
    out = torch.empty_like(p)
    with torch.cuda.device(p.device):
        _check(load().list_data_boundary_samples(p.data_ptr() if p.numel() else None, p.shape[0], float(sigma),
                                                 int(seed) & E._M64, out.data_ptr() if p.numel() else None,
                                                 hip._stream()), "list_data_boundary_samples")
    return out


def farthest_points(clouds, k):
    """Farthest point sampling of device clouds [B,N,3] (or one [N,3]) -> (points [B,K,3], idx int32 [B,K]), the
    leading dimension dropped again for a single cloud."""
    import torch
    c = E._dev_tensor(clouds, torch.float32, "clouds")
    single = c.dim() == 2
    c = c.view(1, -1, 3) if single else c.view(c.shape[0], -1, 3)
    B, N = c.shape[0], c.shape[1]
    idx = torch.empty((B, max(int(k), 0)), dtype=torch.int32, device=c.device)
    with torch.cuda.device(c.device):
        _check(load().list_data_farthest_points(c.data_ptr() if c.numel() else None, B, N, int(k),
                                                idx.data_ptr() if idx.numel() else None, hip._stream()),
               "list_data_farthest_points")
    pts = torch.gather(c, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
    return (pts[0], idx[0]) if single else (pts, idx)


# ---- host -----------------------------------------------------------------------------------------------------------
def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def _safe_div(n, d):
    ok = d > 0
    return np.where(ok, n / np.where(ok, d, np.float32(1)), np.float32(0))


def _seg_d2(px, py, pz, s, e):
    ee = _dot(e[0], e[1], e[2], e[0], e[1], e[2])
    t = _safe_div(_dot(px - s[0], py - s[1], pz - s[2], e[0], e[1], e[2]), ee)
    t = np.minimum(np.maximum(t, np.float32(0)), np.float32(1))
    dx, dy, dz = px - (s[0] + t * e[0]), py - (s[1] + t * e[1]), pz - (s[2] + t * e[2])
    return (dx * dx + dy * dy) + dz * dz


def _tri_d2(px, py, pz, a, b, c, ab, ac):
    """Ericson 5.1.5 in float32 (list_data.h): [q, 1] points against [1, F] faces -> d2 [q, F]."""
    ap = (px - a[0], py - a[1], pz - a[2])
    bp = (px - b[0], py - b[1], pz - b[2])
    cp = (px - c[0], py - c[1], pz - c[2])
    d1, d2 = _dot(*ab, *ap), _dot(*ac, *ap)
    d3, d4 = _dot(*ab, *bp), _dot(*ac, *bp)
    d5, d6 = _dot(*ab, *cp), _dot(*ac, *cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    s = (va + vb) + vc
    den = _safe_div(np.float32(1), s)
    v, w = vb * den, vc * den
    q = [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]            # interior, then the regions in reverse order

    def put(mask, val):
        for k in range(3):
            q[k] = np.where(mask, val[k], q[k])

    wbc = _safe_div(d4 - d3, (d4 - d3) + (d5 - d6))
    put((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), [b[k] + wbc * (c[k] - b[k]) for k in range(3)])
    wac = _safe_div(d2, d2 - d6)
    put((vb <= 0) & (d2 >= 0) & (d6 <= 0), [a[k] + wac * ac[k] for k in range(3)])
    put((d6 >= 0) & (d5 <= d6), c)
    vab = _safe_div(d1, d1 - d3)
    put((vc <= 0) & (d1 >= 0) & (d3 <= 0), [a[k] + vab * ab[k] for k in range(3)])
    put((d3 >= 0) & (d4 <= d3), b)
    put((d1 <= 0) & (d2 <= 0), a)
    dx, dy, dz = px - q[0], py - q[1], pz - q[2]
    return (dx * dx + dy * dy) + dz * dz


def signed_distance_cpu(verts, faces, points, with_winding=False, chunk=None):
    """signed_distance restated in numpy -> (sdf float32 [Q], face_idx int32 [Q], winding float64 [Q] or None)."""
    v, f = _host(verts, np.float32).reshape(-1, 3), _host(faces, np.int32).reshape(-1, 3)
    pts = _host(points, np.float32).reshape(-1, 3)
    if len(f) == 0:
        raise hip.ListError("signed_distance_cpu", hip.ERR_SHAPE, "0 faces: need 1 <= F")
    ok = E._valid_faces(f, len(v))
    t = v[np.where(ok[:, None], f, 0)] if len(v) else np.zeros((len(f), 3, 3), np.float32)   # [F, corner, axis]
    a, b, c = ([t[None, :, j, k] for k in range(3)] for j in range(3))
    ab, ac = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    bc = [c[k] - b[k] for k in range(3)]
    n = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
    flat = (n[0] == 0) & (n[1] == 0) & (n[2] == 0)
    solid = ok[None, :] & ~flat
    t64 = t.astype(np.float64)
    Q, F = len(pts), len(f)
    chunk = chunk or max(1, (1 << 19) // F)
    sdf = np.empty(Q, np.float32)
    face_idx = np.empty(Q, np.int32)
    wind = np.empty(Q, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(0, Q, chunk):
            p = pts[s:s + chunk]
            px, py, pz = p[:, 0:1], p[:, 1:2], p[:, 2:3]
            d2 = _tri_d2(px, py, pz, a, b, c, ab, ac)
            e = np.minimum(np.minimum(_seg_d2(px, py, pz, a, ab), _seg_d2(px, py, pz, a, ac)),
                           _seg_d2(px, py, pz, b, bc))
            d2 = np.where(flat, e, d2)
            d2 = np.where(ok[None, :] & ~np.isnan(d2), d2, np.float32(np.inf))
            j = np.argmin(d2, axis=1)                                  # the first minimum: the smallest face
            best = d2[np.arange(len(p)), j]
            face_idx[s:s + chunk] = np.where(np.isinf(best), -1, j)
            # the generalised winding number, float64
            r = t64[None, :, :, :] - p.astype(np.float64)[:, None, None, :]   # [q, F, corner, axis]
            ra, rb, rc = r[:, :, 0], r[:, :, 1], r[:, :, 2]
            det = np.einsum("qfk,qfk->qf", ra, np.cross(rb, rc))
            la, lb, lc = (np.sqrt(np.einsum("qfk,qfk->qf", x, x)) for x in (ra, rb, rc))
            den = la * lb * lc + np.einsum("qfk,qfk->qf", ra, rb) * lc + np.einsum("qfk,qfk->qf", rb, rc) * la + \
                np.einsum("qfk,qfk->qf", rc, ra) * lb
            w = np.where(solid, np.arctan2(det, den), 0.0).sum(axis=1) / (2 * math.pi)
            wind[s:s + chunk] = w
            mag = np.sqrt(best)
            sdf[s:s + chunk] = np.where(w > 0.5, -mag, mag)
    return sdf, face_idx, (wind if with_winding else None)


def boundary_samples_cpu(points, sigma, seed=0):
    """boundary_samples restated in numpy (the same float64 recipe, rounded to float32 once)."""
    p = _host(points, np.float32).reshape(-1, 3)
    if sigma == 0:
        return p.copy()
    M = len(p)
    c0 = (np.uint64(_BOUNDARY_BASE) + np.uint64(6) * np.arange(M, dtype=np.uint64)[:, None]
          + np.uint64(2) * np.arange(3, dtype=np.uint64)[None, :])
    u1, u2 = E.uniform_cpu(seed, c0), E.uniform_cpu(seed, c0 + np.uint64(1))
    n = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * math.pi * u2)
    return (p.astype(np.float64) + float(np.float32(sigma)) * n).astype(np.float32)


def farthest_points_cpu(clouds, k):
    """farthest_points restated in numpy -> (points [B,K,3], idx int32 [B,K]), [K,3] / [K] for one [N,3] cloud."""
    c = _host(clouds, np.float32)
    single = c.ndim == 2
    c = c.reshape(1, -1, 3) if single else c.reshape(c.shape[0], -1, 3)
    B, N = c.shape[0], c.shape[1]
    k = int(k)
    if not 1 <= N <= MAX_FPS_POINTS or not 1 <= k <= N:
        raise hip.ListError("farthest_points_cpu", hip.ERR_SHAPE, f"N = {N}, K = {k}: need 1 <= K <= N <= {MAX_FPS_POINTS}")
    idx = np.zeros((B, k), np.int32)
    m = np.full((B, N), np.inf, np.float32)
    rows = np.arange(B)
    with np.errstate(invalid="ignore"):
        for s in range(1, k):
            d = c - c[rows, idx[:, s - 1]][:, None, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            m = np.where(d2 < m, d2, m)
            idx[:, s] = np.argmax(m, axis=1)                           # the first maximum: the smallest index
    pts = c[rows[:, None], idx]
    return (pts[0], idx[0]) if single else (pts, idx)


# ---- files ----------------------------------------------------------------------------------------------------------
def _stand_in(path):
    return os.path.splitext(path)[0] + ".npz"


def exists(path):
    """An .h5 path or its .npz stand-in exists (the datasets' rule)."""
    return os.path.exists(path) or os.path.exists(_stand_in(path))


def save_arrays(path, arrays):
    """Keyed arrays to `path` (.h5, gzip) when h5py imports, else to the .npz stand-in next to it -> the written path."""
    try:
        import h5py
    except ImportError:
        np.savez_compressed(_stand_in(path), **arrays)
        return _stand_in(path)
    with h5py.File(path, "w") as f:
        for key, a in arrays.items():
            f.create_dataset(key, data=a, compression="gzip")
    return path


def _on_device(device):
    if device is None:
        return None
    import torch
    dev = torch.device(device)
    return None if dev.type == "cpu" else dev


def prepare_shape(mesh_path, mesh_out_dir, points_out_dir, num_points=50000, sigmas=SIGMAS, n_farthest=5000, seed=0,
                  device="cuda:0"):
    """One mesh -> mesh_out_dir/isosurf_scaled.obj, points_out_dir/sampled_points.h5 (grid_points [M,3],
    query_points_sigma_{s} [M,4] = xyz + sdf, float32) and points_out_dir/farthest_pointclouds.h5
    (points_{n_farthest} [K,3]), as .npz stand-ins without h5py.  The surface samples use `seed`, the boundary
    samples of sigma i use `seed + i`.  device None or "cpu": the numpy restatement.  Returns the written paths."""
    raw = E.load_mesh(mesh_path)
    mesh = scale_mesh(raw.vertices, raw.faces)
    os.makedirs(mesh_out_dir, exist_ok=True)
    os.makedirs(points_out_dir, exist_ok=True)
    mesh_file = mesh.export(os.path.join(mesh_out_dir, "isosurf_scaled.obj"))
    dev = _on_device(device)
    tables = {}
    if dev is None:
        grid, _ = E.sample_surface_cpu(mesh.vertices, mesh.faces, num_points, seed)
        tables["grid_points"] = grid
        for i, s in enumerate(sigmas):
            q = boundary_samples_cpu(grid, s, seed + i)
            sdf = np.zeros(len(q), np.float32) if s == 0 else signed_distance_cpu(mesh.vertices, mesh.faces, q)[0]
            tables[f"query_points_sigma_{float(s)}"] = np.concatenate([q, sdf[:, None]], axis=1)
        far, _ = farthest_points_cpu(grid, n_farthest)
    else:
        import torch
        v, f = torch.from_numpy(mesh.vertices).to(dev), torch.from_numpy(mesh.faces).to(dev)
        grid, _ = E.sample_surface(v, f, num_points, seed)
        tables["grid_points"] = grid
        for i, s in enumerate(sigmas):
            q = boundary_samples(grid, s, seed + i)
            sdf = torch.zeros(q.shape[0], dtype=torch.float32, device=dev) if s == 0 else signed_distance(v, f, q)[0]
            tables[f"query_points_sigma_{float(s)}"] = torch.cat([q, sdf[:, None]], dim=1)
        far, _ = farthest_points(grid, n_farthest)
        tables = {k: t.cpu().numpy() for k, t in tables.items()}
        far = far.cpu().numpy()
    points_file = save_arrays(os.path.join(points_out_dir, "sampled_points.h5"), tables)
    far_file = save_arrays(os.path.join(points_out_dir, "farthest_pointclouds.h5"), {f"points_{n_farthest}": far})
    return {"mesh": mesh_file, "sampled_points": points_file, "farthest_pointclouds": far_file}


# ---- command line ---------------------------------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description="Make the training files (isosurf_scaled.obj, sampled_points, "
                                             "farthest_pointclouds) from raw meshes")
    ap.add_argument("--input_dir", type=str, default="./Datasets/shapenet/DISN/")
    ap.add_argument("--output_dir", type=str, default="./Datasets/shapenet/")
    ap.add_argument("--num_points", type=int, default=50000)
    ap.add_argument("--sigma", nargs="+", type=float, default=list(SIGMAS))
    ap.add_argument("--categories", nargs="+", required=True)
    ap.add_argument("--file_path_glob", type=str, required=True,
                    help="path of the file from the category -> /<instance>*/*filename.ext")
    ap.add_argument("--n_farthest", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=str, default="cuda:0", help='a HIP device, or "cpu" for the numpy path')
    args = ap.parse_args(argv)
    files = []
    for c in args.categories:
        files.extend(sorted(glob(args.input_dir + c + args.file_path_glob)))
    print(args.categories, len(files), flush=True)
    done = skipped = failed = 0
    for path in files:
        cat_id, shape_id = os.path.normpath(path).split(os.sep)[-3:-1]
        point_dir = os.path.join(args.output_dir, "sampled_points", cat_id, shape_id)
        if exists(os.path.join(point_dir, "sampled_points.h5")) and \
                exists(os.path.join(point_dir, "farthest_pointclouds.h5")):
            print(os.path.join(point_dir, "sampled_points.h5") + " Exists. Skipping", flush=True)
            skipped += 1
            continue
        try:
            prepare_shape(path, os.path.join(args.output_dir, "isosurface", cat_id, shape_id), point_dir,
                          args.num_points, args.sigma, args.n_farthest, args.seed, args.device)
            done += 1
        except Exception:                                  # the reference reports and goes on with the next mesh
            print("Problem with ", path, "\n" + traceback.format_exc(), file=sys.stderr, flush=True)
            failed += 1
    print(f"prepared {done}, skipped {skipped}, failed {failed}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
