"""Marching cubes: the iso-surface of an SDF volume as a mesh of shared vertices and triangles.

`marching_cubes` runs on the volume's device through liblist_hip.so (include/list_mesh.h); `marching_cubes_cpu` is the
same algorithm in numpy, with the same case tables (csrc/mc_tables.h, written by tools/gen_mc_tables.py) -- the CPU
fallback and the test oracle.  Both give, in the same order:

  * a corner is inside iff v > level (NaN is outside): the surface mcubes.marching_cubes(-v, -level) extracts, i.e.
    utils.generate_mesh's convention;
  * one vertex per cut grid edge, owned by the edge's low end; vertices in raster order of their points, and per point
    in axis order; t = (level - v0) / (v1 - v0) clamped to [0, 1], 0.5 where not finite;
  * vertices mapped per axis to bb_min + (idx + t) * (bb_max - bb_min) / (n - 1), axes in array order;
  * triangles in raster order of their cells, right-hand normals toward decreasing v (outward for a field that is
    positive inside).
"""
import ctypes as C
import os
import re

import numpy as np

from . import hip

_TABLES_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_tables.h")
INT32_MAX = 2 ** 31 - 1

MESH_EXPORTS = {
    "list_mc_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "list_mc_count": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_void_p]),
    "list_mc_emit": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_float),
                               C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_int64, C.c_void_p]),
    "list_mesh_last_error": (C.c_char_p, []),
}

_section = hip.Section(MESH_EXPORTS, "list_mesh_last_error")    # include/list_mesh.h on hip.load()'s handle
load, _check = _section.load, _section.check


# ---- tables ---------------------------------------------------------------------------------------------------------
_tables = None


def tables():
    """(edge_mask [256] uint16, tri_count [256] int64, tri_edges [256, 15] int64) parsed from csrc/mc_tables.h."""
    global _tables
    if _tables is None:
        text = open(_TABLES_H).read()

        def body(name):
            m = re.search(name + r"\[[^=]*=\s*\{(.*?)\n\};", text, flags=re.S)
            return [int(x, 0) for x in re.findall(r"-?(?:0x[0-9a-f]+|\d+)", re.sub(r"//[^\n]*", "", m.group(1)))]

        edge_mask = np.array(body("kMcEdgeMask"), dtype=np.uint16)
        count = np.array(body("kMcTriCount"), dtype=np.int64)
        edges = np.array(body("kMcTriEdges"), dtype=np.int64).reshape(256, -1)
        assert edge_mask.shape == (256,) and count.shape == (256,) and edges.shape[0] == 256
        _tables = edge_mask, count, edges
    return _tables


def edge_owner(e):
    """Edge e of a cell -> (offset of its owning point from the cell's low corner, axis)."""
    a, o1, o2 = e >> 2, e & 1, (e >> 1) & 1
    off = [0, 0, 0]
    others = [b for b in range(3) if b != a]
    off[others[0]], off[others[1]] = o1, o2
    return tuple(off), a


def _bounds3(x, name):
    b = np.broadcast_to(np.asarray(x, dtype=np.float32), (3,)).copy()
    if not np.all(np.isfinite(b)):
        raise ValueError(f"{name} must be finite, got {x}")
    return b


def _check_shape(shape):
    if len(shape) != 3 or min(shape) < 2:
        raise hip.ListError("marching_cubes", hip.ERR_SHAPE, f"volume of shape {tuple(shape)}: need [X,Y,Z], each >= 2")
    if 3 * int(np.prod(shape, dtype=np.int64)) > INT32_MAX:
        raise hip.ListError("marching_cubes", hip.ERR_SHAPE, f"volume {tuple(shape)}: 3 * X * Y * Z exceeds INT32_MAX")


# ---- device ---------------------------------------------------------------------------------------------------------
def marching_cubes(volume, level=0.0, bb_min=-0.5, bb_max=0.5):
    """Iso-surface {v = level} of a float32 [X,Y,Z] device tensor -> (verts [V,3] float32, faces [F,3] int32), both on
    the volume's device, computed on its current stream.  The one host synchronisation reads V and F back.
    bb_min / bb_max: scalars or one value per axis."""
    import torch
    hip._f32_cuda(volume, "volume")
    _check_shape(volume.shape)
    bmin, bmax = _bounds3(bb_min, "bb_min"), _bounds3(bb_max, "bb_max")
    lib = load()
    dev = volume.device
    X, Y, Z = (int(s) for s in volume.shape)
    with torch.cuda.device(dev):
        vol = volume.contiguous()
        ws = _section.workspace(dev, lib.list_mc_workspace_bytes(X, Y, Z), "list_mc_workspace_bytes")
        totals = torch.empty((2,), dtype=torch.int64, device=dev)
        stream = hip._stream()
        _check(lib.list_mc_count(vol.data_ptr(), X, Y, Z, float(level), ws.data_ptr(), ws.numel(), totals.data_ptr(),
                                 stream), "list_mc_count")
        V, F = (int(x) for x in totals.tolist())
        if F > INT32_MAX:
            raise hip.ListError("list_mc_count", hip.ERR_SHAPE, f"{F} triangles exceed INT32_MAX")
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        fmin, fmax = (C.c_float * 3)(*bmin.tolist()), (C.c_float * 3)(*bmax.tolist())
        _check(lib.list_mc_emit(vol.data_ptr(), X, Y, Z, float(level), fmin, fmax, ws.data_ptr(), ws.numel(),
                                verts.data_ptr() if V else None, V, faces.data_ptr() if F else None, F, stream),
               "list_mc_emit")
    return verts, faces


# ---- host -----------------------------------------------------------------------------------------------------------
def marching_cubes_cpu(volume, level=0.0, bb_min=-0.5, bb_max=0.5):
    """marching_cubes restated in numpy: the same vertices (to float32 rounding of the same operations) and the same
    faces, in the same order.  volume: array-like [X,Y,Z] (a tensor is copied to the host) -> (verts float32 [V,3],
    faces int32 [F,3])."""
    if hasattr(volume, "detach"):
        volume = volume.detach().cpu().numpy()
    v = np.ascontiguousarray(volume, dtype=np.float32)
    _check_shape(v.shape)
    X, Y, Z = v.shape
    lv = np.float32(level)
    bmin, bmax = _bounds3(bb_min, "bb_min"), _bounds3(bb_max, "bb_max")
    scale = ((bmax.astype(np.float64) - bmin.astype(np.float64)) / (np.array(v.shape) - 1)).astype(np.float32)
    _, tri_count, tri_edges = tables()

    inside = v > lv                                            # NaN compares False: outside
    mask = np.zeros(v.shape, dtype=np.uint8)
    mask[:-1, :, :] |= (inside[:-1] != inside[1:]).astype(np.uint8)
    mask[:, :-1, :] |= (inside[:, :-1] != inside[:, 1:]).astype(np.uint8) << 1
    mask[:, :, :-1] |= (inside[:, :, :-1] != inside[:, :, 1:]).astype(np.uint8) << 2
    flat_mask = mask.ravel()
    nv = (flat_mask & 1) + ((flat_mask >> 1) & 1) + ((flat_mask >> 2) & 1)
    voff = np.zeros(flat_mask.size, dtype=np.int64)
    np.cumsum(nv[:-1], out=voff[1:])
    V = int(voff[-1] + nv[-1])

    # vertices: point p's cut edges, axis by axis, at voff[p] + (number of its cut edges on lower axes)
    verts = np.empty((V, 3), dtype=np.float32)
    grid = [np.arange(n, dtype=np.float32) for n in v.shape]
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            p = np.flatnonzero(flat_mask & (1 << a))
            idx = np.unravel_index(p, v.shape)
            nb = list(idx)
            nb[a] = nb[a] + 1
            v0, v1 = v[idx], v[tuple(nb)]
            t = (lv - v0) / (v1 - v0)
            t = np.where(np.isfinite(t), np.clip(t, np.float32(0), np.float32(1)), np.float32(0.5)).astype(np.float32)
            rank = np.zeros(p.size, dtype=np.int64)
            for b in range(a):
                rank += (flat_mask[p] >> b) & 1
            out = voff[p] + rank
            for c in range(3):
                g = grid[c][idx[c]]
                coord = (g + t) if c == a else g
                verts[out, c] = coord * scale[c] + bmin[c]

    # faces: cells in raster order, each with its case's triangles in table order
    cs = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cs |= inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << c
    cells = np.flatnonzero(tri_count[cs.ravel()])
    ci = np.unravel_index(cells, cs.shape)
    ccase = cs.ravel()[cells]
    n_t = tri_count[ccase]
    F = int(n_t.sum())
    slots = np.arange(tri_edges.shape[1] // 3)
    keep = slots[None, :] < n_t[:, None]                      # [cells, 5]: which triangle slots are used
    edges = tri_edges[ccase].reshape(-1, tri_edges.shape[1] // 3, 3)[keep]     # [F, 3], raster + table order
    cell_of = np.repeat(np.arange(cells.size), n_t)
    base = [ci[d][cell_of] for d in range(3)]
    faces = np.empty((F, 3), dtype=np.int32)
    owners = [edge_owner(e) for e in range(12)]
    off_tab = np.array([o for o, _ in owners], dtype=np.int64)
    axis_tab = np.array([a for _, a in owners], dtype=np.int64)
    for k in range(3):
        e = edges[:, k]
        q = np.ravel_multi_index(tuple(base[d] + off_tab[e, d] for d in range(3)), v.shape)
        below = (np.int64(1) << axis_tab[e]) - 1
        m = flat_mask[q].astype(np.int64) & below
        faces[:, k] = voff[q] + (m & 1) + ((m >> 1) & 1)
    return verts, faces


# ---- mesh -----------------------------------------------------------------------------------------------------------
class Mesh:
    """vertices float32 [V,3] and faces int32 [F,3] (0-based) on the host.  Made from CUDA tensors (as marching_cubes,
    components.keep_components and simplify.simplify return them) it also keeps those, for render() and export()."""

    def __init__(self, vertices, faces):
        self._device = None
        if getattr(vertices, "is_cuda", False) and getattr(faces, "is_cuda", False):
            import torch
            self._device = (vertices.detach().to(torch.float32).reshape(-1, 3).contiguous(),
                            faces.detach().to(torch.int32).reshape(-1, 3).contiguous())
        if hasattr(vertices, "detach"):
            vertices = vertices.detach().cpu().numpy()
        if hasattr(faces, "detach"):
            faces = faces.detach().cpu().numpy()
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)

    def __repr__(self):
        return f"Mesh(vertices={len(self.vertices)}, faces={len(self.faces)})"

    def export(self, path):
        """Write .obj (utils.write_obj's bytes; composed in HIP on the device the mesh was made on, objtext.write_obj,
        else by utils.write_obj itself) or binary little-endian .ply, by the file's extension."""
        ext = os.path.splitext(path)[1].lower()
        if ext == ".obj":
            if self._device is not None:
                from . import objtext
                objtext.write_obj(path, *self._device)
            else:
                from . import utils
                utils.write_obj(path, self.vertices, self.faces)
        elif ext == ".ply":
            head = ("ply\nformat binary_little_endian 1.0\n"
                    f"element vertex {len(self.vertices)}\nproperty float x\nproperty float y\nproperty float z\n"
                    f"element face {len(self.faces)}\nproperty list uchar int vertex_indices\nend_header\n")
            tri = np.empty(len(self.faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
            tri["n"], tri["i"] = 3, self.faces
            with open(path, "wb") as f:
                f.write(head.encode("ascii"))
                f.write(self.vertices.astype("<f4").tobytes())
                f.write(tri.tobytes())
        else:
            raise ValueError(f"{path}: export writes .obj or .ply")
        return path

    def keep_components(self, keep="all", min_faces=0, return_info=False):
        """A new Mesh of the components components.select_components keeps (the `keep` with the most faces, of those
        with at least `min_faces`), vertices and faces in their order, on the host (components.keep_components_cpu);
        with return_info also its info dict."""
        from . import components
        v, f, info = components.keep_components_cpu(self.vertices, self.faces, keep, min_faces)
        m = Mesh(v, f)
        return (m, info) if return_info else m

    def simplify(self, cells, bb_min=-0.5, bb_max=0.5, return_info=False):
        """A new Mesh with the vertices of every cell of the `cells` grid over [bb_min, bb_max] merged into one
        (simplify.py's rule), on the host (simplify.simplify_cpu); with return_info also its info dict."""
        from . import simplify as S
        v, f, info = S.simplify_cpu(self.vertices, self.faces, cells, bb_min, bb_max)
        m = Mesh(v, f)
        return (m, info) if return_info else m

    def render(self, camera, H, W, mode="lambert", background=None, alpha=1.0):
        """A picture of the mesh from `camera` (render.Camera) -> uint8 [H,W,3] on the host: render.rasterize + shade, in
        HIP on the device the mesh was made on, else in numpy.  mode: "lambert" (head-light grey) or "normal"; background:
        uint8 [H,W,3] (array or tensor; white when None); alpha: the mesh's opacity over it."""
        from . import render as R
        if self._device is not None:
            v, f = self._device
            if background is not None:
                import torch
                background = torch.as_tensor(np.asarray(background.detach().cpu() if hasattr(background, "detach")
                                                        else background, dtype=np.uint8)).contiguous().to(v.device)
            return R.render(v, f, camera, H, W, mode, background, alpha).cpu().numpy()
        return R.render(self.vertices, self.faces, camera, H, W, mode, background, alpha)

    def to_trimesh(self):
        import trimesh
        return trimesh.Trimesh(self.vertices, self.faces, process=False)
