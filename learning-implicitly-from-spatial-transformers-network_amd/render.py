"""Pictures of a mesh: an exact z-buffer rasteriser for the meshes mesh.marching_cubes / components.keep_components
leave on the device, from the model's own camera (the spatial transformer's 4x3 trans_mat) or an orthographic one.

`rasterize` and `shade` run on the tensors' device through liblist_hip.so (include/list_render.h) when they are given
CUDA tensors; `rasterize_cpu` / `shade_cpu` are the same rules in numpy -- the CPU fallback and the test oracle.  Both
give, exactly (csrc/render_math.h holds the same rules as code):

  * a vertex v (the coordinates marching_cubes returns, axes in array order) becomes p = 2 * (v[2], v[1], v[0]), the
    query permutation and scale of models.py:91-92, and X, Y, Z = [p, 1] T by the fma chain, in k order, of the query
    path's projection (csrc/point_math.h: project);
  * LIST camera: den = Z + 1e-8f, u = X / den, v = Y / den on the map_size plane WITHOUT the reference's clamp, pixel
    x = u * (W-1)/(map_size-1), y = v * (H-1)/(map_size-1) in float64 from the float32 X, Y, den; 1 / den decides
    visibility (larger is nearer).  Orthographic camera: x = X, y = Y, the smaller Z is nearer;
  * pixel (x, y) is column x of row y and its centre has the coordinates (x, y); coordinates snap to 1/16 pixel,
    floor(x * 16 + 0.5) in float64;
  * a face is dropped whole, and counted, for the first of: a vertex index outside [0, V); a non-finite X, Y or Z
    (den); LIST camera and a den <= z_near (no clipping); a snapped coordinate beyond +-2^24 sub-pixels; zero area after
    snapping;
  * coverage is decided by int64 edge functions with the top-left fill rule after the face was given positive
    orientation: both windings are drawn and two faces that share an edge cover each centre on it exactly once;
  * the depth at a centre is ((e0 * d0 + e1 * d1) + e2 * d2) / area in float64 (e: the edge values, d: the vertices'
    1 / den or Z), rounded to float32;
  * the winner of a pixel is the nearest fragment and, among equal float32 depths, the lowest face index: the smallest
    of the 64-bit keys (monotone depth bits above the face index);
  * face_id is -1 and depth +inf on background; depth is den (LIST camera, 1 / the winning 1 / den) or Z;
  * stats counts every face once: bad_index, non_finite, behind_near, guard_band, zero_area, offscreen (no centre of
    the image in its bounding box), small / large (rasterised; a clamped bounding box of at most CAP x CAP centres is
    small -- the device's two paths);
  * shading: the face normal n = (b - a) x (c - a) in float32, mesh axis order.  "normal": rgb = round((n / |n| * 0.5 +
    0.5) * 255).  "lambert": head-light grey round(|n . d| / (|n| |d|) * 255) with d = eye.xyz - eye.w * a towards the
    camera's centre.  Over a background (white without one): (a * shade + (256 - a) * background + 128) >> 8 with
    a = round(alpha * 256) on the mesh's pixels, the background elsewhere.
"""
import ctypes as C

import numpy as np

from . import hip

INT32_MAX = 2 ** 31 - 1
ORTHO, LIST = 0, 1                                   # LIST_RENDER_ORTHO, LIST_RENDER_LIST
CAP = 8                                              # LIST_RENDER_CAP
LARGE_GROUPS = 256                                   # LIST_RENDER_LARGE_GROUPS
MAX_SIDE, MAX_PIXELS = 16384, 1 << 26                # LIST_RENDER_MAX_SIDE, LIST_RENDER_MAX_PIXELS
N_STEPS = 4                                          # LIST_RENDER_N_STEPS: clear, setup + small, large, resolve
STEP_NAMES = ("k_render_clear", "k_render_setup_small", "k_render_large", "k_render_resolve")
STATS = ("bad_index", "non_finite", "behind_near", "guard_band", "zero_area", "offscreen", "small", "large")
SHADES = {"normal": 0, "lambert": 1}
SUBPIXEL = 16
GUARD = float(2 ** 24)
F32, F64 = np.float32, np.float64
BACKGROUND_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


class ListRenderCamera(C.Structure):
    _fields_ = [("T", C.c_float * 12), ("eye", C.c_float * 4), ("mode", C.c_int32), ("map_size", C.c_int32)]


RENDER_EXPORTS = {
    "list_render_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "list_render_rasterize": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(ListRenderCamera),
                                        C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "list_render_shade": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.POINTER(ListRenderCamera), C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    "list_render_last_error": (C.c_char_p, []),
}

_section = hip.Section(RENDER_EXPORTS, "list_render_last_error")      # include/list_render.h on hip.load()'s handle
load, _check = _section.load, _section.check


def _refuse(msg, code=hip.ERR_ARG):
    return hip.ListError("render", code, msg)


# ---- camera ---------------------------------------------------------------------------------------------------------
class Camera:
    """A 4x3 float32 matrix T (row-major as trans_mat[b]), the mode (LIST or ORTHO), the LIST camera's map_size and the
    camera's centre `eye` in homogeneous mesh coordinates (eye[3] = 0: a direction), which only the head-light uses."""

    def __init__(self, T, mode, map_size=137, eye=None):
        if hasattr(T, "detach"):
            T = T.detach().cpu().numpy()
        T = np.asarray(T, dtype=F32)
        if T.size != 12:
            raise ValueError(f"a camera matrix of shape {T.shape}: need [4,3] (one image's trans_mat)")
        self.T = np.ascontiguousarray(T.reshape(4, 3))
        self.mode, self.map_size = int(mode), int(map_size)
        if self.mode not in (ORTHO, LIST):
            raise ValueError(f"camera mode {mode!r}: ORTHO (0) or LIST (1)")
        if self.mode == LIST and self.map_size < 2:
            raise ValueError(f"map_size {map_size}: the LIST camera needs a plane of at least 2 x 2")
        self.eye = np.asarray(self.centre(self.T) if eye is None else eye, dtype=F32).reshape(4)

    @staticmethod
    def centre(T):
        """The point every ray of [p, 1] T passes through, in homogeneous MESH coordinates, scaled to max |.| = 1: the
        left null vector of T by cofactors in float64, taken from p = 2 * (v[2], v[1], v[0]) back to v.  Zeros when T
        has rank < 3."""
        T = np.asarray(T, dtype=F64).reshape(4, 3)
        c = np.array([(-1.0) ** i * np.linalg.det(np.delete(T, i, axis=0)) for i in range(4)])
        e = np.array([c[2], c[1], c[0], 2.0 * c[3]])
        top = np.abs(e).max()
        return (e / top if top > 0 and np.isfinite(top) else np.zeros(4)).astype(F32)

    @classmethod
    def from_transmat(cls, trans_mat, map_size=137):
        """The model's own camera: trans_mat [4,3] (or [1,4,3]) as LIST.encode returns it or the batch carries it."""
        return cls(trans_mat, LIST, map_size)

    @classmethod
    def orthographic(cls, axis, H, W, bb_min=-0.5, bb_max=0.5):
        """Looks along array axis `axis` (0, 1 or 2; the smaller coordinate is nearer).  Of the other two axes the first
        runs down the rows and the second along the columns, bb_min at pixel 0 and bb_max at pixel size - 1."""
        if axis not in (0, 1, 2):
            raise ValueError(f"axis {axis!r}: 0, 1 or 2")
        if not bb_max > bb_min:
            raise ValueError(f"bb_min {bb_min}, bb_max {bb_max}")
        rows, cols = [a for a in (0, 1, 2) if a != axis]
        sx, sy = (W - 1) / (bb_max - bb_min), (H - 1) / (bb_max - bb_min)
        T = np.zeros((4, 3), dtype=F64)
        T[2 - cols, 0], T[3, 0] = sx / 2.0, -bb_min * sx          # p[k] = 2 * v[2 - k]
        T[2 - rows, 1], T[3, 1] = sy / 2.0, -bb_min * sy
        T[2 - axis, 2] = 0.5
        eye = np.zeros(4, dtype=F32)
        eye[axis] = 1.0
        return cls(T.astype(F32), ORTHO, 0, eye)

    def struct(self):
        s = ListRenderCamera()
        s.T[:] = self.T.ravel().tolist()
        s.eye[:] = self.eye.tolist()
        s.mode, s.map_size = self.mode, self.map_size
        return s


def _chain(T, v):
    """X, Y, Z float32 [N] of the vertices v float32 [N,3]: project()'s fma chain (a float32 product is exact in
    float64, so one float64 add and a rounding is the fma)."""
    p = (v[:, 2] * F32(2), v[:, 1] * F32(2), v[:, 0] * F32(2))
    out = []
    for j in range(3):
        x = (p[0] * T[0, j]).astype(F32)
        x = (p[1].astype(F64) * F64(T[1, j]) + x.astype(F64)).astype(F32)
        x = (p[2].astype(F64) * F64(T[2, j]) + x.astype(F64)).astype(F32)
        out.append((x + T[3, j]).astype(F32))
    return out


def project_uv(verts, camera):
    """The LIST camera's unsnapped float32 (u, v) [N,2] on the map_size plane: the query path's projection (csrc/
    point_math.h: project, oracle.list_oracle.project_points) without its clamp to [0, map_size - 1]."""
    v = _verts_host(verts)
    with np.errstate(all="ignore"):
        X, Y, Z = _chain(camera.T, v)
        den = (Z + F32(1e-8)).astype(F32)
        return np.stack([(X / den).astype(F32), (Y / den).astype(F32)], axis=1)


# ---- device ---------------------------------------------------------------------------------------------------------
def _is_cuda(x):
    return hasattr(x, "is_cuda") and x.is_cuda


def _check_image(H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and H * W <= MAX_PIXELS):
        raise _refuse(f"image of {H} x {W}: each side must be in [1, {MAX_SIDE}] and H * W <= {MAX_PIXELS}", hip.ERR_SHAPE)
    return H, W


def _mesh_cuda(verts, faces):
    import torch
    for t, name, dtype, what in ((verts, "verts", torch.float32, "float32 [V,3]"), (faces, "faces", torch.int32, "int32 [F,3]")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            raise _refuse(f"{name} must be a {what} CUDA/HIP tensor (got {type(t).__name__} "
                          f"{getattr(t, 'dtype', None)} {getattr(t, 'device', None)})")
        if t.dim() != 2 or t.shape[1] != 3:
            raise _refuse(f"{name} of shape {tuple(t.shape)}: need {what}", hip.ERR_SHAPE)
        if not t.is_contiguous():
            raise _refuse(f"{name} must be contiguous (strides {tuple(t.stride())})")
    if verts.device != faces.device:
        raise _refuse(f"verts on {verts.device}, faces on {faces.device}")
    return int(verts.shape[0]), int(faces.shape[0])


def _z_near(z_near):
    z = float(z_near)
    if not (0.0 <= z < float("inf")):
        raise _refuse(f"z_near = {z_near!r}: must be finite and >= 0")
    return z


def rasterize_device(verts, faces, camera, H, W, z_near=1e-6, steps=(0, N_STEPS)):
    """rasterize on the device without the read-back of the stats -> (face_id int32 [H,W], depth float32 [H,W],
    stats int32 [8] in the order of STATS), all on the mesh's device.  steps: the launches to run (timing tools)."""
    import torch
    V, F = _mesh_cuda(verts, faces)
    z = _z_near(z_near)
    lib = load()
    dev = verts.device
    H, W = int(H), int(W)
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_render_workspace_bytes(F, H, W), "list_render_workspace_bytes")
        face_id = torch.empty((H, W), dtype=torch.int32, device=dev)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        stats = torch.empty((len(STATS),), dtype=torch.int32, device=dev)
        cam = camera.struct()
        _check(lib.list_render_rasterize(verts.data_ptr() if V else None, V, faces.data_ptr() if F else None, F,
                                         C.byref(cam), H, W, z, ws.data_ptr(), ws.numel(), face_id.data_ptr(),
                                         depth.data_ptr(), stats.data_ptr(), int(steps[0]), int(steps[1]), hip._stream()),
               "list_render_rasterize")
    return face_id, depth, stats


def rasterize(verts, faces, camera, H, W, z_near=1e-6):
    """The nearest face and its depth at every pixel centre of an H x W image -> (face_id int32 [H,W], -1 on
    background; depth float32 [H,W], +inf on background; stats: a dict of the counters in STATS).

    CUDA tensors (verts float32 [V,3], faces int32 [F,3], contiguous, one device) take the HIP path on their device
    and current stream and get tensors on that device; another dtype, a non-contiguous tensor or an image beyond
    MAX_SIDE / MAX_PIXELS is refused (hip.ListError).  The stats are read back: the one synchronisation.  CPU tensors
    and array-likes go to rasterize_cpu and get numpy arrays."""
    if not (_is_cuda(verts) or _is_cuda(faces)):
        return rasterize_cpu(verts, faces, camera, H, W, z_near)
    face_id, depth, stats = rasterize_device(verts, faces, camera, H, W, z_near)
    return face_id, depth, dict(zip(STATS, stats.tolist()))


def _alpha256(alpha):
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise _refuse(f"alpha = {alpha!r}: must be in [0, 1]")
    return int(np.floor(a * 256.0 + 0.5))


def _shade_mode(mode):
    if mode not in SHADES:
        raise _refuse(f"mode {mode!r}: 'normal' or 'lambert'")
    return SHADES[mode]


def shade(verts, faces, face_id, camera, mode="lambert", background=None, alpha=1.0):
    """The picture of a rasterised mesh -> uint8 [H,W,3].  mode "normal": the faces' unit normals as colours; "lambert":
    head-light grey.  background: uint8 [H,W,3] (white when None); alpha: the mesh's opacity over it, in 1/256 steps.
    CUDA tensors take the HIP path (face_id int32 [H,W] and the background contiguous on the mesh's device, else
    hip.ListError); anything else goes to shade_cpu."""
    if not (_is_cuda(verts) or _is_cuda(faces) or _is_cuda(face_id)):
        return shade_cpu(verts, faces, face_id, camera, mode, background, alpha)
    import torch
    V, F = _mesh_cuda(verts, faces)
    dev = verts.device
    if not isinstance(face_id, torch.Tensor) or face_id.dtype != torch.int32 or face_id.device != dev or \
            face_id.dim() != 2 or not face_id.is_contiguous():
        raise _refuse(f"face_id must be a contiguous int32 [H,W] tensor on {dev}")
    H, W = _check_image(*face_id.shape)
    if background is not None and (not isinstance(background, torch.Tensor) or background.dtype != torch.uint8 or
                                   background.device != dev or tuple(background.shape) != (H, W, 3) or
                                   not background.is_contiguous()):
        raise _refuse(f"background must be a contiguous uint8 [{H},{W},3] tensor on {dev}")
    sm, a = _shade_mode(mode), _alpha256(alpha)
    lib = load()
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    cam = camera.struct()
    with torch.cuda.device(dev):
        _check(lib.list_render_shade(verts.data_ptr() if V else None, V, faces.data_ptr() if F else None, F,
                                     face_id.data_ptr(), C.byref(cam), H, W, sm,
                                     background.data_ptr() if background is not None else None, a, rgb.data_ptr(),
                                     hip._stream()), "list_render_shade")
    return rgb


def render(verts, faces, camera, H, W, mode="lambert", background=None, alpha=1.0, z_near=1e-6):
    """rasterize + shade -> uint8 [H,W,3], on the device for CUDA tensors (no read-back), else in numpy."""
    if _is_cuda(verts) or _is_cuda(faces):
        face_id = rasterize_device(verts, faces, camera, H, W, z_near)[0]
    else:
        face_id = rasterize_cpu(verts, faces, camera, H, W, z_near)[0]
    return shade(verts, faces, face_id, camera, mode, background, alpha)


def save_png(path, rgb):
    """Write a uint8 [H,W,3] picture (a tensor is copied to the host) as PNG."""
    from PIL import Image
    if hasattr(rgb, "detach"):
        rgb = rgb.detach().cpu().numpy()
    Image.fromarray(np.ascontiguousarray(rgb, dtype=np.uint8), "RGB").save(path, format="PNG")
    return path


# ---- host -----------------------------------------------------------------------------------------------------------
def _verts_host(verts):
    if hasattr(verts, "detach"):
        verts = verts.detach().cpu().numpy()
    v = np.asarray(verts, dtype=F32)
    return np.ascontiguousarray(v.reshape(-1, 3))


def _faces_host(faces):
    if hasattr(faces, "detach"):
        faces = faces.detach().cpu().numpy()
    f = np.asarray(faces)
    if f.size == 0:
        return np.zeros((0, 3), dtype=np.int64)
    if f.dtype.kind not in "iu":
        raise TypeError(f"faces must hold integers (got {f.dtype})")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces of shape {f.shape}: need [F,3]")
    return f.astype(np.int64)


def _project_host(v, camera, H, W, z_near):
    """Per vertex: snapped sx, sy int64 (0 when flagged), depth value d float64, and the flags non_finite / behind_near /
    guard_band (bool [N] each)."""
    with np.errstate(all="ignore"):
        X, Y, Z = _chain(camera.T, v)
        if camera.mode == LIST:
            den = (Z + F32(1e-8)).astype(F32)
            non_finite = ~(np.isfinite(X) & np.isfinite(Y) & np.isfinite(den))
            near = ~non_finite & (den <= F32(z_near))
            dd = den.astype(F64)
            xs = (X.astype(F64) / dd) * (F64(W - 1) / F64(camera.map_size - 1))
            ys = (Y.astype(F64) / dd) * (F64(H - 1) / F64(camera.map_size - 1))
            d = 1.0 / dd
        else:
            non_finite = ~(np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z))
            near = np.zeros(len(v), dtype=bool)
            xs, ys, d = X.astype(F64), Y.astype(F64), Z.astype(F64)
        fx, fy = np.floor(xs * 16.0 + 0.5), np.floor(ys * 16.0 + 0.5)
        ok = ~non_finite & ~near
        guard = ok & ~((np.abs(fx) <= GUARD) & (np.abs(fy) <= GUARD))
        ok &= ~guard
        sx = np.where(ok, fx, 0.0).astype(np.int64)
        sy = np.where(ok, fy, 0.0).astype(np.int64)
    return sx, sy, np.where(ok, d, 0.0), non_finite, near, guard


def _keys(q, face, mode):
    b = np.ascontiguousarray(q, dtype=F32).view(np.uint32)
    m = np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000))
    if mode == LIST:
        m = ~m
    return (m.astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64)


def _rasterize_host(v, f, camera, H, W, z_near):
    """-> (keys uint64 [H*W], outcome int64 [F]: each face's index into STATS)."""
    V, F = len(v), len(f)
    if V > INT32_MAX or F > INT32_MAX:
        raise _refuse(f"V = {V}, F = {F}: both must be in [0, INT32_MAX]", hip.ERR_SHAPE)
    keys = np.full(H * W, BACKGROUND_KEY, dtype=np.uint64)
    outcome = np.zeros(F, dtype=np.int64)                      # 0 = bad_index until shown otherwise
    valid = ((f >= 0) & (f < V)).all(axis=1)
    idx = np.flatnonzero(valid)
    if idx.size:
        sx, sy, d, non_finite, near, guard = _project_host(v, camera, H, W, z_near)
        g = f[idx]
        reason = np.full(idx.size, -1, dtype=np.int64)
        for code, flag in ((3, guard), (2, near), (1, non_finite)):         # the first in the rules' order wins
            reason[flag[g].any(axis=1)] = code
        x, y, dv = sx[g], sy[g], d[g]                              # [n,3]
        area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        reason[(reason < 0) & (area == 0)] = 4
        flip = area < 0                                            # positive orientation: swap the last two vertices
        for a in (x, y, dv):
            a[flip, 1], a[flip, 2] = a[flip, 2].copy(), a[flip, 1].copy()
        area = np.abs(area)
        cx0, cx1 = (x.min(axis=1) + (SUBPIXEL - 1)) >> 4, x.max(axis=1) >> 4
        cy0, cy1 = (y.min(axis=1) + (SUBPIXEL - 1)) >> 4, y.max(axis=1) >> 4
        ix0, ix1 = np.maximum(cx0, 0), np.minimum(cx1, W - 1)
        iy0, iy1 = np.maximum(cy0, 0), np.minimum(cy1, H - 1)
        bw, bh = ix1 - ix0 + 1, iy1 - iy0 + 1
        empty = (bw < 1) | (bh < 1)
        reason[(reason < 0) & empty] = 5
        drawn = reason < 0
        reason[drawn & (bw <= CAP) & (bh <= CAP)] = 6
        reason[reason < 0] = 7
        outcome[idx] = reason
        sel = np.flatnonzero(drawn)
        if sel.size:
            size = bw[sel] * (MAX_SIDE + 1) + bh[sel]
            for s in np.unique(size):
                group = sel[size == s]
                w_, h_ = int(s // (MAX_SIDE + 1)), int(s % (MAX_SIDE + 1))
                per = max(1, (1 << 21) // (w_ * h_))
                for lo in range(0, group.size, per):
                    _raster_group(group[lo:lo + per], w_, h_, x, y, dv, area, ix0, iy0, idx, camera.mode, W, keys)
    return keys, outcome


def face_outcomes_cpu(verts, faces, camera, H, W, z_near=1e-6):
    """What becomes of each face -> int64 [F] of indices into STATS (6 / 7: rasterised as a small / large face)."""
    H, W = _check_image(H, W)
    return _rasterize_host(_verts_host(verts), _faces_host(faces), camera, H, W, _z_near(z_near))[1]


def rasterize_cpu(verts, faces, camera, H, W, z_near=1e-6):
    """rasterize restated in numpy (module docstring) -> (face_id int32 [H,W], depth float32 [H,W], stats dict), on the
    host.  Vectorised over the faces of one bounding-box size at a time; the winner is np.minimum.at on the keys."""
    H, W = _check_image(H, W)
    keys, outcome = _rasterize_host(_verts_host(verts), _faces_host(faces), camera, H, W, _z_near(z_near))
    stats = dict(zip(STATS, np.bincount(outcome, minlength=len(STATS)).tolist()))
    keys = keys.reshape(H, W)
    bg = keys == BACKGROUND_KEY
    face_id = np.where(bg, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    m = (keys >> np.uint64(32)).astype(np.uint32)
    if camera.mode == LIST:
        m = ~m
    q = np.where(m & np.uint32(0x80000000), m & np.uint32(0x7FFFFFFF), ~m).astype(np.uint32).view(F32)
    with np.errstate(all="ignore"):
        depth = (1.0 / q.astype(F64)).astype(F32) if camera.mode == LIST else q.copy()
    depth[bg] = np.inf
    return face_id, depth, stats


def _raster_group(k, bw, bh, x, y, dv, area, ix0, iy0, idx, mode, W, keys):
    """The faces k (rows of the per-face arrays), all with a clamped bounding box of bw x bh centres."""
    ix = ix0[k][:, None, None] + np.arange(bw, dtype=np.int64)[None, None, :]
    iy = iy0[k][:, None, None] + np.arange(bh, dtype=np.int64)[None, :, None]
    px, py = ix * SUBPIXEL, iy * SUBPIXEL
    cover = np.ones((k.size, bh, bw), dtype=bool)
    e = []
    for a, b in ((1, 2), (2, 0), (0, 1)):                        # the weight of vertex 0, 1, 2
        xa, ya = x[k, a][:, None, None], y[k, a][:, None, None]
        dx, dy = (x[k, b] - x[k, a])[:, None, None], (y[k, b] - y[k, a])[:, None, None]
        ev = dx * (py - ya) - dy * (px - xa)
        top_left = (dy < 0) | ((dy == 0) & (dx > 0))
        cover &= (ev > 0) | ((ev == 0) & top_left)
        e.append(ev)
    d0, d1, d2 = (dv[k, j][:, None, None] for j in range(3))
    s = (e[0].astype(F64) * d0 + e[1].astype(F64) * d1) + e[2].astype(F64) * d2
    with np.errstate(all="ignore"):
        q = (s / area[k][:, None, None].astype(F64)).astype(F32)
    face = np.broadcast_to(idx[k][:, None, None], cover.shape)
    pix = np.broadcast_to(iy * W + ix, cover.shape)
    np.minimum.at(keys, pix[cover], _keys(q[cover], face[cover], mode))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def shade_cpu(verts, faces, face_id, camera, mode="lambert", background=None, alpha=1.0):
    """shade restated in numpy -> uint8 [H,W,3] on the host."""
    v, f = _verts_host(verts), _faces_host(faces)
    if hasattr(face_id, "detach"):
        face_id = face_id.detach().cpu().numpy()
    fid = np.asarray(face_id)
    if fid.ndim != 2 or fid.dtype.kind not in "iu":
        raise ValueError(f"face_id must be an integer [H,W] array (got {fid.dtype} {fid.shape})")
    H, W = _check_image(*fid.shape)
    sm, a256 = _shade_mode(mode), _alpha256(alpha)
    if background is None:
        bg = np.full((H, W, 3), 255, dtype=np.int64)
    else:
        if hasattr(background, "detach"):
            background = background.detach().cpu().numpy()
        bg = np.asarray(background)
        if bg.dtype != np.uint8 or bg.shape != (H, W, 3):
            raise ValueError(f"background must be uint8 [{H},{W},3] (got {bg.dtype} {bg.shape})")
        bg = bg.astype(np.int64)
    out = bg.copy()
    fid = fid.astype(np.int64)
    on = (fid >= 0) & (fid < len(f))
    if on.any():
        tri = f[fid[on]]
        ok = ((tri >= 0) & (tri < len(v))).all(axis=1)
        rows = np.flatnonzero(on.ravel())[ok]
        tri = tri[ok]
        a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
        with np.errstate(all="ignore"):
            u, w = b - a, c - a
            n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                          u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1).astype(F32)
            if sm == 0:
                length = np.sqrt(_dot(n, n)).astype(F32)
                good = (length > 0) & np.isfinite(length)
                t = (n / length[:, None]).astype(F32)
                val = np.floor((t * F32(0.5) + F32(0.5)) * F32(255) + F32(0.5))
                fg = np.where(good[:, None], np.clip(np.where(np.isnan(val), 0, val), 0, 255), 128).astype(np.int64)
            else:
                eye = camera.eye.astype(F32)
                d = (eye[None, :3] - eye[3] * a).astype(F32)
                length = (np.sqrt(_dot(n, n)).astype(F32) * np.sqrt(_dot(d, d)).astype(F32)).astype(F32)
                good = (length > 0) & np.isfinite(length)
                cosine = (np.abs(_dot(n, d)).astype(F32) / length).astype(F32)
                good &= ~np.isnan(cosine)
                val = np.floor(np.minimum(cosine, F32(1)) * F32(255) + F32(0.5))
                grey = np.where(good, np.clip(np.where(np.isnan(val), 0, val), 0, 255), 0).astype(np.int64)
                fg = np.repeat(grey[:, None], 3, axis=1)
        flat = out.reshape(-1, 3)
        flat[rows] = (a256 * fg + (256 - a256) * flat[rows] + 128) >> 8
    return out.astype(np.uint8)
