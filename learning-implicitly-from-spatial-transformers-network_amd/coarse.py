"""The coarse stage in HIP: everything between the image encoders and the occupancy encoder, through liblist_hip.so
(include/list_coarse.h).  From the image code feat_g [B,F0] to the coarse cloud (network.modules.TreeGraphDecoder), its
512-wide code (PointMLP and the max over the points), the camera (LIST.spatial_transformer) and the occupancy grid
(LIST.create_occ).  Inference forward only; `forward` refuses training mode and gradients instead of falling back.

The decoder's W_branch parameters (268 MB for the default network) are read where they lie; everything else is small
and packed once: W_loop's two Linears, which have no nonlinearity between them, are composed into one [out,in] matrix
in float64 and rounded once; eval-mode BN becomes an fp32 scale and shift.

  pack(model)                      -> Packed, cached on the module (LIST, CoarseNet or a bare TreeGraphDecoder)
  decode(packed, feat_g, ...)      -> (pc, coarse, trans_mat, occ): the whole stage
  decode_steps(...)                   a sub-range of its launches, in step_names() order
  time_steps(...)                     milliseconds per launch
  forward(model, feat_g, ...)         pack + decode after the eval-mode / no-gradient checks (what the models call)
  decode_cpu(params, feat_g, ...)     the numpy restatement: the test oracle, not a path of the model

One difference from the torch modules: a point with a non-finite coordinate marks no voxel (create_occ casts it to an
integer, which is undefined)."""
import ctypes as C

import numpy as np

from . import hip, stage

MAX_LAYERS, MAX_R, CODE, GROUP, TILE = 8, 256, 512, 16, 64
MLP_WIDTHS = (3, 64, 256, 512)
SLOPE = 0.2

_FP = C.c_void_p


class _Shape(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("n_degrees", C.c_int32), ("features", C.c_int32 * (MAX_LAYERS + 1)),
                ("degrees", C.c_int32 * MAX_LAYERS), ("activation", C.c_int32 * MAX_LAYERS),
                ("has_mlp", C.c_int32), ("has_camera", C.c_int32), ("g2", C.c_int32), ("hidden", C.c_int32)]


class _Params(C.Structure):
    _fields_ = [("w_root", (_FP * MAX_LAYERS) * MAX_LAYERS), ("wc", _FP * MAX_LAYERS), ("bias", _FP * MAX_LAYERS),
                ("mlp_w", _FP * 3), ("mlp_b", _FP * 3), ("mlp_s", _FP * 3), ("mlp_t", _FP * 3),
                ("cam_w", _FP * 3), ("cam_b", _FP * 3), ("cam_s", _FP * 2), ("cam_t", _FP * 2)]


class _IO(C.Structure):
    _fields_ = [("B", C.c_int32), ("R", C.c_int32), ("bb_min", C.c_float), ("bb_extent", C.c_float),
                ("feat_g", _FP), ("feat_g2", _FP), ("w_branch", _FP * MAX_LAYERS),
                ("packed", _FP), ("packed_bytes", C.c_size_t), ("workspace", _FP), ("workspace_bytes", C.c_size_t),
                ("pc", _FP), ("coarse", _FP), ("trans_mat", _FP), ("occ", _FP)]


_SP, _IOP = C.POINTER(_Shape), C.POINTER(_IO)
COARSE_EXPORTS = {
    "list_coarse_weight_bytes": (C.c_size_t, [_SP]),
    "list_coarse_prep_weights": (C.c_int, [_SP, C.POINTER(_Params), C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_coarse_workspace_bytes": (C.c_size_t, [_SP, C.c_int32]),
    "list_coarse_forward": (C.c_int, [_SP, _IOP, C.c_void_p]),
    "list_coarse_n_steps": (C.c_int32, [_SP]),
    "list_coarse_forward_steps": (C.c_int, [_SP, _IOP, C.c_int32, C.c_int32, C.c_void_p]),
    "list_coarse_last_error": (C.c_char_p, []),
}

_section = hip.Section(COARSE_EXPORTS, "list_coarse_last_error")    # include/list_coarse.h on hip.load()'s handle
load, _check, last_error = _section.load, _section.check, _section.last_error


def shape_of(features, degrees, activation=None, has_mlp=True, has_camera=True, g2=128, hidden=128):
    """The ListCoarseShape of a network.  Lists too long for the struct are refused here, as the library would."""
    features, degrees = [int(f) for f in features], [int(d) for d in degrees]
    if len(degrees) > MAX_LAYERS or len(features) > MAX_LAYERS + 1:
        raise hip.ListError("coarse.shape_of", hip.ERR_SHAPE,
                            f"{len(features)} features, {len(degrees)} degrees: at most {MAX_LAYERS} layers")
    if activation is None:
        activation = [1] * (len(degrees) - 1) + [0]
    s = _Shape()
    s.n_features, s.n_degrees = len(features), len(degrees)
    for i, f in enumerate(features):
        s.features[i] = f
    for i, d in enumerate(degrees):
        s.degrees[i] = d
        s.activation[i] = int(bool(activation[i])) if i < len(activation) else 0
    s.has_mlp, s.has_camera, s.g2, s.hidden = int(has_mlp), int(has_camera), int(g2), int(hidden)
    return s


def _lists(shape):
    L = shape.n_degrees
    return [shape.features[i] for i in range(L + 1)], [shape.degrees[i] for i in range(L)]


# ---- closed forms of the two buffer sizes (the C side is the authority; the tests compare) ---------------------------
_align = stage.align256


def _nodes(degrees, l):
    return int(np.prod(degrees[:l], dtype=np.int64)) if l else 1


def weight_bytes_closed_form(shape):
    """fp32 arrays, each on a 256-byte boundary: per tree layer its W_root matrices, Wc and (with activation) the
    bias; the point MLP's and the camera's weights, biases, scales and shifts.  No W_branch."""
    f, d = _lists(shape)
    o = 0
    for l in range(len(d)):
        o += sum(_align(4 * f[i] * f[l + 1]) for i in range(l + 1)) + _align(4 * f[l] * f[l + 1])
        if shape.activation[l]:
            o += _align(4 * d[l] * f[l + 1])
    if shape.has_mlp:
        for k in range(3):
            o += _align(4 * MLP_WIDTHS[k] * MLP_WIDTHS[k + 1]) + 3 * _align(4 * MLP_WIDTHS[k + 1])
    if shape.has_camera:
        for k, (i, n) in enumerate(((CODE + shape.g2, shape.hidden), (shape.hidden, shape.hidden), (shape.hidden, 12))):
            o += _align(4 * i * n) + _align(4 * n) * (3 if k < 2 else 1)
    return o


def workspace_bytes_closed_form(shape, B):
    """The tree's inner levels [B,nodes,features] and the point MLP's per-tile maxima [B,tiles,512], fp32."""
    f, d = _lists(shape)
    o = sum(_align(4 * B * _nodes(d, l) * f[l]) for l in range(1, len(d)))
    if shape.has_mlp:
        o += _align(4 * B * ((_nodes(d, len(d)) + TILE - 1) // TILE) * CODE)
    return o or 256


def weight_bytes(shape):
    return _section.sized(load().list_coarse_weight_bytes(C.byref(shape)), "list_coarse_weight_bytes")


def workspace_bytes(shape, B):
    return _section.sized(load().list_coarse_workspace_bytes(C.byref(shape), int(B)), "list_coarse_workspace_bytes")


def step_names(shape):
    return [f"tree_{l}" for l in range(shape.n_degrees)] + ["point_mlp", "point_max", "camera", "occ_clear", "occ_mark"]


# ---- parameters ------------------------------------------------------------------------------------------------------
def _parts(model):
    """(decoder, point MLP or None, camera or None) of a LIST, a CoarseNet or a bare TreeGraphDecoder."""
    dec = getattr(model, "point_decoder", model)
    if not hasattr(dec, "gcn"):
        raise RuntimeError(f"coarse: {type(model).__name__} holds no TreeGraphDecoder")
    return dec, getattr(model, "point_mlp_coarse", None), getattr(model, "spatial_transformer", None)


def _np(t):
    return t.detach().cpu().numpy()


def params_of(model, branch=True):
    """The stage's parameters as numpy arrays -- what decode_cpu reads (branch=False leaves W_branch, the one large
    array, where it is: None in its place)."""
    dec, mlp, cam = _parts(model)
    layers = []
    for g in dec.gcn:
        layers.append({"root": [_np(w.weight) for w in g.W_root], "branch": _np(g.W_branch) if branch else None,
                       "loop0": _np(g.W_loop[0].weight), "loop1": _np(g.W_loop[1].weight), "bias": _np(g.bias)[0],
                       "activation": bool(g.activation), "degree": int(g.degree)})
    features = [layers[0]["root"][0].shape[1]] + [l["root"][0].shape[0] for l in layers]
    out = {"features": features, "degrees": [l["degree"] for l in layers], "layers": layers, "mlp": None, "cam": None}

    def bn(m):
        s = stage.state_numpy(m)
        return {"g": s["weight"], "b": s["bias"], "m": s["running_mean"], "v": s["running_var"], "eps": float(m.eps)}
    if mlp is not None:
        out["mlp"] = [{"w": _np(blk[0].weight).reshape(blk[0].weight.shape[0], -1), "b": _np(blk[0].bias), "bn": bn(blk[1])}
                      for blk in (mlp.block1, mlp.block2, mlp.block3)]
    if cam is not None:
        out["cam"] = [{"w": _np(cam[0].weight), "b": _np(cam[0].bias), "bn": bn(cam[2])},
                      {"w": _np(cam[3].weight), "b": _np(cam[3].bias), "bn": bn(cam[5])},
                      {"w": _np(cam[6].weight), "b": _np(cam[6].bias), "bn": None}]
    return out


def shape_of_params(params):
    cam = params["cam"]
    return shape_of(params["features"], params["degrees"], [l["activation"] for l in params["layers"]],
                    has_mlp=params["mlp"] is not None, has_camera=cam is not None,
                    g2=cam[0]["w"].shape[1] - CODE if cam else 0, hidden=cam[0]["w"].shape[0] if cam else 0)


def compose(loop0, loop1, dtype=np.float32):
    """W_loop as one matrix: loop1 @ loop0 in float64, rounded once."""
    return (np.asarray(loop1, dtype=np.float64) @ np.asarray(loop0, dtype=np.float64)).astype(dtype)


def bn_affine(bn, exact=False):
    """Eval-mode BN as y * s + t.  fp32: s = g / sqrt(v + eps), t = b - m * s, each operation rounded; exact: float64."""
    return stage.bn_affine(bn["g"], bn["b"], bn["m"], bn["v"], bn["eps"], exact)


class Packed:
    """Prepared weights (list_coarse_prep_weights) on one device, and the W_branch parameters they go with."""

    def __init__(self, blob, shape, branches):
        self.blob, self.shape, self.branches = blob, shape, branches

    @property
    def device(self):
        return self.blob.device


def _prep(model):
    import torch
    dec, mlp, cam = _parts(model)
    dev = next(dec.parameters()).device
    stage.require_hip_module("coarse.pack", dev)
    params = params_of(model, branch=False)                       # W_branch stays on the device: never copied
    shape = shape_of_params(params)
    need = weight_bytes(shape)
    ptr, keep = stage.f32_pointers(dev)
    p = _Params()
    for l, lay in enumerate(params["layers"]):
        for i, w in enumerate(lay["root"]):
            p.w_root[l][i] = ptr(w)
        p.wc[l] = ptr(compose(lay["loop0"], lay["loop1"]))
        p.bias[l] = ptr(lay["bias"])
    for k, lay in enumerate(params["mlp"] or ()):
        s, t = bn_affine(lay["bn"])
        p.mlp_w[k], p.mlp_b[k], p.mlp_s[k], p.mlp_t[k] = ptr(lay["w"]), ptr(lay["b"]), ptr(s), ptr(t)
    for k, lay in enumerate(params["cam"] or ()):
        p.cam_w[k], p.cam_b[k] = ptr(lay["w"]), ptr(lay["b"])
        if lay["bn"] is not None:
            s, t = bn_affine(lay["bn"])
            p.cam_s[k], p.cam_t[k] = ptr(s), ptr(t)
    branches = []
    for g in dec.gcn:
        w = g.W_branch.detach()
        if w.dtype != torch.float32 or not w.is_contiguous() or w.data_ptr() % 16:
            raise RuntimeError("coarse.pack: W_branch must be a contiguous, 16-byte aligned float32 parameter (it is "
                               f"read in place): {w.dtype}, contiguous = {w.is_contiguous()}")
        branches.append(w)
    blob = stage.new_blob(dev, need)
    with torch.cuda.device(dev):
        _check(load().list_coarse_prep_weights(C.byref(shape), C.byref(p), blob.data_ptr(), need, hip._stream()),
               "list_coarse_prep_weights")
    return Packed(blob, shape, branches)          # (`keep` is released stream-ordered by the caching allocator)


def _module_tensors(model):
    ts = []
    for m in _parts(model):
        if m is not None:
            ts += list(m.parameters()) + list(m.buffers())
    return ts


def pack(model):
    """Prepared weights of the stage, cached on the module and keyed as voxenc.pack is: the SAME parameter and buffer
    tensors with unchanged version counters, storage addresses and devices."""
    return stage.pack_cached(model, "_coarse_pack", _module_tensors(model), lambda: _prep(model))


# ---- device ----------------------------------------------------------------------------------------------------------
class Buffers:
    """The workspace and the outputs of one call (occ is None without vox_res)."""

    def __init__(self, B, R, ws, pc, coarse, trans_mat, occ):
        self.B, self.R, self.ws, self.pc, self.coarse, self.trans_mat, self.occ = B, R, ws, pc, coarse, trans_mat, occ


def _f32(t, name, width, packed):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"coarse.decode: {name} must be a float32 tensor on a HIP device (got "
                           f"{getattr(t, 'dtype', None)} {getattr(t, 'device', None)})")
    if t.device != packed.device:
        raise RuntimeError(f"coarse.decode: weights on {packed.device}, {name} on {t.device}")
    t = t.detach().reshape(t.shape[0], -1).contiguous()
    if t.shape[1] != width:
        raise hip.ListError("coarse.decode", hip.ERR_SHAPE, f"{name} of shape {tuple(t.shape)}: {width} values per image")
    return t


def buffers(packed, B, vox_res=None):
    import torch
    s, dev = packed.shape, packed.device
    f, d = _lists(s)
    ws = torch.empty((workspace_bytes(s, B),), dtype=torch.uint8, device=dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    R = int(vox_res) if vox_res else 0
    return Buffers(B, R, ws, new(B, _nodes(d, len(d)), 3), new(B, CODE) if s.has_mlp else None,
                   new(B, 4, 3) if s.has_camera else None, new(B, R, R, R) if R else None)


def level_view(buf, packed, l):
    """Tree level l (1 .. L - 1) in a workspace: float32 [B,nodes,features]."""
    import torch
    f, d = _lists(packed.shape)
    o = sum(_align(4 * buf.B * _nodes(d, i) * f[i]) for i in range(1, l))
    n = buf.B * _nodes(d, l) * f[l]
    return buf.ws[o:o + 4 * n].view(torch.float32).view(buf.B, _nodes(d, l), f[l])


def tile_max_view(buf, packed):
    import torch
    f, d = _lists(packed.shape)
    o = sum(_align(4 * buf.B * _nodes(d, i) * f[i]) for i in range(1, len(d)))
    tiles = (_nodes(d, len(d)) + TILE - 1) // TILE
    return buf.ws[o:o + 4 * buf.B * tiles * CODE].view(torch.float32).view(buf.B, tiles, CODE)


def _io(packed, feat_g, feat_g2, buf, bb_min, bb_max):
    f, _ = _lists(packed.shape)
    feat_g = _f32(feat_g, "feat_g", f[0], packed)
    if feat_g.shape[0] != buf.B:
        raise RuntimeError(f"coarse.decode: feat_g of {feat_g.shape[0]} images on buffers of B = {buf.B}")
    io = _IO()
    io.B, io.R = buf.B, buf.R
    io.bb_min, io.bb_extent = float(bb_min), float(bb_max) - float(bb_min)
    io.feat_g = feat_g.data_ptr()
    keep = [feat_g]
    if feat_g2 is not None:
        feat_g2 = _f32(feat_g2, "feat_g2", packed.shape.g2, packed)
        if feat_g2.shape[0] != buf.B:
            raise RuntimeError(f"coarse.decode: feat_g2 of {feat_g2.shape[0]} images on buffers of B = {buf.B}")
        io.feat_g2 = feat_g2.data_ptr()
        keep.append(feat_g2)
    for l, w in enumerate(packed.branches):
        io.w_branch[l] = w.data_ptr()
    io.packed, io.packed_bytes = packed.blob.data_ptr(), packed.blob.numel()
    io.workspace, io.workspace_bytes = buf.ws.data_ptr(), buf.ws.numel()
    io.pc = buf.pc.data_ptr()
    for name in ("coarse", "trans_mat", "occ"):
        t = getattr(buf, name)
        setattr(io, name, t.data_ptr() if t is not None else None)
    return io, keep


def decode_steps(packed, feat_g, begin, end, feat_g2=None, buf=None, vox_res=None, bb_min=-0.5, bb_max=0.5):
    """Launches [begin, end) of the stage, in step_names() order, on `buf` (a previous call's; None allocates).
    Returns buf: .pc, .coarse, .trans_mat (written only with feat_g2), .occ (only with vox_res), .ws.  The launches
    before `begin` must have run on the same buffers."""
    import torch
    if buf is None:
        buf = buffers(packed, int(feat_g.shape[0]), vox_res)
    io, keep = _io(packed, feat_g, feat_g2, buf, bb_min, bb_max)
    with torch.cuda.device(packed.device):
        _check(load().list_coarse_forward_steps(C.byref(packed.shape), C.byref(io), int(begin), int(end), hip._stream()),
               "list_coarse_forward_steps")
    return buf


def decode(packed, feat_g, feat_g2=None, vox_res=None, bb_min=-0.5, bb_max=0.5):
    """The whole stage on the current stream -> (pc [B,P,3], coarse [B,512] or None, trans_mat [B,4,3] or None (without
    feat_g2, or for a network without a camera), occ [B,R,R,R] or None (without vox_res))."""
    import torch
    buf = buffers(packed, int(feat_g.shape[0]), vox_res)
    io, keep = _io(packed, feat_g, feat_g2, buf, bb_min, bb_max)
    with torch.cuda.device(packed.device):
        _check(load().list_coarse_forward(C.byref(packed.shape), C.byref(io), hip._stream()), "list_coarse_forward")
    return buf.pc, buf.coarse, buf.trans_mat if feat_g2 is not None else None, buf.occ


def time_steps(packed, feat_g, feat_g2=None, vox_res=None, reps=10):
    """Milliseconds per launch (median over reps), in step_names() order: each step alone between two events, on the
    buffers a whole forward has filled."""
    import torch
    buf = buffers(packed, int(feat_g.shape[0]), vox_res)
    io, keep = _io(packed, feat_g, feat_g2, buf, -0.5, 0.5)
    lib, n = load(), len(step_names(packed.shape))

    def run(b, e):
        _check(lib.list_coarse_forward_steps(C.byref(packed.shape), C.byref(io), b, e, hip._stream()),
               "list_coarse_forward_steps")
    with torch.cuda.device(packed.device):
        return stage.time_launches(run, n, reps)


def forward(model, feat_g, feat_g2=None, vox_res=None, bb_min=-0.5, bb_max=0.5):
    """The stage in HIP for an eval-mode model on a HIP device: decode(pack(model), ...).  Raises -- and never falls
    back to the torch modules -- when the model is in training mode (batch-statistics BN is not implemented) or when
    autograd would record the call (the stage has no HIP backward)."""
    mods = [m for m in _parts(model) if m is not None]
    stage.refuse_training_and_grad("coarse_stage", "stage", mods, [feat_g, feat_g2])
    return decode(pack(model), feat_g, feat_g2, vox_res, bb_min, bb_max)


# ---- host restatement ------------------------------------------------------------------------------------------------
def _leaky(x):
    return np.where(x > 0, x, x.dtype.type(SLOPE) * x)            # (a NaN stays a NaN)


def _relu(x):
    return np.where(x < 0, x.dtype.type(0), x)


def occupancy_cpu(pc, R, bb_min=-0.5, bb_max=0.5):
    """LIST.create_occ in numpy, operation for operation in fp32; a point with a non-finite coordinate marks nothing."""
    f32 = np.float32
    pc = np.asarray(pc).astype(f32)
    B = pc.shape[0]
    occ = np.zeros((B, R, R, R), dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((pc - f32(bb_min)) / f32(float(bb_max) - float(bb_min))).astype(f32) * f32(R - 1)
        t = np.floor(t.astype(f32) + f32(0.5))
        ok = np.isfinite(pc).all(axis=2)
        ijk = np.clip(np.where(np.isfinite(t), t, 0), 0, R - 1).astype(np.int64)
    for b in range(B):
        i = ijk[b][ok[b]]
        occ[b, i[:, 0], i[:, 1], i[:, 2]] = 1
    return occ


def tree_layer_cpu(params, l, levels, arithmetic="device"):
    """TreeGCN layer l on the levels before it ([B,nodes,features] each; levels[l]: the leaves) -> [B,nodes*deg,out]."""
    exact = arithmetic == "exact"
    lay, f64 = params["layers"][l], np.float64
    leaves = np.asarray(levels[l], dtype=f64)
    B, node, fin = leaves.shape
    deg, out = lay["degree"], lay["root"][0].shape[0]
    root = np.zeros((B, node, out), dtype=f64)
    for lvl, w in zip(levels[:l + 1], lay["root"]):
        z = np.asarray(lvl, dtype=f64) @ np.asarray(w, dtype=f64).T
        root += np.repeat(z, node // z.shape[1], axis=1)
    g = np.einsum("bni,nij->bnj", leaves, np.asarray(lay["branch"], dtype=f64)).reshape(B, node * deg, fin)
    if exact:
        grown = (_leaky(g) @ np.asarray(lay["loop0"], f64).T) @ np.asarray(lay["loop1"], f64).T
        z = np.repeat(root, deg, axis=1) + grown
        return _leaky(z + np.tile(np.asarray(lay["bias"], f64), (node, 1))) if lay["activation"] else z
    g = _leaky(g.astype(np.float32))
    wc = compose(lay["loop0"], lay["loop1"]).astype(f64)
    z = (np.repeat(root, deg, axis=1) + g.astype(f64) @ wc.T).astype(np.float32)
    if lay["activation"]:
        z = _leaky(z + np.tile(np.asarray(lay["bias"], np.float32), (node, 1)))
    return z


def _dense(x, lay, exact, kind):
    """One layer of the point MLP ("bn_relu": conv, BN, ReLU) or of the camera ("leaky_bn": Linear, leaky, BN; "none")."""
    ty = np.float64 if exact else np.float32
    z = (np.asarray(x, np.float64) @ np.asarray(lay["w"], np.float64).T).astype(ty) + np.asarray(lay["b"]).astype(ty)
    if kind == "none":
        return z
    s, t = bn_affine(lay["bn"], exact)
    return _relu(z * s + t) if kind == "bn_relu" else _leaky(z) * s + t


def decode_cpu(params, feat_g, feat_g2=None, arithmetic="device", vox_res=None, bb_min=-0.5, bb_max=0.5):
    """numpy restatement of the stage -> dict of every intermediate the steps produce: "levels" (the tree, level 0 the
    image code, the last one pc), "pc", "tile_max" [B,tiles,512], "coarse", "hidden" (the camera's two), "trans_mat",
    "occ" (those the network and the arguments give; the others None).

    arithmetic="device": fp32 inputs, sums in float64 rounded once per output, fp32 epilogues, the composed Wc.
    arithmetic="exact": float64 throughout and W_loop uncomposed -- the reference formula."""
    if arithmetic not in ("device", "exact"):
        raise ValueError(f"arithmetic = {arithmetic!r}: 'device' or 'exact'")
    exact = arithmetic == "exact"
    ty = np.float64 if exact else np.float32
    feat_g = np.asarray(feat_g)
    B = feat_g.shape[0]
    out = dict.fromkeys(("tile_max", "coarse", "hidden", "trans_mat", "occ"))
    with np.errstate(invalid="ignore", over="ignore"):
        levels = [feat_g.reshape(B, 1, -1).astype(ty)]
        for l in range(len(params["layers"])):
            levels.append(tree_layer_cpu(params, l, levels, arithmetic))
        pc = levels[-1]
        out["levels"], out["pc"] = levels, pc
        if params["mlp"] is not None:
            h = pc
            for lay in params["mlp"]:
                h = _dense(h, lay, exact, "bn_relu")
            P = pc.shape[1]
            tiles = (P + TILE - 1) // TILE
            out["tile_max"] = np.stack([h[:, i * TILE:min(P, (i + 1) * TILE)].max(axis=1) for i in range(tiles)], axis=1)
            out["coarse"] = out["tile_max"].max(axis=1)
        if params["cam"] is not None and feat_g2 is not None:
            x = np.concatenate([out["coarse"], np.asarray(feat_g2).reshape(B, -1).astype(ty)], axis=1)
            h1 = _dense(x, params["cam"][0], exact, "leaky_bn")
            h2 = _dense(h1, params["cam"][1], exact, "leaky_bn")
            out["hidden"] = [h1, h2]
            out["trans_mat"] = _dense(h2, params["cam"][2], exact, "none").reshape(B, 4, 3)
        if vox_res:
            out["occ"] = occupancy_cpu(pc, int(vox_res), bb_min, bb_max)
    return out
