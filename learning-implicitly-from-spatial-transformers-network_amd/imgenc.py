"""The image encoder (network.modules.ResEncoder: ResNet-18 with a stride-1 7x7 stem) in HIP: its inference forward,
from the image [B,3,H,W] to the global 128-vector and the five feature maps, through liblist_hip.so
(include/list_imgenc.h).

One arithmetic: the stem in fp32, every other convolution an implicit GEMM on the matrix cores with fp16 operands and
fp32 accumulation, the epilogue (acc * s + t, plus the identity, ReLU) in fp32; activations between layers are fp16
channels-last in the workspace, the five levels are the fp32 epilogue values, channels-last, which hotpath and
list_prep_img_maps read where they lie.  fp16 values are not saturated.  Eval mode only: the training forward
(batch-statistics BN) and the backward stay with the torch module; `forward` refuses them instead of falling back.

  pack(module)            -> Packed: the prepared weights on the module's device, cached on the module
  encode(packed, img)     -> (vec [B,128], [f0 .. f4] as [B,C,h,w] views with channels-last strides)
  forward(module, img)    -> pack + encode, after the eval-mode / no-gradient checks (what LIST.encode calls)
  encode_cpu(params, img, arithmetic, storage)   the numpy restatement: the test oracle, not a path of the model
"""
import ctypes as C

import numpy as np

from . import hip, stage

N_LEVELS, N_CONVS, MIN_HW, MAX_HW, VEC, FC = 5, 20, 32, 512, 128, 1000
LEVEL_CHANNELS = (64, 64, 128, 256, 512)


class _Conv(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bn_weight", C.c_void_p), ("bn_bias", C.c_void_p), ("bn_mean", C.c_void_p),
                ("bn_var", C.c_void_p), ("bn_eps", C.c_float)]


class _Params(C.Structure):
    _fields_ = [("conv", _Conv * N_CONVS), ("fc_w", C.c_void_p), ("fc_b", C.c_void_p), ("fc1_w", C.c_void_p),
                ("fc1_b", C.c_void_p)]


class _IO(C.Structure):
    _fields_ = [("img", C.c_void_p), ("img_sb", C.c_int64), ("img_sc", C.c_int64), ("img_sh", C.c_int64),
                ("img_sw", C.c_int64), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("packed", C.c_void_p),
                ("packed_bytes", C.c_size_t), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("vec", C.c_void_p), ("levels_out", C.c_void_p * N_LEVELS)]


IMGENC_EXPORTS = {
    "list_imgenc_weight_bytes": (C.c_size_t, []),
    "list_imgenc_prep_weights": (C.c_int, [C.POINTER(_Params), C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_imgenc_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "list_imgenc_forward": (C.c_int, [C.POINTER(_IO), C.c_void_p]),
    "list_imgenc_n_steps": (C.c_int32, []),
    "list_imgenc_forward_steps": (C.c_int, [C.POINTER(_IO), C.c_int32, C.c_int32, C.c_void_p]),
    "list_imgenc_last_error": (C.c_char_p, []),
}

_section = hip.Section(IMGENC_EXPORTS, "list_imgenc_last_error")    # include/list_imgenc.h on hip.load()'s handle
load, _check, last_error = _section.load, _section.check, _section.last_error


# ---- the fixed network as a table of launches (the C side's make_net) ------------------------------------------------
class Step:
    """One launch.  kind: "stem", "pool", "conv" or "head"; the output is (H >> shift) x (W >> shift) x cout; src / idt:
    index of the launch whose fp16 activation is the input / the identity (None: none); level: index of the fp32 level
    written beside the activation; key / bn: state_dict prefixes of the convolution and its BN."""

    def __init__(self, name, kind, cin, cout, ks, stride, shift, src, idt, level, relu, key=None, bn=None):
        self.name, self.kind, self.cin, self.cout, self.ks, self.stride, self.shift = name, kind, cin, cout, ks, stride, shift
        self.src, self.idt, self.level, self.relu, self.key, self.bn = src, idt, level, relu, key, bn


def _make_steps():
    s = [Step("stem", "stem", 3, 64, 7, 1, 0, None, None, 0, True, "conv1", "bn1"),
         Step("pool", "pool", 64, 64, 3, 2, 1, 0, None, None, False)]

    def conv(name, cin, cout, ks, stride, shift, src, idt, level, relu, key, bn):
        s.append(Step(name, "conv", cin, cout, ks, stride, shift, src, idt, level, relu, key, bn))
    conv("layer1_0_conv1", 64, 64, 3, 1, 1, 1, None, None, True, "layer1.0.conv1", "layer1.0.bn1")
    conv("layer1_0_conv2", 64, 64, 3, 1, 1, 2, 1, None, True, "layer1.0.conv2", "layer1.0.bn2")
    conv("layer1_1_conv1", 64, 64, 3, 1, 1, 3, None, None, True, "layer1.1.conv1", "layer1.1.bn1")
    conv("layer1_1_conv2", 64, 64, 3, 1, 1, 4, 3, 1, True, "layer1.1.conv2", "layer1.1.bn2")
    for L in (2, 3, 4):
        b, cin = len(s), 32 << (L - 1)
        cout, p = 2 * cin, f"layer{L}"
        conv(f"{p}_0_conv1", cin, cout, 3, 2, L, b - 1, None, None, True, f"{p}.0.conv1", f"{p}.0.bn1")
        conv(f"{p}_0_down", cin, cout, 1, 2, L, b - 1, None, None, False, f"{p}.0.downsample.0", f"{p}.0.downsample.1")
        conv(f"{p}_0_conv2", cout, cout, 3, 1, L, b, b + 1, None, True, f"{p}.0.conv2", f"{p}.0.bn2")
        conv(f"{p}_1_conv1", cout, cout, 3, 1, L, b + 2, None, None, True, f"{p}.1.conv1", f"{p}.1.bn1")
        conv(f"{p}_1_conv2", cout, cout, 3, 1, L, b + 3, b + 2, L, True, f"{p}.1.conv2", f"{p}.1.bn2")
    s.append(Step("head", "head", 512, VEC, 1, 1, 4, None, None, None, False))
    return s


STEPS = _make_steps()
CONV_STEPS = [s for s in STEPS if s.key]                   # in ListImgencParams.conv order


def step_names():
    return [s.name for s in STEPS]


def n_steps():
    return int(load().list_imgenc_n_steps())


# ---- closed forms of the two buffer sizes (the C side is the authority; the tests compare) ---------------------------
_align = stage.align256


def weight_bytes_closed_form():
    """Per convolution its weights (fp32 [147][64] for the stem, else the fp16 MFMA operand: cin k k cout halfs) and the BN
    scale and shift; the composed head [512][128] and its bias.  Every array starts on a 256-byte boundary."""
    o = 0
    for s in CONV_STEPS:
        o += _align(147 * 64 * 4 if s.kind == "stem" else s.cin * s.ks * s.ks * s.cout * 2) + 2 * _align(s.cout * 4)
    return o + _align(512 * VEC * 4) + _align(VEC * 4)


def _act_offsets(B, H, W):
    offs, o = [], 0
    for s in STEPS[:-1]:
        offs.append(o)
        o += _align(B * (H >> s.shift) * (W >> s.shift) * s.cout * 2)
    return offs, o


def workspace_bytes_closed_form(B, H, W):
    """One fp16 channels-last activation per launch but the head."""
    return _act_offsets(B, H, W)[1]


def weight_bytes():
    return int(load().list_imgenc_weight_bytes())


def workspace_bytes(B, H, W):
    return _section.sized(load().list_imgenc_workspace_bytes(int(B), int(H), int(W)), "list_imgenc_workspace_bytes")


# ---- parameters ------------------------------------------------------------------------------------------------------
def _bn_of(module, prefix):
    m = module
    for part in prefix.split("."):
        m = m[int(part)] if part.isdigit() else getattr(m, part)
    return m


def params_of(module):
    """The encoder's parameters as numpy arrays: {"state": state_dict as numpy, "eps": BN prefix -> eps} -- what
    encode_cpu reads."""
    return {"state": stage.state_numpy(module),
            "eps": {s.bn: float(_bn_of(module, s.bn).eps) for s in CONV_STEPS}}


class Packed:
    """Prepared weights (list_imgenc_prep_weights) on one device."""

    def __init__(self, blob):
        self.blob = blob

    @property
    def device(self):
        return self.blob.device

    def head(self):
        """The composed head as the device holds it: (W [128,512], bias [128]) float32 tensors."""
        import torch
        o = weight_bytes_closed_form() - _align(512 * VEC * 4) - _align(VEC * 4)
        wt = self.blob[o:o + 512 * VEC * 4].view(torch.float32).view(512, VEC)
        o += _align(512 * VEC * 4)
        return wt.t(), self.blob[o:o + VEC * 4].view(torch.float32)


def _prep(module):
    import torch
    dev = next(module.parameters()).device
    stage.require_hip_module("imgenc.pack", dev)
    need = weight_bytes()
    ptr, keep = stage.f32_pointers()
    p = _Params()
    for i, s in enumerate(CONV_STEPS):
        bn = _bn_of(module, s.bn)
        c = p.conv[i]
        c.w = ptr(_bn_of(module, s.key).weight)
        c.bn_weight, c.bn_bias, c.bn_mean, c.bn_var = ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var)
        c.bn_eps = float(bn.eps)
    p.fc_w, p.fc_b, p.fc1_w, p.fc1_b = ptr(module.fc.weight), ptr(module.fc.bias), ptr(module.fc1.weight), ptr(module.fc1.bias)
    blob = stage.new_blob(dev, need)
    with torch.cuda.device(dev):
        _check(load().list_imgenc_prep_weights(C.byref(p), blob.data_ptr(), need, hip._stream()),
               "list_imgenc_prep_weights")
    return Packed(blob)


def pack(module):
    """Prepared weights of a ResEncoder, cached on the module for its parameter and buffer tensors as they are
    (stage.pack_cached: an optimizer step, load_state_dict, module.to() or .half() all rebuild)."""
    tensors = list(module.parameters()) + list(module.buffers())
    return stage.pack_cached(module, "_imgenc_pack", tensors, lambda: _prep(module))


# ---- device ----------------------------------------------------------------------------------------------------------
def _buffers(packed, img):
    import torch
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.float32 or img.dim() != 4 \
            or img.shape[1] != 3:
        raise RuntimeError("imgenc.encode: img must be a float32 [B,3,H,W] tensor on a HIP device (got "
                           f"{getattr(img, 'dtype', None)} {getattr(img, 'device', None)} "
                           f"{tuple(getattr(img, 'shape', ()))})")
    if packed.device != img.device:
        raise RuntimeError(f"imgenc.encode: weights on {packed.device}, img on {img.device}")
    B, H, W = int(img.shape[0]), int(img.shape[2]), int(img.shape[3])
    need = workspace_bytes(B, H, W)
    dev = img.device
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    vec = torch.empty((B, VEC), dtype=torch.float32, device=dev)
    store = [torch.empty((B, H >> k, W >> k, c), dtype=torch.float32, device=dev) for k, c in enumerate(LEVEL_CHANNELS)]
    return B, H, W, ws, vec, store


def _io(packed, img, buffers):
    B, H, W, ws, vec, store = buffers
    io = _IO()
    io.img = img.data_ptr()
    io.img_sb, io.img_sc, io.img_sh, io.img_sw = [int(x) for x in img.stride()]
    io.B, io.H, io.W = B, H, W
    io.packed, io.packed_bytes = packed.blob.data_ptr(), packed.blob.numel()
    io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel()
    io.vec = vec.data_ptr()
    for k, s in enumerate(store):
        io.levels_out[k] = s.data_ptr()
    return io


def _views(store):
    return [s.permute(0, 3, 1, 2) for s in store]


def encode_steps(packed, img, begin, end, buffers=None):
    """Launches [begin, end) of the forward, in step_names() order, on `buffers` (those a previous call returned; None
    allocates them).  Returns (vec, levels, ws, buffers): encode()'s outputs, the workspace and the handle to pass on.
    The launches before `begin` must have run on the same buffers."""
    import torch
    if buffers is None:
        buffers = _buffers(packed, img)
    if tuple(img.shape) != (buffers[0], 3, buffers[1], buffers[2]):
        raise RuntimeError(f"imgenc.encode_steps: img of shape {tuple(img.shape)} on buffers of B, H, W = {buffers[:3]}")
    io = _io(packed, img, buffers)
    with torch.cuda.device(img.device):
        _check(load().list_imgenc_forward_steps(C.byref(io), int(begin), int(end), hip._stream()),
               "list_imgenc_forward_steps")
    return buffers[4], _views(buffers[5]), buffers[3], buffers


def encode(packed, img):
    """img float32 [B,3,H,W] on the device (any strides) -> (vec float32 [B,128], [f0 .. f4]: float32, logically
    [B,C,h,w] with channels-last strides).  Enqueued on the current stream."""
    import torch
    buffers = _buffers(packed, img)
    io = _io(packed, img, buffers)
    with torch.cuda.device(img.device):
        _check(load().list_imgenc_forward(C.byref(io), hip._stream()), "list_imgenc_forward")
    return buffers[4], _views(buffers[5])


def mid_view(ws, B, H, W, name):
    """The fp16 activation that launch `name` (step_names(); not the head) wrote, in a workspace that encode_steps
    returned: float16 [B,C,h,w] view with channels-last strides."""
    import torch
    k = step_names().index(name)
    s = STEPS[k]
    if s.kind == "head":
        raise ValueError("the head writes vec, not an activation")
    o = _act_offsets(B, H, W)[0][k]
    h, w = H >> s.shift, W >> s.shift
    n = B * h * w * s.cout
    return ws[o:o + 2 * n].view(torch.float16).view(B, h, w, s.cout).permute(0, 3, 1, 2)


def time_steps(packed, img, reps=10):
    """Milliseconds per launch of the forward (median over reps), in step_names() order: each step alone between two
    events, on the buffers a whole forward has filled."""
    import torch
    buffers = _buffers(packed, img)
    io = _io(packed, img, buffers)
    lib = load()

    def run(b, e):
        _check(lib.list_imgenc_forward_steps(C.byref(io), b, e, hip._stream()), "list_imgenc_forward_steps")
    with torch.cuda.device(img.device):
        return stage.time_launches(run, lib.list_imgenc_n_steps(), reps)


def step_flops(B, H, W):
    """Floating-point operations of every launch (2 per multiply-add; 0 for the pool), in step_names() order."""
    out = []
    for s in STEPS:
        px = B * (H >> s.shift) * (W >> s.shift)
        out.append(0 if s.kind == "pool" else 2 * 512 * VEC * B + 512 * px if s.kind == "head"
                   else 2 * px * s.cin * s.ks * s.ks * s.cout)
    return out


def step_bytes(B, H, W):
    """Bytes every launch must move at least (its input, identity, outputs and weights once), in step_names() order."""
    out = []
    for s in STEPS:
        px = B * (H >> s.shift) * (W >> s.shift)
        if s.kind == "head":
            out.append(px * 512 * 4 + 512 * VEC * 4)
            continue
        pin = px * s.stride * s.stride
        n = pin * s.cin * (4 if s.kind == "stem" else 2) + px * s.cout * 2
        n += px * s.cout * 2 if s.idt is not None else 0
        n += px * s.cout * 4 if s.level is not None else 0
        n += 0 if s.kind == "pool" else s.cin * s.ks * s.ks * s.cout * (4 if s.kind == "stem" else 2)
        out.append(n)
    return out


def forward(module, img):
    """ResEncoder.forward in HIP for an eval-mode module on a HIP device.  Raises -- and never falls back to the torch
    module -- when the module is in training mode (batch-statistics BN is not implemented), when autograd would record
    the call (there is no HIP backward of the encoder), or when the module is not on a HIP device."""
    stage.refuse_training_and_grad("img_encoder", "encoder", [module], [img])
    return encode(pack(module), img)


# ---- host restatement ------------------------------------------------------------------------------------------------
def _conv2(x, w, stride, pad):
    """x float64 [B,H,W,Cin], w float64 [Cout,Cin,k,k] -> float64 [B,Ho,Wo,Cout]: cross-correlation, zero padding,
    accumulated in float64."""
    k = w.shape[2]
    H, W = x.shape[1:3]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    wt = np.ascontiguousarray(w.transpose(2, 3, 1, 0))      # [k,k,Cin,Cout]
    out = np.zeros((x.shape[0], Ho, Wo, w.shape[0]), dtype=np.float64)
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :] @ wt[ky, kx]
    return out


def _pool(x):
    """3x3 stride-2 pad-1 max-pool of [B,H,W,C]; a NaN wins, the padding never does."""
    H, W = x.shape[1:3]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-np.inf)
    out = None
    for dy in range(3):
        for dx in range(3):
            v = xp[:, dy:dy + H - 1:2, dx:dx + W - 1:2, :]
            out = v if out is None else np.maximum(out, v)
    return out


def bn_affine(state, eps, prefix, exact=False):
    """s, t of the BN `prefix`: in fp32, operation for operation as the device's prep computes them, or in float64."""
    return stage.bn_affine(state[prefix + ".weight"], state[prefix + ".bias"], state[prefix + ".running_mean"],
                           state[prefix + ".running_var"], eps, exact)


def compose_head(state, dtype=np.float32):
    """fc1 o fc as one matrix [128,512] and one bias, composed in float64 and rounded once to `dtype`."""
    f64 = np.float64
    w1, w0 = np.asarray(state["fc1.weight"]).astype(f64), np.asarray(state["fc.weight"]).astype(f64)
    b = w1 @ np.asarray(state["fc.bias"]).astype(f64) + np.asarray(state["fc1.bias"]).astype(f64)
    return (w1 @ w0).astype(dtype), b.astype(dtype)


def encode_cpu(params, img, arithmetic="device", storage="fp16"):
    """numpy restatement of the encoder.  img: [B,3,H,W]; params: params_of(module).  Returns a dict: every launch's
    output under its step name as a channels-last array [B,h,w,C] (the activation as it is stored; "head" is vec), "vec"
    [B,128] and "levels", the five maps as [B,C,h,w] (the epilogue values before the storage rounding).

    arithmetic="device" states the device arithmetic: sums in float64 rounded once to float32, the epilogue (scale,
    shift, identity, ReLU) in float32, the head composed.  storage="fp16": the weights of the matrix-core layers and
    the activations between layers rounded to fp16, as on the device; storage="fp32": neither is rounded (the same
    graph in fp32, for the bound against "exact").  arithmetic="exact": float64 throughout, fc and fc1 uncomposed
    (`storage` is not used)."""
    if arithmetic not in ("device", "exact"):
        raise ValueError(f"arithmetic = {arithmetic!r}: 'device' or 'exact'")
    if storage not in ("fp16", "fp32"):
        raise ValueError(f"storage = {storage!r}: 'fp16' or 'fp32'")
    exact, half = arithmetic == "exact", arithmetic == "device" and storage == "fp16"
    st, eps = params["state"], params["eps"]
    f32, f64 = np.float32, np.float64
    work = f64 if exact else f32
    x = np.moveaxis(np.asarray(img), 1, 3)
    out, acts, levels = {}, [], [None] * N_LEVELS
    with np.errstate(over="ignore", invalid="ignore"):
        for s in STEPS:
            if s.kind == "pool":
                y = lvl = _pool(acts[s.src])
            elif s.kind == "head":
                f4 = levels[4].astype(f64)
                if exact:
                    mean = f4.mean(axis=(1, 2))
                    z = mean @ np.asarray(st["fc.weight"]).astype(f64).T + np.asarray(st["fc.bias"]).astype(f64)
                    y = z @ np.asarray(st["fc1.weight"]).astype(f64).T + np.asarray(st["fc1.bias"]).astype(f64)
                else:
                    hw = f4.shape[1] * f4.shape[2]
                    mean = f4.reshape(f4.shape[0], hw, -1).sum(axis=1).astype(f32) / f32(hw)
                    wc, bc = compose_head(st)
                    y = (mean.astype(f64) @ wc.astype(f64).T).astype(f32) + bc
                out["vec"] = lvl = y
            else:
                w = np.asarray(st[s.key + ".weight"])
                w = w.astype(f64) if exact else w.astype(f32)
                if half and s.kind == "conv":
                    w = w.astype(np.float16)
                src = x if s.kind == "stem" else acts[s.src]
                z = _conv2(src.astype(f64), w.astype(f64), s.stride, s.ks // 2).astype(work)
                sc, sh = bn_affine(st, eps[s.bn], s.bn, exact)
                v = z * sc + sh                                  # float32: two roundings, as on the device
                if s.idt is not None:
                    v = v + acts[s.idt].astype(work)
                if s.relu:
                    v = np.where(v < 0, work(0), v)              # (a NaN stays a NaN)
                lvl = v
                y = v.astype(np.float16) if half else v
            out[s.name] = y
            acts.append(y)
            if s.level is not None:
                levels[s.level] = lvl
    out["levels"] = [np.moveaxis(v, 3, 1) for v in levels]
    return out
