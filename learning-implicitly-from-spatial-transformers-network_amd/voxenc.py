"""The 3-D occupancy encoder (network.modules.VoxelEncoder2) in HIP: its inference forward, from the occupancy grid
[B,R,R,R] to the six feature volumes, through liblist_hip.so (include/list_voxenc.h).

One arithmetic: the one-channel convolutions (conv_0 .. conv_3) in fp32, every other convolution an implicit GEMM on
the matrix cores with fp16 operands and fp32 accumulation; level 0 is fp32, the activations between layers and levels
1 .. 5 are fp16 channels-last, which hip.prep_vox_maps(levels, "f16") takes where they lie.  fp16 values are not
saturated.  Eval mode only: the training forward (batch-statistics BN) and the backward stay with the torch module;
`forward` refuses them instead of falling back.

  pack(module)            -> Packed: the prepared weights on the module's device, cached on the module
  encode(occ, packed)     -> the six torch tensors
  forward(module, occ)    -> pack + encode, after the eval-mode / no-gradient checks (what LIST.encode calls)
  encode_cpu(occ, params, storage)   the numpy restatement: the test oracle, not a path of the model
"""
import ctypes as C

import numpy as np

from . import hip, stage

N_LAYERS, N_LEVELS, MAX_R = 9, 6, 256
N_STAGES = N_LAYERS - 1
MFMA_CHANNELS = (16, 32, 64, 128)


class _Stage(C.Structure):
    _fields_ = [("conv_w", C.c_void_p), ("conv_b", C.c_void_p), ("conv2_w", C.c_void_p), ("conv2_b", C.c_void_p),
                ("bn_weight", C.c_void_p), ("bn_bias", C.c_void_p), ("bn_mean", C.c_void_p), ("bn_var", C.c_void_p),
                ("bn_eps", C.c_float)]


_I32P = C.POINTER(C.c_int32)
_FWD_ARGS = [C.c_void_p, C.c_int32, C.c_int32, _I32P, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
             C.POINTER(C.c_void_p)]
VOXENC_EXPORTS = {
    "list_voxenc_weight_bytes": (C.c_size_t, [_I32P, C.c_int32]),
    "list_voxenc_prep_weights": (C.c_int, [C.POINTER(_Stage), _I32P, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_voxenc_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, _I32P, C.c_int32]),
    "list_voxenc_forward": (C.c_int, _FWD_ARGS + [C.c_void_p]),
    "list_voxenc_n_steps": (C.c_int32, [_I32P, C.c_int32]),
    "list_voxenc_forward_steps": (C.c_int, _FWD_ARGS + [C.c_int32, C.c_int32, C.c_void_p]),
    "list_voxenc_last_error": (C.c_char_p, []),
}

_section = hip.Section(VOXENC_EXPORTS, "list_voxenc_last_error")    # include/list_voxenc.h on hip.load()'s handle
load, _check, last_error = _section.load, _section.check, _section.last_error


def _layers_arg(layers):
    layers = [int(c) for c in layers]
    return (C.c_int32 * len(layers))(*layers), len(layers)


# ---- closed forms of the two buffer sizes (the C side is the authority; the tests compare) ---------------------------
_align = stage.align256


def _wpk_bytes(cin, cout):
    steps = 14 if cin == 16 else (cin // 32) * 27
    return steps * (cout // 16) * 64 * 8 * 2


def weight_bytes_closed_form(layers):
    """Packed blob: per stage the first convolution's weights (fp32 [C][27] for one input channel, else the fp16 MFMA
    operand) and bias, BN scale and shift for stages 0 and 1; from stage 3 on the second convolution's weights, bias,
    scale and shift.  Every array starts on a 256-byte boundary."""
    o = 0
    for l in range(N_STAGES):
        cin, cout = layers[l], layers[l + 1]
        o += _align(cout * 27 * 4 if cin == 1 else _wpk_bytes(cin, cout)) + _align(cout * 4)
        if l < 2:
            o += 2 * _align(cout * 4)
        if l >= 3:
            o += _align(_wpk_bytes(cout, cout)) + 3 * _align(cout * 4)
    return o


def workspace_bytes_closed_form(B, R, layers):
    """Two fp32 one-channel volumes, the largest fp16 activation between the two convolutions of a stage, and the
    pooled outputs of stages 3 .. 6."""
    o = 2 * _align(B * R ** 3 * 4)
    o += _align(max(B * (R >> (l - 3)) ** 3 * layers[l + 1] * 2 for l in range(3, N_STAGES)))
    for l in range(3, N_STAGES - 1):
        o += _align(B * (R >> (l - 2)) ** 3 * layers[l + 1] * 2)
    return o


def weight_bytes(layers):
    arr, n = _layers_arg(layers)
    return _section.sized(load().list_voxenc_weight_bytes(arr, n), "list_voxenc_weight_bytes")


def workspace_bytes(B, R, layers):
    arr, n = _layers_arg(layers)
    return _section.sized(load().list_voxenc_workspace_bytes(int(B), int(R), arr, n), "list_voxenc_workspace_bytes")


# ---- parameters ------------------------------------------------------------------------------------------------------
def params_of(module):
    """The encoder's parameters as numpy arrays: {"layers", "eps": per stage, "state": state_dict as numpy} -- what
    encode_cpu reads."""
    return {"layers": [int(c) for c in module.layers], "eps": [float(b.eps) for b in module.bn],
            "state": stage.state_numpy(module)}


class Packed:
    """Prepared weights (list_voxenc_prep_weights) on one device."""

    def __init__(self, blob, layers):
        self.blob, self.layers = blob, [int(c) for c in layers]

    @property
    def device(self):
        return self.blob.device


def _prep(module):
    import torch
    layers = [int(c) for c in module.layers]
    dev = next(module.parameters()).device
    stage.require_hip_module("voxenc.pack", dev)
    need = weight_bytes(layers)
    ptr, keep = stage.f32_pointers()
    stages = (_Stage * N_STAGES)()
    for l in range(N_STAGES):
        conv, bn = module.conv[f"conv_{l}"], module.bn[l]
        st = stages[l]
        st.conv_w, st.conv_b = ptr(conv.weight), ptr(conv.bias)
        if l > 2:
            conv2 = module.conv[f"conv_{l}_0"]
            st.conv2_w, st.conv2_b = ptr(conv2.weight), ptr(conv2.bias)
        st.bn_weight, st.bn_bias = ptr(bn.weight), ptr(bn.bias)
        st.bn_mean, st.bn_var = ptr(bn.running_mean), ptr(bn.running_var)
        st.bn_eps = float(bn.eps)
    arr, n = _layers_arg(layers)
    blob = stage.new_blob(dev, need)
    with torch.cuda.device(dev):
        _check(load().list_voxenc_prep_weights(stages, arr, n, blob.data_ptr(), need, hip._stream()),
               "list_voxenc_prep_weights")
    return Packed(blob, layers)


def pack(module):
    """Prepared weights of a VoxelEncoder2, cached on the module for its parameter and buffer tensors as they are
    (stage.pack_cached: an optimizer step, load_state_dict, module.to() or .half() all rebuild)."""
    tensors = list(module.parameters()) + list(module.buffers())
    return stage.pack_cached(module, "_voxenc_pack", tensors, lambda: _prep(module))


# ---- device ----------------------------------------------------------------------------------------------------------
def _buffers(occ, packed):
    import torch
    if not isinstance(occ, torch.Tensor) or not occ.is_cuda or occ.dtype != torch.float32 or occ.dim() != 4:
        raise RuntimeError("voxenc.encode: occ must be a float32 [B,R,R,R] tensor on a HIP device (got "
                           f"{getattr(occ, 'dtype', None)} {getattr(occ, 'device', None)} "
                           f"{tuple(getattr(occ, 'shape', ()))})")
    B, R = int(occ.shape[0]), int(occ.shape[1])
    if occ.shape[2] != R or occ.shape[3] != R:
        raise hip.ListError("voxenc.encode", hip.ERR_SHAPE, f"occ of shape {tuple(occ.shape)}: the grid must be a cube")
    if packed.device != occ.device:
        raise RuntimeError(f"voxenc.encode: weights on {packed.device}, occ on {occ.device}")
    layers = packed.layers
    need = workspace_bytes(B, R, layers)
    dev = occ.device
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    store = [torch.empty((B, R, R, R), dtype=torch.float32, device=dev)]
    for k in range(1, N_LEVELS):
        D = R >> (k - 1)
        store.append(torch.empty((B, D, D, D, layers[k + 3]), dtype=torch.float16, device=dev))
    return B, R, ws, store


def _views(store):
    return [store[0].unsqueeze(1)] + [s.permute(0, 4, 1, 2, 3) for s in store[1:]]


def encode(occ, packed, return_workspace=False):
    """occ float32 [B,R,R,R] on the device -> [level 0: float32 [B,1,R,R,R]; levels 1 .. 5: float16, logically
    [B,C,D,D,D] with channels_last_3d strides].  Enqueued on the current stream."""
    import torch
    B, R, ws, store = _buffers(occ, packed)
    occ = occ.contiguous()
    arr, n = _layers_arg(packed.layers)
    outs = (C.c_void_p * N_LEVELS)(*[s.data_ptr() for s in store])
    with torch.cuda.device(occ.device):
        _check(load().list_voxenc_forward(occ.data_ptr(), B, R, arr, n, packed.blob.data_ptr(), packed.blob.numel(),
                                          ws.data_ptr(), ws.numel(), outs, hip._stream()), "list_voxenc_forward")
    levels = _views(store)
    return (levels, ws) if return_workspace else levels


def pooled_view(ws, B, R, layers, stage):
    """The max-pooled output of `stage` (3 .. 6) in a workspace that encode(..., return_workspace=True) returned:
    float16 [B,C,D,D,D] view with channels_last_3d strides."""
    import torch
    o = 2 * _align(B * R ** 3 * 4)
    o += _align(max(B * (R >> (l - 3)) ** 3 * layers[l + 1] * 2 for l in range(3, N_STAGES)))
    for l in range(3, stage):
        o += _align(B * (R >> (l - 2)) ** 3 * layers[l + 1] * 2)
    D, Cc = R >> (stage - 2), layers[stage + 1]
    n = B * D ** 3 * Cc
    return ws[o:o + 2 * n].view(torch.float16).view(B, D, D, D, Cc).permute(0, 4, 1, 2, 3)


def mid_view(ws, B, R, layers, stage):
    """The activation between the two convolutions of `stage` (3 .. 7) in a workspace: float16 [B,C,D,D,D] view with
    channels_last_3d strides, C = layers[stage + 1], D = R >> (stage - 3).  One buffer serves every stage: the view
    holds that stage's activation only between its two launches (see encode_steps)."""
    import torch
    o = 2 * _align(B * R ** 3 * 4)
    D, Cc = R >> (stage - 3), layers[stage + 1]
    n = B * D ** 3 * Cc
    return ws[o:o + 2 * n].view(torch.float16).view(B, D, D, D, Cc).permute(0, 4, 1, 2, 3)


def encode_steps(occ, packed, begin, end, buffers=None):
    """Launches [begin, end) of the forward, in step_names() order, on `buffers` (those a previous call returned; None
    allocates them).  Returns (levels, ws, buffers): the six level views of encode(), the workspace and the handle to
    pass on.  The launches before `begin` must have run on the same buffers."""
    import torch
    if buffers is None:
        buffers = _buffers(occ, packed)
    B, R, ws, store = buffers
    if tuple(occ.shape) != (B, R, R, R):
        raise RuntimeError(f"voxenc.encode_steps: occ of shape {tuple(occ.shape)} on buffers of B = {B}, R = {R}")
    occ = occ.contiguous()
    arr, n = _layers_arg(packed.layers)
    outs = (C.c_void_p * N_LEVELS)(*[s.data_ptr() for s in store])
    with torch.cuda.device(occ.device):
        _check(load().list_voxenc_forward_steps(occ.data_ptr(), B, R, arr, n, packed.blob.data_ptr(),
                                                packed.blob.numel(), ws.data_ptr(), ws.numel(), outs, int(begin),
                                                int(end), hip._stream()), "list_voxenc_forward_steps")
    return _views(store), ws, buffers


def step_names(layers):
    names = ["conv_0", "conv_1", "conv_2"]
    for l in range(3, N_STAGES):
        names += [f"conv_{l}", f"conv_{l}_0"]
    return names


def time_steps(occ, packed, reps=10):
    """Milliseconds per launch of the forward (median over reps), in step_names() order: each step alone between two
    events, on the buffers a whole forward has filled."""
    import torch
    B, R, ws, store = _buffers(occ, packed)
    occ = occ.contiguous()
    arr, n = _layers_arg(packed.layers)
    outs = (C.c_void_p * N_LEVELS)(*[s.data_ptr() for s in store])
    lib = load()
    n_steps = lib.list_voxenc_n_steps(arr, n)

    def run(b, e):
        _check(lib.list_voxenc_forward_steps(occ.data_ptr(), B, R, arr, n, packed.blob.data_ptr(),
                                             packed.blob.numel(), ws.data_ptr(), ws.numel(), outs, b, e,
                                             hip._stream()), "list_voxenc_forward_steps")
    with torch.cuda.device(occ.device):
        return stage.time_launches(run, n_steps, reps)


def forward(module, occ):
    """VoxelEncoder2.forward in HIP for an eval-mode module on a HIP device.  Raises -- and never falls back to the
    torch module -- when the module is in training mode (batch-statistics BN is not implemented) or when autograd
    would record the call (there is no HIP backward of the encoder yet)."""
    stage.refuse_training_and_grad("vox_encoder", "encoder", [module], [occ])
    return encode(occ, pack(module))


# ---- host restatement ------------------------------------------------------------------------------------------------
def _conv3(x, w):
    """x float64 [B,Dz,Dy,Dx,Cin], w float64 [Cout,Cin,3,3,3] -> float64 [B,Dz,Dy,Dx,Cout]: 3x3x3 cross-correlation,
    zero padding 1, accumulated in float64."""
    Dz, Dy, Dx = x.shape[1:4]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)))
    wt = np.ascontiguousarray(w.transpose(2, 3, 4, 1, 0))    # [3,3,3,Cin,Cout]: contiguous taps, or the GEMM crawls
    out = np.zeros(x.shape[:4] + (w.shape[0],), dtype=np.float64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                out += xp[:, kz:kz + Dz, ky:ky + Dy, kx:kx + Dx, :] @ wt[kz, ky, kx]
    return out


def _pool(x):
    B, D, _, _, Cc = x.shape
    v = x.reshape(B, D // 2, 2, D // 2, 2, D // 2, 2, Cc)
    return v.max(axis=(2, 4, 6))


def encode_cpu(occ, params, storage="fp16", start=None, stop_after=None):
    """numpy restatement of the encoder.  occ: [B,R,R,R]; params: params_of(module).  Returns the six levels as
    [B,C,D,D,D] arrays (float32 level 0; float16 levels 1 .. 5 under storage="fp16", float64 under "exact").

    storage="fp16" states the device arithmetic: fp32 weights for the one-channel layers, fp16-rounded weights and
    activations where the device has them, sums in float64 rounded once to float32, the epilogue (bias, ReLU, BN
    scale and shift, sigmoid) in float32, then the rounding to fp16.  storage="exact": float64 throughout.

    start=(l, act): begin at stage l >= 4 from the pooled activation act [B,C,D,D,D] of stage l - 1 (the levels
    before are returned as None).  stop_after=l: return after stage l (later levels None; with l = 3 the grid may
    be a crop of any size: nothing is pooled)."""
    if storage not in ("fp16", "exact"):
        raise ValueError(f"storage = {storage!r}: 'fp16' or 'exact'")
    exact = storage == "exact"
    layers, eps, st = params["layers"], params["eps"], params["state"]
    f32 = np.float32

    def weight(name, half):
        w = np.asarray(st[name])
        if exact:
            return w.astype(np.float64)
        w = w.astype(f32)
        return (w.astype(np.float16) if half else w).astype(np.float64)

    def affine(l):
        return stage.bn_affine(st[f"bn.{l}.weight"], st[f"bn.{l}.bias"], st[f"bn.{l}.running_mean"],
                               st[f"bn.{l}.running_var"], eps[l], exact)

    def conv(x, name, half):
        z = _conv3(x.astype(np.float64), weight(f"conv.{name}.weight", half))
        if exact:
            return z + np.asarray(st[f"conv.{name}.bias"]).astype(np.float64)
        return z.astype(f32) + np.asarray(st[f"conv.{name}.bias"]).astype(f32)

    def relu(z):
        return np.where(z < 0, z.dtype.type(0), z)           # (a NaN stays a NaN)

    def bn(z, l):
        s, t = affine(l)
        return z * s + t                                     # float32: two roundings, as on the device

    def store(z):
        return z if exact else z.astype(np.float16)

    levels = [None] * N_LEVELS
    with np.errstate(over="ignore", invalid="ignore"):
        if start is None:
            net = np.asarray(occ)[..., None].astype(np.float64 if exact else f32)
            for l in range(2):
                net = bn(relu(conv(net, f"conv_{l}", False)), l)
            z = conv(net, "conv_2", False).astype(np.float64)
            net = 1.0 / (1.0 + np.exp(-z))
            net = net if exact else net.astype(f32)
            levels[0] = np.moveaxis(net, 4, 1)
            first = 3
        else:
            first, act = start
            net = np.moveaxis(np.asarray(act), 1, 4)
        for l in range(first, N_STAGES):
            net = store(relu(conv(net, f"conv_{l}", layers[l] != 1)))
            net = store(bn(relu(conv(net, f"conv_{l}_0", True)), l))
            levels[l - 2] = np.moveaxis(net, 4, 1)
            if stop_after is not None and l >= stop_after:
                break
            if l < N_STAGES - 1:
                net = _pool(net)
    return levels
