"""Stage 2's loss (LIST: the weighted binary cross-entropy of the occupancy head and the reference's SDFLoss) with its
gradients, what network.executors.LIST.calc_loss writes as torch expressions.

The device functions run through liblist_hip.so (include/list_s2loss.h) on the tensors' device: the forward reads the
occupancy volume and its target once, the backward reads them once more and writes one gradient; float64 sums in a fixed
order and no float atomics, so two runs give the same bits.  Every `*_cpu` function is the header's contract restated
in numpy float64: the test oracle.

  * stage2_loss(occ, occ_gt, sdf_pred, sdf_gt, sdf_scale, w=0.9) -> {'occ_loss', 'sdf_loss', 'ignore_sdf_loss_realvalue',
                                                                     'ignore_sdf_accuracy'}, a torch.autograd.Function
  * stage2_loss_cpu / stage2_grad_cpu                             the same values and gradients in numpy
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import hip

S2LOSS_EXPORTS = {
    "list_s2loss_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "list_s2loss_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_s2loss_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "list_s2loss_log": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "list_s2loss_last_error": (C.c_char_p, []),
}
KIND_F32, KIND_U8 = 0, 1    # list_s2loss.h: occ_gt_kind
KEYS = ("occ_loss", "sdf_loss", "ignore_sdf_loss_realvalue", "ignore_sdf_accuracy")
OCC_GROUPS, SDF_GROUPS = 1024, 64     # list_s2loss.h: workgroups of the occupancy sums and of the SDF sums
IN_FLIGHT = 4                         # s2loss_kernels.hip (kUnroll): items a lane loads before it uses the first


def grid_elements(groups=OCC_GROUPS):
    """Elements the fixed grid of `groups` workgroups covers with one item per lane (256 lanes, items of four)."""
    return groups * 256 * 4


def sweep_elements(groups=OCC_GROUPS):
    """Elements of one sweep of the forward's main loop: IN_FLIGHT items per lane.  A sum of fewer elements than this is
    taken by the one-item-at-a-time loop behind it alone."""
    return IN_FLIGHT * grid_elements(groups)


_section = hip.Section(S2LOSS_EXPORTS, "list_s2loss_last_error")    # include/list_s2loss.h on hip.load()'s handle
load, _check = _section.load, _section.check


def _sdf_dims(sdf_pred):
    """SDFLoss sums over the last axis and averages over the others: [B, N] with B the product of the leading axes."""
    n = sdf_pred.shape[-1] if sdf_pred.dim() else 1
    return sdf_pred.numel() // max(n, 1), n


class _Stage2LossFn(torch.autograd.Function):
    """(occ, occ_gt, sdf_pred, sdf_gt: contiguous device tensors of the header's dtypes) -> out float32 [4]."""

    @staticmethod
    def forward(ctx, occ, occ_gt, sdf_pred, sdf_gt, sdf_scale, w):
        lib = load()
        dev = occ.device
        B, N = _sdf_dims(sdf_pred)
        kind = KIND_F32 if occ_gt.dtype == torch.float32 else KIND_U8
        out = torch.empty((4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = _section.workspace(dev, lib.list_s2loss_workspace_bytes(occ.numel(), B, N), "list_s2loss_workspace_bytes")
            _check(lib.list_s2loss_fwd(occ.data_ptr(), occ_gt.data_ptr(), kind, occ.numel(), sdf_pred.data_ptr(),
                                       sdf_gt.data_ptr(), B, N, sdf_scale, w, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       hip._stream()), "list_s2loss_fwd")
        ctx.save_for_backward(occ, occ_gt, sdf_pred, sdf_gt)
        ctx.consts = (kind, B, N, sdf_scale, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        want_occ, want_sdf = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if not (want_occ or want_sdf):
            return None, None, None, None, None, None
        occ, occ_gt, sdf_pred, sdf_gt = ctx.saved_tensors
        kind, B, N, sdf_scale, w = ctx.consts
        lib = load()
        g = grad_out.detach().to(device=occ.device, dtype=torch.float32).contiguous()
        g_occ = torch.empty_like(occ) if want_occ else None
        g_sdf = torch.empty_like(sdf_pred) if want_sdf else None
        with torch.cuda.device(occ.device):
            _check(lib.list_s2loss_bwd(occ.data_ptr(), occ_gt.data_ptr(), kind, occ.numel(), sdf_pred.data_ptr(),
                                       sdf_gt.data_ptr(), B, N, sdf_scale, w, g.data_ptr(),
                                       g_occ.data_ptr() if want_occ else None, g_sdf.data_ptr() if want_sdf else None,
                                       hip._stream()), "list_s2loss_bwd")
        return g_occ, None, g_sdf, None, None, None


def _validate(occ, occ_gt, sdf_pred, sdf_gt):
    for name, t in (("occ", occ), ("occ_gt", occ_gt), ("sdf_pred", sdf_pred), ("sdf_gt", sdf_gt)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor (got {type(t).__name__})")
    if occ.numel() == 0 or occ.numel() != occ_gt.numel():
        raise ValueError(f"occ {tuple(occ.shape)} and occ_gt {tuple(occ_gt.shape)} must hold the same, non-zero, number "
                         "of elements")
    if sdf_pred.numel() == 0 or sdf_pred.shape != sdf_gt.shape:
        raise ValueError(f"sdf_pred {tuple(sdf_pred.shape)} and sdf_gt {tuple(sdf_gt.shape)} must be of one non-empty shape")
    if not occ.is_floating_point() or not sdf_pred.is_floating_point():
        raise ValueError(f"occ and sdf_pred must be floating point (got {occ.dtype}, {sdf_pred.dtype})")
    for name, t in (("occ_gt", occ_gt), ("sdf_pred", sdf_pred), ("sdf_gt", sdf_gt)):
        if t.device != occ.device:
            raise ValueError(f"occ is on {occ.device} and {name} on {t.device}: all four tensors must be on one device")


def _as_f32(t):
    return t.to(torch.float32).contiguous()


def stage2_loss(occ, occ_gt, sdf_pred, sdf_gt, sdf_scale, w=0.9):
    """The local terms of LIST.calc_loss on the GPU -> the reference's dict:
      occ_loss                   1000 * (-w * mean(occ_gt * log(occ + 1e-8)) - (1 - w) * mean((1 - occ_gt) * log(1 - occ + 1e-8)))
      sdf_loss                   SDFLoss: squared error summed over the points, averaged over the batch
      ignore_sdf_loss_realvalue  1e4 * mean squared error of the unscaled values
      ignore_sdf_accuracy        fraction of points on the same side of 0.5
    0-dim float32 tensors.  Gradients flow to occ and sdf_pred through occ_loss and sdf_loss; the two `ignore_` values
    carry no graph (requires_grad is False: they are reported, never trained on), and no gradient reaches occ_gt or sdf_gt.

    occ [any shape] and sdf_pred [..., N] are read as float32 (other float dtypes and non-contiguous tensors are
    converted; the gradients come back in the inputs' own dtype and layout through torch).  occ_gt may be float32, uint8 or
    bool and is read where it lies; any other dtype is converted to float32.  CPU tensors raise: stage2_loss_cpu is the
    numpy form, the executor's torch expressions the torch one."""
    _validate(occ, occ_gt, sdf_pred, sdf_gt)
    if not occ.is_cuda:
        raise ValueError(f"stage2_loss runs on the GPU (got tensors on {occ.device}); stage2_loss_cpu is the numpy form")
    if occ_gt.dtype == torch.bool:
        occ_gt = occ_gt.contiguous().view(torch.uint8)
    elif occ_gt.dtype in (torch.float32, torch.uint8):
        occ_gt = occ_gt.contiguous()
    else:
        occ_gt = _as_f32(occ_gt)
    out = _Stage2LossFn.apply(_as_f32(occ), occ_gt.detach(), _as_f32(sdf_pred), _as_f32(sdf_gt.detach()),
                              float(sdf_scale), float(w))
    return {KEYS[0]: out[0], KEYS[1]: out[1], KEYS[2]: out[2].detach(), KEYS[3]: out[3].detach()}


def device_log(x):
    """Diagnostic (list_s2loss_log): the forward's float64 logarithm of a float32 device tensor, as the device computes
    it -> float64 tensor of x's shape."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0):
        raise ValueError("device_log takes a non-empty float32 tensor on the GPU")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(load().list_s2loss_log(x.data_ptr(), x.numel(), out.data_ptr(), hip._stream()), "list_s2loss_log")
    return out


# ---- numpy restatement of include/list_s2loss.h ---------------------------------------------------------------------------
def _inputs_cpu(occ, occ_gt, sdf_pred, sdf_gt):
    """occ and sdf_pred keep their float32 or float64 (anything else becomes float32); targets widen exactly."""
    def keep(a):
        a = np.asarray(a)
        return a if a.dtype in (np.float32, np.float64) else a.astype(np.float32)
    occ, sdf_pred = keep(occ).reshape(-1), keep(sdf_pred)
    t = np.asarray(occ_gt).reshape(-1).astype(np.float64)
    if t.size != occ.size or occ.size == 0:
        raise ValueError(f"occ holds {occ.size} elements and occ_gt {t.size}")
    sdf_gt = keep(sdf_gt)
    if sdf_gt.shape != sdf_pred.shape or sdf_pred.size == 0:
        raise ValueError(f"sdf_pred {sdf_pred.shape} and sdf_gt {sdf_gt.shape} must be of one non-empty shape")
    N = sdf_pred.shape[-1] if sdf_pred.ndim else 1
    return occ, t, sdf_pred.reshape(-1), sdf_gt.reshape(-1), sdf_pred.size // N, N


def _log_args(occ):
    """a = occ + 1e-8 and b = (1 - occ) + 1e-8 in occ's own precision, as torch forms them -> float64."""
    one, eps = occ.dtype.type(1.0), occ.dtype.type(1e-8)
    return (occ + eps).astype(np.float64), ((one - occ) + eps).astype(np.float64)


def _device_consts(sdf_scale, w, device):
    """The constants as the library receives them (float32 arguments) when restating a device call."""
    return (float(np.float32(sdf_scale)), float(np.float32(w))) if device else (float(sdf_scale), float(w))


def stage2_loss_cpu(occ, occ_gt, sdf_pred, sdf_gt, sdf_scale, w=0.9, device=False):
    """The four values of list_s2loss_fwd in numpy -> dict of float64 (before the final rounding to float32).  occ and
    sdf_pred may be float32 (the device's case) or float64 (then the logarithms' arguments are formed in float64, which
    is what the torch expressions do on float64 tensors); sdf_scale and w are used as given.  device=True restates a
    call of the library: sdf_scale and w rounded to float32 as its arguments are, the values rounded to float32."""
    occ, t, p, sg, B, N = _inputs_cpu(occ, occ_gt, sdf_pred, sdf_gt)
    s, w = _device_consts(sdf_scale, w, device)
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = _log_args(occ)
        n = float(occ.size)
        s1, s0 = float(np.sum(t * np.log(a))), float(np.sum((1.0 - t) * np.log(b)))
        p64, t64 = p.astype(np.float64), sg.astype(np.float64)
        d, q = t64 * s - p64, t64 - p64 / s
        same = int(np.count_nonzero((sg > 0.5) == (p > 0.5)))
        out = {KEYS[0]: 1000.0 * (-w * s1 / n - (1.0 - w) * s0 / n), KEYS[1]: float(np.sum(d * d)) / B,
               KEYS[2]: 1e4 * float(np.sum(q * q)) / (B * N), KEYS[3]: same / float(B * N)}
    return {k: (np.float32(v) if device else np.float64(v)) for k, v in out.items()}


def stage2_grad_cpu(occ, occ_gt, sdf_pred, sdf_gt, sdf_scale, w=0.9, grad_out=(1.0, 1.0), device=False):
    """The gradients of list_s2loss_bwd in numpy -> (grad_occ, grad_sdf_pred) float64 in the inputs' shapes, for the
    upstream gradients grad_out = (g0 of occ_loss, g1 of sdf_loss).  device=True as in stage2_loss_cpu (g0 and g1 rounded
    to float32 as well, the gradients float32)."""
    shape_occ, shape_sdf = np.shape(occ), np.shape(sdf_pred)
    occ, t, p, sg, B, N = _inputs_cpu(occ, occ_gt, sdf_pred, sdf_gt)
    s, w = _device_consts(sdf_scale, w, device)
    g0, g1 = (float(np.float32(g)) for g in grad_out) if device else (float(g) for g in grad_out)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b = _log_args(occ)
        g_occ = (g0 * (1000.0 / float(occ.size))) * ((-w * t) / a + ((1.0 - w) * (1.0 - t)) / b)
        g_sdf = (g1 * (-2.0 / B)) * (sg.astype(np.float64) * s - p.astype(np.float64))
        if device:
            g_occ, g_sdf = g_occ.astype(np.float32), g_sdf.astype(np.float32)
    return g_occ.reshape(shape_occ), g_sdf.reshape(shape_sdf)
