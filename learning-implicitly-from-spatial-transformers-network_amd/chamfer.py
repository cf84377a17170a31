"""Chamfer distance of stage 1 (CoarseNet's loss: the predicted coarse cloud against the farthest-point cloud of the
ground truth), what the reference takes from pytorch3d.loss.chamfer_distance with its default arguments
(point_reduction="mean", batch_reduction="mean", norm=2), with its gradient.

The device functions run through liblist_hip.so (include/list_loss.h) on the tensors' device: brute-force nearest
neighbours in both directions without the B x N x M distance matrix, a float64 loss in a fixed order, and a backward
that gathers the sources of every point through a stable counting sort -- no float atomics, so two runs give the same
bits.  Every `*_cpu` function is the header's contract restated in numpy: the test oracle.

  * nearest_sq(x, y)        -> (d2_xy, idx_xy, d2_yx, idx_yx): squared distance to, and index of, the nearest point of
                               the other cloud (smallest index on ties).
  * chamfer_distance(x, y)  -> (loss, None) like pytorch3d; a torch.autograd.Function on the GPU, the existing torch
                               path (network.executors.chamfer_distance) on CPU tensors.
"""
import ctypes as C

import numpy as np
import torch

from . import hip

LOSS_EXPORTS = {
    "list_chamfer_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "list_chamfer_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_chamfer_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_loss_last_error": (C.c_char_p, []),
}
SERIAL_MAX = 32             # list_loss.h: a target with more sources than this is summed by a whole wave
_RED_LANES = 256            # list_loss.h: lanes of the per-batch float64 sum

_section = hip.Section(LOSS_EXPORTS, "list_loss_last_error")    # include/list_loss.h on hip.load()'s handle
load, _check = _section.load, _section.check


def _validate(x, y):
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise ValueError(f"x and y must be tensors (got {type(x).__name__}, {type(y).__name__})")
    if x.dim() != 3 or y.dim() != 3 or x.shape[-1] != 3 or y.shape[-1] != 3:
        raise ValueError(f"x and y must be [B,N,3] and [B,M,3] (got {tuple(x.shape)} and {tuple(y.shape)})")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"x and y hold {x.shape[0]} and {y.shape[0]} clouds: the batch sizes must match")
    if x.shape[0] == 0 or x.shape[1] == 0 or y.shape[1] == 0:
        raise ValueError(f"empty cloud: x {tuple(x.shape)}, y {tuple(y.shape)}")
    if x.device != y.device:
        raise ValueError(f"x is on {x.device} and y on {y.device}: both clouds must be on one device")
    if not x.is_floating_point() or not y.is_floating_point():
        raise ValueError(f"x and y must be floating point (got {x.dtype}, {y.dtype})")


def _fwd(x, y):
    """x, y: float32 contiguous device tensors -> (loss [], d2_xy, idx_xy, d2_yx, idx_yx)."""
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    dev = x.device
    lib = load()
    d2_xy = torch.empty((B, N), dtype=torch.float32, device=dev)
    idx_xy = torch.empty((B, N), dtype=torch.int32, device=dev)
    d2_yx = torch.empty((B, M), dtype=torch.float32, device=dev)
    idx_yx = torch.empty((B, M), dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_chamfer_workspace_bytes(B, N, M), "list_chamfer_workspace_bytes")
        _check(lib.list_chamfer_fwd(x.data_ptr(), y.data_ptr(), B, N, M, d2_xy.data_ptr(), idx_xy.data_ptr(),
                                    d2_yx.data_ptr(), idx_yx.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                    hip._stream()), "list_chamfer_fwd")
    return loss, d2_xy, idx_xy, d2_yx, idx_yx


def _bwd(x, y, idx_xy, idx_yx, grad_loss, want_x, want_y):
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    dev = x.device
    lib = load()
    g = grad_loss.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous()
    gx = torch.empty_like(x) if want_x else None
    gy = torch.empty_like(y) if want_y else None
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_chamfer_workspace_bytes(B, N, M), "list_chamfer_workspace_bytes")
        _check(lib.list_chamfer_bwd(x.data_ptr(), y.data_ptr(), B, N, M, idx_xy.data_ptr(), idx_yx.data_ptr(),
                                    g.data_ptr(), gx.data_ptr() if want_x else None,
                                    gy.data_ptr() if want_y else None, ws.data_ptr(), ws.numel(), hip._stream()),
               "list_chamfer_bwd")
    return gx, gy


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        loss, _, idx_xy, _, idx_yx = _fwd(x, y)
        ctx.save_for_backward(x, y, idx_xy, idx_yx)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_y):
            return None, None
        x, y, idx_xy, idx_yx = ctx.saved_tensors
        return _bwd(x, y, idx_xy, idx_yx, grad_loss, want_x, want_y)


def _as_f32(t):
    return t.to(torch.float32).contiguous()


def nearest_sq(x, y):
    """Nearest neighbours in both directions of x [B,N,3] and y [B,M,3] on the device -> (d2_xy float32 [B,N],
    idx_xy int32 [B,N], d2_yx float32 [B,M], idx_yx int32 [B,M]).  No gradient."""
    _validate(x, y)
    if not x.is_cuda:
        raise ValueError(f"nearest_sq runs on the GPU (got tensors on {x.device}); nearest_sq_cpu is the numpy form")
    with torch.no_grad():
        _, d2_xy, idx_xy, d2_yx, idx_yx = _fwd(_as_f32(x), _as_f32(y))
    return d2_xy, idx_xy, d2_yx, idx_yx


def chamfer_distance(x, y):
    """Symmetric mean squared nearest-neighbour distance of x [B,N,3] and y [B,M,3] -> (loss, None), as
    pytorch3d.loss.chamfer_distance(x, y) returns it.  On the GPU the HIP loss of include/list_loss.h (float32
    arithmetic; other float dtypes are converted, and the loss and gradients come back in x's dtype); on CPU tensors
    the torch path of network.executors.chamfer_distance."""
    _validate(x, y)
    if not x.is_cuda:
        from .network.executors import chamfer_distance as torch_path
        return torch_path(x, y)
    loss = _ChamferFn.apply(_as_f32(x), _as_f32(y))
    return loss.to(x.dtype), None


# ---- numpy restatement of include/list_loss.h -----------------------------------------------------------------------------
def _clouds_cpu(x, y):
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    if x.ndim != 3 or y.ndim != 3 or x.shape[-1] != 3 or y.shape[-1] != 3 or x.shape[0] != y.shape[0]:
        raise ValueError(f"x and y must be [B,N,3] and [B,M,3] (got {x.shape} and {y.shape})")
    return x, y


def nearest_sq_cpu(x, y, rows=512):
    """nearest_sq in numpy, bit for bit: d2 = (dx*dx + dy*dy) + dz*dz in float32, smallest index on ties, a NaN pair
    never the minimum, +inf and index 0 when nothing is below +inf, NaN for a point with a NaN coordinate."""
    x, y = _clouds_cpu(x, y)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    d2_xy = np.empty((B, N), np.float32)
    idx_xy = np.empty((B, N), np.int32)
    d2_yx = np.full((B, M), np.inf, np.float32)
    idx_yx = np.zeros((B, M), np.int32)
    for b in range(B):
        for i0 in range(0, N, rows):
            xs = x[b, i0:i0 + rows]
            dx = xs[:, None, 0] - y[b][None, :, 0]
            dy = xs[:, None, 1] - y[b][None, :, 1]
            dz = xs[:, None, 2] - y[b][None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            d[np.isnan(d)] = np.inf
            k = np.argmin(d, axis=1)
            d2_xy[b, i0:i0 + len(xs)] = d[np.arange(len(xs)), k]
            idx_xy[b, i0:i0 + len(xs)] = k
            kc = np.argmin(d, axis=0)                           # first minimum in this block of rows
            vc = d[kc, np.arange(M)]
            better = vc < d2_yx[b]                              # strict: an earlier block keeps a tie
            d2_yx[b][better] = vc[better]
            idx_yx[b][better] = (kc + i0)[better]
        d2_xy[b][np.isnan(x[b]).any(axis=1)] = np.nan
        d2_yx[b][np.isnan(y[b]).any(axis=1)] = np.nan
    return d2_xy, idx_xy, d2_yx, idx_yx


def _sum_in_order(d2):
    """The header's float64 sum of one batch's d2: 256 lanes in turn, then the fixed fold."""
    v = np.asarray(d2, dtype=np.float64)
    v = np.concatenate([v, np.zeros((-len(v)) % _RED_LANES)]).reshape(-1, _RED_LANES)
    p = np.zeros(_RED_LANES)
    for row in v:
        p = p + row
    w = _RED_LANES // 2
    while w:
        p[:w] = p[:w] + p[w:2 * w]
        w //= 2
    return float(p[0])


def chamfer_distance_cpu(x, y, nearest=None):
    """The loss of list_chamfer_fwd in numpy (float32 result of the float64 sums in the header's order)."""
    x, y = _clouds_cpu(x, y)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    d2_xy, _, d2_yx, _ = nearest if nearest is not None else nearest_sq_cpu(x, y)
    lx = ly = 0.0
    for b in range(B):
        lx += _sum_in_order(d2_xy[b]) / N
    for b in range(B):
        ly += _sum_in_order(d2_yx[b]) / M
    return np.float32(lx / B + ly / B)


def chamfer_grad_cpu(x, y, grad_loss=1.0, nearest=None):
    """The gradients of list_chamfer_bwd in numpy -> (grad_x float32 [B,N,3], grad_y float32 [B,M,3]): float64
    differences of the coordinates, the reverse sums in source-index order."""
    x, y = _clouds_cpu(x, y)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    _, idx_xy, _, idx_yx = nearest if nearest is not None else nearest_sq_cpu(x, y)
    g = float(np.float32(grad_loss))
    kx, ky = g * (2.0 / (B * N)), g * (2.0 / (B * M))
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    gx = np.empty((B, N, 3), np.float32)
    gy = np.empty((B, M, 3), np.float32)
    for b in range(B):
        ixy, iyx = idx_xy[b].astype(np.int64), idx_yx[b].astype(np.int64)
        sx = np.zeros((N, 3))
        np.add.at(sx, iyx, x64[b][iyx] - y64[b])
        sy = np.zeros((M, 3))
        np.add.at(sy, ixy, y64[b][ixy] - x64[b])
        gx[b] = (kx * (x64[b] - y64[b][ixy]) + ky * sx).astype(np.float32)
        gy[b] = (ky * (y64[b] - x64[b][iyx]) + kx * sy).astype(np.float32)
    return gx, gy
