"""Ragged-batch image resize: the reference's Pix3D transform T.Resize((224, 224)) behind the flip and the colour jitter and
ahead of T.ToTensor() (datasets/Datasets.py:330-344), for images of different sizes, without torchvision.

On a PIL image T.Resize is Image.resize(size, BILINEAR): an antialiased, separable filter in 22-bit fixed point.
include/list_resize.h restates it so that every byte equals Pillow's; this module holds the forms of it:

  * apply(ragged, out_h, out_w, params, channels_last)   the device form through liblist_hip.so: a RaggedImages on the GPU ->
                                                         float32 [B,3,out_h,out_w], two launches per batch (--augment hip)
  * apply_cpu(ragged, out_h, out_w, params)              the header restated in numpy: the test oracle, and what CPU
                                                         tensors take
  * coeffs_cpu(n_in, n_out), resize_cpu(image, h, w)     the axis tables and one image uint8 -> uint8 in numpy
  * resize_pil(image, size)                              Pillow's own Image.resize: the host path of the Pix3D dataset
  * plan(ragged, out_h, out_w), host(image, h, w)        list_resize_plan's buffer and list_resize_host, for tests and tools

The flip and the colour steps are augment.py's (PARAMS records, one per image) and act on the source pixels.
"""
import ctypes as C

import numpy as np
import torch

from . import augment, hip

RESIZE_EXPORTS = {
    "list_resize_plan_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    "list_resize_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    "list_resize_plan": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]),
    "list_resize_fwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_resize_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]),
    "list_resize_last_error": (C.c_char_p, []),
}
MAX_SIDE, MAX_BATCH = 16384, 65535
PRECISION_BITS = 22
COPY, HORIZONTAL, VERTICAL = 0, 1, 2                    # what a stage does
# ListResizeImage (16 bytes), ListResizePlanHeader (40), ListResizePlanImage (80)
IMAGE = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4")])
PLAN_HEADER = np.dtype([("plan_bytes", "<i8"), ("workspace_bytes", "<i8"), ("src_bytes", "<i8"), ("magic", "<i4"),
                        ("B", "<i4"), ("out_h", "<i4"), ("out_w", "<i4")])
PLAN_IMAGE = np.dtype([("src_offset", "<i8"), ("mid_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("mid_h", "<i4"),
                       ("mid_w", "<i4"), ("stage", "<i4", (2,)), ("ksize", "<i4", (2,)), ("bounds", "<i8", (2,)),
                       ("weights", "<i8", (2,))])
assert (IMAGE.itemsize, PLAN_HEADER.itemsize, PLAN_IMAGE.itemsize) == (16, 40, 80)

_section = hip.Section(RESIZE_EXPORTS, "list_resize_last_error")      # include/list_resize.h on hip.load()'s handle
load, _check = _section.load, _section.check


# ---- a batch of images of different sizes -------------------------------------------------------------------------------------
class RaggedImages:
    """uint8 images [H_i,W_i,3] packed into one 1-D uint8 tensor `data` (which may live on the device), with the int64
    table `sizes` [B,2] = (H, W) and the int64 byte offsets `offsets` [B] of the images in `data` (both on the host, where
    the plan is made; the offsets are the dense packing's unless given)."""

    def __init__(self, data, sizes, offsets=None):
        sizes = torch.as_tensor(sizes, dtype=torch.int64).reshape(-1, 2).cpu()
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError("RaggedImages takes a 1-D uint8 tensor of packed pixels")
        if len(sizes) < 1 or int(sizes.min()) < 1:
            raise ValueError(f"RaggedImages takes at least one image and sides >= 1 (got sizes {sizes.tolist()})")
        extents = 3 * sizes[:, 0] * sizes[:, 1]
        if offsets is None:
            offsets = torch.cumsum(extents, 0) - extents
        offsets = torch.as_tensor(offsets, dtype=torch.int64).reshape(-1).cpu()
        if offsets.shape != extents.shape or int(offsets.min()) < 0 or int((offsets + extents).max()) > data.numel():
            raise ValueError(f"RaggedImages: offsets {offsets.tolist()} with sizes {sizes.tolist()} do not lie inside the "
                             f"{data.numel()} packed bytes")
        self.data, self.sizes, self.offsets = data, sizes, offsets

    @classmethod
    def pack(cls, images):
        """A list of uint8 [H,W,3] arrays or tensors, densely packed in their order."""
        arrays = [np.ascontiguousarray(im.numpy() if isinstance(im, torch.Tensor) else im) for im in images]
        for a in arrays:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
                raise ValueError(f"pack takes non-empty uint8 images [H,W,3] (got {a.dtype} {a.shape})")
        if not arrays:
            raise ValueError("pack takes at least one image")
        data = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays]))
        return cls(data, [a.shape[:2] for a in arrays])

    def to(self, device, non_blocking=False):
        return RaggedImages(self.data.to(device, non_blocking=non_blocking), self.sizes, self.offsets)

    def pin_memory(self):
        return RaggedImages(self.data.pin_memory(), self.sizes, self.offsets)

    def __len__(self):
        return int(self.sizes.shape[0])

    @property
    def device(self):
        return self.data.device

    def image(self, i):
        """Image i as a uint8 [H,W,3] view of the packed tensor."""
        (h, w), o = self.sizes[i].tolist(), int(self.offsets[i])
        return self.data[o:o + 3 * h * w].view(h, w, 3)

    def records(self):
        """ListResizeImage [B]."""
        r = np.zeros(len(self), IMAGE)
        r["offset"], r["H"], r["W"] = self.offsets.numpy(), self.sizes[:, 0].numpy(), self.sizes[:, 1].numpy()
        return r


# ---- numpy restatement of include/list_resize.h -------------------------------------------------------------------------------
def coeffs_cpu(n_in, n_out):
    """The tables of the axis n_in -> n_out: bounds int32 [n_out,2] = (xmin, xmax) and the fixed-point weights int32
    [n_out,ksize], zero beyond xmax.  float64, every operation rounded on its own, as Pillow's precompute_coeffs and
    normalize_coeffs_8bpc."""
    n_in, n_out = int(n_in), int(n_out)
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support = np.float64(1.0) * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = np.float64(1.0) / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                   # (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None]
    t = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((x < xmax[:, None]) & (t < 1.0), 1.0 - t, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                     # summed in ascending x (np.sum adds pairwise)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(ww != 0.0, w / ww, w)
    K = np.where(k < 0.0, -0.5 + k * float(1 << PRECISION_BITS), 0.5 + k * float(1 << PRECISION_BITS)).astype(np.int32)
    assert (255 * K.astype(np.int64).sum(1) + (1 << (PRECISION_BITS - 1)) < 1 << 31).all()
    return np.stack([xmin, xmax], 1).astype(np.int32), K


def stages_cpu(H, W, out_h, out_w):
    """The two stages of H x W -> out_h x out_w and the intermediate's size: ((stage0, stage1), (mid_h, mid_w))."""
    need_h, need_v = W != out_w, H != out_h
    if need_h and need_v:
        stages = (VERTICAL, HORIZONTAL) if H > 100 * W and out_h < H else (HORIZONTAL, VERTICAL)
    else:
        stages = (HORIZONTAL if need_h else VERTICAL if need_v else COPY, COPY)
    mid = {HORIZONTAL: (H, out_w), VERTICAL: (out_h, W), COPY: (H, W)}[stages[0]]
    return stages, mid


def _pass_cpu(image, n_out, axis):
    """One pass along `axis` (0 vertical, 1 horizontal) of uint8 [H,W,C] -> uint8."""
    n_in = image.shape[axis]
    bounds, K = coeffs_cpu(n_in, n_out)
    a = np.moveaxis(image, axis, 0).astype(np.int64)                                # [n_in, other, C]
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    step = max(1, (1 << 22) // max(1, K.shape[1] * a[0].size))
    for s in range(0, n_out, step):
        idx = np.minimum(bounds[s:s + step, :1].astype(np.int64) + np.arange(K.shape[1]), n_in - 1)     # weights are 0 past xmax
        acc = (1 << (PRECISION_BITS - 1)) + (a[idx] * K[s:s + step, :, None, None].astype(np.int64)).sum(1)
        assert int(acc.max()) < 1 << 31
        out[s:s + step] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_cpu(image_u8, out_h, out_w):
    """Image.resize((out_w, out_h), BILINEAR) of a uint8 [H,W,C] array in numpy -> uint8 [out_h,out_w,C]."""
    image = np.asarray(image_u8)
    if image.dtype != np.uint8 or image.ndim != 3 or image.size == 0 or out_h < 1 or out_w < 1:
        raise ValueError(f"resize_cpu takes a non-empty uint8 array [H,W,C] and sizes >= 1 (got {image.dtype} {image.shape} "
                         f"-> {out_h} x {out_w})")
    stages, _ = stages_cpu(image.shape[0], image.shape[1], int(out_h), int(out_w))
    for stage in stages:
        if stage == HORIZONTAL:
            image = _pass_cpu(image, int(out_w), 1)
        elif stage == VERTICAL:
            image = _pass_cpu(image, int(out_h), 0)
    return np.array(image, copy=True) if stages == (COPY, COPY) else image


def _check_call(ragged, out_h, out_w):
    if not isinstance(ragged, RaggedImages):
        raise ValueError(f"expected a RaggedImages (got {type(ragged).__name__})")
    if not (1 <= int(out_h) <= MAX_SIDE and 1 <= int(out_w) <= MAX_SIDE) or len(ragged) > MAX_BATCH \
            or int(ragged.sizes.max()) > MAX_SIDE:
        raise ValueError(f"sides and target sizes are 1 ... {MAX_SIDE}, a batch at most {MAX_BATCH} images (got "
                         f"{len(ragged)} images up to {int(ragged.sizes.max())} -> {out_h} x {out_w})")
    return int(out_h), int(out_w)


def apply_cpu(ragged, out_h, out_w, params=None):
    """list_resize_fwd in numpy: per image the flip, the colour steps, the resize and ToTensor -> float32
    [B,3,out_h,out_w] (C-contiguous)."""
    out_h, out_w = _check_call(ragged, out_h, out_w)
    p = augment._records(params, len(ragged))
    out = np.empty((len(ragged), 3, out_h, out_w), np.float32)
    for i, r in enumerate(p):
        x = ragged.image(i).cpu().numpy()
        if int(r["ops"]) & augment.FLIP:
            x = x[:, ::-1]
        if int(r["ops"]) & augment.JITTER:
            x = augment.colour_cpu(x, r).astype(np.uint8)
        y = resize_cpu(np.ascontiguousarray(x), out_h, out_w)
        out[i] = (y.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    return out


# ---- the library's forms ------------------------------------------------------------------------------------------------------
def _aligned_bytes(n):
    """A writable uint8 array of n bytes on an 8-byte boundary."""
    return np.zeros((n + 7) // 8, np.int64).view(np.uint8)[:n]


def plan(ragged, out_h, out_w):
    """list_resize_plan: the host plan buffer (uint8, 8-byte aligned) of the batch for the target size."""
    out_h, out_w = _check_call(ragged, out_h, out_w)
    lib, rec = load(), ragged.records()
    need = _section.sized(lib.list_resize_plan_bytes(rec.ctypes.data, len(rec), out_h, out_w), "list_resize_plan_bytes")
    buf = _aligned_bytes(need)
    _check(lib.list_resize_plan(rec.ctypes.data, len(rec), ragged.data.numel(), out_h, out_w, buf.ctypes.data, need),
           "list_resize_plan")
    return buf


def parse_plan(buf):
    """A plan buffer as (header record, image records [B], tables(i, s) -> (bounds [n_out,2], weights [n_out,ksize]) or
    None for a copy)."""
    head = buf[:PLAN_HEADER.itemsize].view(PLAN_HEADER)[0]
    B = int(head["B"])
    images = buf[PLAN_HEADER.itemsize:PLAN_HEADER.itemsize + B * PLAN_IMAGE.itemsize].view(PLAN_IMAGE)

    def tables(i, s):
        r = images[i]
        if r["stage"][s] == COPY:
            return None
        ksize, lo, hi = int(r["ksize"][s]), int(r["bounds"][s]), int(r["weights"][s])
        n_out = (hi - lo) // 8
        return (buf[lo:hi].view(np.int32).reshape(n_out, 2), buf[hi:hi + 4 * n_out * ksize].view(np.int32).reshape(n_out, ksize))

    return head, images, tables


def host(image_u8, out_h, out_w):
    """list_resize_host: one uint8 [H,W,3] image through csrc/resize_math.h as the host compiles it -> uint8
    [out_h,out_w,3]."""
    image = np.ascontiguousarray(image_u8)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"host takes a uint8 array [H,W,3] (got {image.dtype} {image.shape})")
    out = np.empty((int(out_h), int(out_w), 3), np.uint8)
    _check(load().list_resize_host(image.ctypes.data, image.shape[0], image.shape[1], out.ctypes.data, int(out_h), int(out_w)),
           "list_resize_host")
    return out


def apply(ragged, out_h, out_w, params=None, channels_last=False):
    """A RaggedImages -> float32 [B,3,out_h,out_w] on the images' device: per image the flip and the colour steps of
    `params` (augment.PARAMS records, one per image; None is the plain resize) on the source pixels, Pillow's bilinear
    resize, ToTensor.  channels_last=True returns the same logical tensor in torch.channels_last memory format.  On the GPU
    this is list_resize_fwd (two launches); CPU tensors take apply_cpu."""
    out_h, out_w = _check_call(ragged, out_h, out_w)
    B = len(ragged)
    p = None if params is None else augment._records(params, B)
    if not ragged.data.is_cuda:
        out = apply_cpu(ragged, out_h, out_w, p)
        if channels_last:
            return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
        return torch.from_numpy(out)
    src, dev = ragged.data.contiguous(), ragged.data.device
    lib, rec = load(), ragged.records()
    buf = plan(ragged, out_h, out_w)
    need = _section.sized(lib.list_resize_workspace_bytes(rec.ctypes.data, B, out_h, out_w), "list_resize_workspace_bytes")
    if channels_last:       # [B,H,W,3] in memory (strides as torch.channels_last gives them, size-1 axes included)
        out = torch.empty((B, out_h, out_w, 3), dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    else:
        out = torch.empty((B, 3, out_h, out_w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = hip._workspace(dev, need)
        plan_dev = torch.from_numpy(buf).to(dev)
        p_dev = None if p is None else torch.from_numpy(p.view(np.uint8).reshape(B, augment.PARAMS.itemsize)).to(dev)
        _check(lib.list_resize_fwd(src.data_ptr(), src.numel(), buf.ctypes.data, plan_dev.data_ptr(), buf.size,
                                   None if p is None else p.ctypes.data, None if p is None else p_dev.data_ptr(),
                                   out.data_ptr(), int(bool(channels_last)), ws.data_ptr(), ws.numel(), hip._stream()),
               "list_resize_fwd")
    return out


# ---- the host path: Pillow's own resize ---------------------------------------------------------------------------------------
def resize_pil(image, size):
    """Image.resize(size, BILINEAR) of a PIL image or a uint8 [H,W,3] array -> PIL image; `size` is (width, height), or
    one int for a square."""
    from PIL import Image
    img = image if isinstance(image, Image.Image) else Image.fromarray(np.ascontiguousarray(image, np.uint8))
    size = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    return img.resize(size, Image.Resampling.BILINEAR)
