"""Training-image augmentation: the reference's T.RandomHorizontalFlip(0.5) and T.ColorJitter(brightness=0.3,
saturation=0.5, hue=0.5) followed by T.ToTensor() (datasets/Datasets.py:24-38,161-174), without torchvision.

On PIL images ColorJitter is three Pillow operations in a random order, each from uint8 RGB to uint8 RGB.
include/list_augment.h restates them so that every byte equals Pillow's; this module holds the three forms of it:

  * apply(images_u8, params, channels_last)   the device form through liblist_hip.so: uint8 [B,H,W,3] on the GPU ->
                                              float32 [B,3,H,W], one launch per batch (--augment hip)
  * apply_cpu(images_u8, params)              the header restated in numpy: the test oracle, and what CPU tensors take
  * jitter_pil(image, params)                 the same parameters applied with Pillow's own ImageEnhance /
                                              convert("HSV"): the host path of the datasets (--augment host)

Parameters are records of PARAMS (the C ABI's ListAugmentParams), one per image: draw_params draws a batch of them from a
torch.Generator with torchvision's get_params distribution, draw_jitter one from a Python or numpy random state.  The
draws are not the reference's, which come from unseeded worker state.

The hue step's shift is this project's definition: shift = trunc(hue * 255) mod 256 (hue_shift); torchvision's uint8
wrap-around add is not compared with.
"""
import ctypes as C

import numpy as np
import torch

from . import hip

AUGMENT_EXPORTS = {
    "list_augment_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "list_augment_pixel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "list_augment_last_error": (C.c_char_p, []),
}
FLIP, BRIGHTNESS, SATURATION, HUE = 1, 2, 4, 8          # list_augment.h: bits of ops
JITTER = BRIGHTNESS | SATURATION | HUE
SLOT_BRIGHTNESS, SLOT_CONTRAST, SLOT_SATURATION, SLOT_HUE = 0, 1, 2, 3      # values of an order slot; contrast is a no-op
BRIGHTNESS_RANGE, SATURATION_RANGE, HUE_RANGE = (0.7, 1.3), (0.5, 1.5), (-0.5, 0.5)
# ListAugmentParams, 32 bytes
PARAMS = np.dtype([("ops", "<i4"), ("order", "<i4", (4,)), ("brightness", "<f4"), ("saturation", "<f4"),
                   ("hue_shift", "<i4")])
assert PARAMS.itemsize == 32

_section = hip.Section(AUGMENT_EXPORTS, "list_augment_last_error")    # include/list_augment.h on hip.load()'s handle
load, _check = _section.load, _section.check


# ---- parameters -------------------------------------------------------------------------------------------------------------
def hue_shift(hue):
    """The hue step's shift for a hue factor in [-0.5, 0.5]: trunc(hue * 255) mod 256."""
    return int(float(hue) * 255.0) % 256


def identity_params(batch):
    """`batch` records that do nothing (plain ToTensor): ops 0, the identity order, factors 1 and shift 0."""
    p = np.zeros(int(batch), PARAMS)
    p["order"], p["brightness"], p["saturation"] = np.arange(4), 1.0, 1.0
    return p


def make_params(ops=0, order=(0, 1, 2, 3), brightness=1.0, saturation=1.0, shift=0):
    """One record from its fields (a 1-element PARAMS array)."""
    p = identity_params(1)
    p["ops"], p["order"], p["brightness"], p["saturation"], p["hue_shift"] = ops, order, brightness, saturation, shift
    return p


def draw_params(batch, flip, jitter, generator):
    """A batch of records from the CPU torch.Generator `generator`.  Per image, in this order: the flip coin
    (torch.rand(1) < 0.5, when `flip`), then when `jitter` torch.randperm(4) and the brightness, saturation and hue
    uniforms: torchvision's RandomHorizontalFlip and ColorJitter.get_params."""
    p = identity_params(batch)
    for i in range(int(batch)):
        ops = 0
        if flip and float(torch.rand(1, generator=generator)) < 0.5:
            ops |= FLIP
        if jitter:
            ops |= JITTER
            p["order"][i] = torch.randperm(4, generator=generator).numpy()
            b, s, h = (float(torch.empty(1).uniform_(lo, hi, generator=generator))
                       for lo, hi in (BRIGHTNESS_RANGE, SATURATION_RANGE, HUE_RANGE))
            p["brightness"][i], p["saturation"][i], p["hue_shift"][i] = b, s, hue_shift(h)
        p["ops"][i] = ops
    return p


def draw_jitter(rng):
    """One jitter record from `rng.random()` (the `random` module, a random.Random or a numpy RandomState), in the order
    of draw_params: the permutation (Fisher-Yates from the last slot down), then brightness, saturation and hue."""
    p = make_params(JITTER)
    order = [0, 1, 2, 3]
    for k in (3, 2, 1):
        j = int(rng.random() * (k + 1))
        order[k], order[j] = order[j], order[k]
    b, s, h = (lo + (hi - lo) * rng.random() for lo, hi in (BRIGHTNESS_RANGE, SATURATION_RANGE, HUE_RANGE))
    p["order"], p["brightness"], p["saturation"], p["hue_shift"] = order, b, s, hue_shift(h)
    return p


def _records(params, batch):
    """`params` as a C-contiguous PARAMS array of `batch` records, checked as list_augment_fwd checks them."""
    p = identity_params(batch) if params is None else np.ascontiguousarray(np.atleast_1d(params))
    if p.dtype != PARAMS or p.shape != (batch,):
        raise ValueError(f"params must be {batch} record(s) of augment.PARAMS (got {p.dtype} {p.shape})")
    for i, r in enumerate(p):
        ops = int(r["ops"])
        if ops & ~(FLIP | JITTER):
            raise ValueError(f"params[{i}].ops = {ops}: bits beyond flip | brightness | saturation | hue (15)")
        if sorted(int(k) for k in r["order"]) != [0, 1, 2, 3]:
            raise ValueError(f"params[{i}].order = {tuple(int(k) for k in r['order'])}: not a permutation of 0 ... 3")
        for bit, name, (lo, hi) in ((BRIGHTNESS, "brightness", BRIGHTNESS_RANGE), (SATURATION, "saturation", SATURATION_RANGE),
                                    (HUE, "hue_shift", (0, 255))):
            if ops & bit and not np.float32(lo) <= r[name] <= np.float32(hi):
                raise ValueError(f"params[{i}].{name} = {r[name]}: outside [{lo}, {hi}]")
    return p


# ---- the device form ----------------------------------------------------------------------------------------------------------
def apply(images_u8, params=None, channels_last=False):
    """uint8 [B,H,W,3] -> float32 [B,3,H,W] on the images' device: flip, colour steps and ToTensor per image as `params`
    (PARAMS records, one per image; None is plain ToTensor) says.  channels_last=True returns the same logical tensor in
    torch.channels_last memory format.  On the GPU this is one launch (list_augment_fwd); CPU tensors take apply_cpu."""
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 \
            or images_u8.shape[3] != 3 or images_u8.numel() == 0:
        raise ValueError("apply takes a non-empty uint8 tensor [B,H,W,3] (got "
                         f"{getattr(images_u8, 'dtype', type(images_u8).__name__)} {tuple(getattr(images_u8, 'shape', ()))})")
    B, H, W, _ = images_u8.shape
    p = _records(params, B)
    if not images_u8.is_cuda:
        out = apply_cpu(images_u8.numpy(), p)
        if channels_last:
            return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
        return torch.from_numpy(out)
    src, dev = images_u8.contiguous(), images_u8.device
    if channels_last:       # [B,H,W,3] in memory (strides as torch.channels_last gives them, size-1 axes included)
        out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    else:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    p_dev = torch.from_numpy(p.view(np.uint8).reshape(B, PARAMS.itemsize)).to(dev)
    with torch.cuda.device(dev):
        _check(load().list_augment_fwd(src.data_ptr(), out.data_ptr(), B, H, W, int(bool(channels_last)), p.ctypes.data,
                                       p_dev.data_ptr(), hip._stream()), "list_augment_fwd")
    return out


def pixel(rgb, params):
    """list_augment_pixel: one pixel through the colour steps of one record, as the host compiles csrc/augment_math.h ->
    (uint8 [3] levels, float32 [3] ToTensor values)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(3)
    p = np.ascontiguousarray(np.atleast_1d(params))
    if p.dtype != PARAMS or p.shape != (1,):
        raise ValueError("pixel takes one record of augment.PARAMS")
    levels, values = np.empty(3, np.uint8), np.empty(3, np.float32)
    _check(load().list_augment_pixel(rgb.ctypes.data, p.ctypes.data, levels.ctypes.data, values.ctypes.data),
           "list_augment_pixel")
    return levels, values


# ---- numpy restatement of include/list_augment.h ---------------------------------------------------------------------------
def _clip_trunc(t):
    """A blend's float32 values to levels: 0 below, 255 above, truncated between."""
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.int32)


def _brightness_cpu(x, f):
    return _clip_trunc(np.float32(f) * x.astype(np.float32))


def _saturation_cpu(x, f):
    L = (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16
    L = L[..., None]
    return _clip_trunc(L.astype(np.float32) + np.float32(f) * (x - L).astype(np.float32))


def _rgb_to_hsv_cpu(x):
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(-1), x.min(-1)
    grey = maxc == minc
    f32, f64 = np.float32, np.float64
    with np.errstate(invalid="ignore", divide="ignore"):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc.astype(f64) - gc.astype(f64),
                     np.where(g == maxc, 2.0 + rc.astype(f64) - bc.astype(f64), 4.0 + gc.astype(f64) - rc.astype(f64)))
        h = np.fmod(h.astype(f32).astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.clip((np.where(grey, 0.0, h).astype(f64) * 255.0).astype(np.int32), 0, 255)
        S = np.clip((np.where(grey, 0.0, s).astype(f64) * 255.0).astype(np.int32), 0, 255)
    return H, S, maxc


def _hsv_to_rgb_cpu(H, S, V):
    fh, fs, v = H.astype(np.float64) * 6.0 / 255.0, S.astype(np.float64) / 255.0, V.astype(np.float64)
    fl = np.floor(fh)
    f, i = fh - fl, fl.astype(np.int32) % 6
    level = lambda a: np.clip(np.rint(a).astype(np.int32), 0, 255)
    p, q, t = level(v * (1.0 - fs)), level(v * (1.0 - fs * f)), level(v * (1.0 - fs * (1.0 - f)))
    table = (((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)))
    out = np.stack([np.choose(i, [row[c] for row in table]) for c in range(3)], -1)
    return np.where((S == 0)[..., None], V[..., None], out).astype(np.int32)


def _hue_cpu(x, shift):
    H, S, V = _rgb_to_hsv_cpu(x)
    return _hsv_to_rgb_cpu((H + int(shift)) & 255, S, V)


def colour_cpu(image, record):
    """The colour steps of one record on int32 levels [..., 3] -> int32 levels."""
    x, ops = np.asarray(image).astype(np.int32), int(record["ops"])
    for slot in record["order"]:
        if slot == SLOT_BRIGHTNESS and ops & BRIGHTNESS:
            x = _brightness_cpu(x, record["brightness"])
        elif slot == SLOT_SATURATION and ops & SATURATION:
            x = _saturation_cpu(x, record["saturation"])
        elif slot == SLOT_HUE and ops & HUE:
            x = _hue_cpu(x, record["hue_shift"])
    return x


def apply_cpu(images_u8, params=None):
    """list_augment_fwd in numpy: uint8 [B,H,W,3] -> float32 [B,3,H,W] (C-contiguous)."""
    images = np.asarray(images_u8)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3 or images.size == 0:
        raise ValueError(f"apply_cpu takes a non-empty uint8 array [B,H,W,3] (got {images.dtype} {images.shape})")
    p = _records(params, images.shape[0])
    out = np.empty((images.shape[0], 3) + images.shape[1:3], np.float32)
    for i, r in enumerate(p):
        x = images[i, :, ::-1] if int(r["ops"]) & FLIP else images[i]
        out[i] = (colour_cpu(x, r).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    return out


# ---- the host path: Pillow's own operations ---------------------------------------------------------------------------------
def jitter_pil(image, params):
    """One record applied with Pillow: Image.transpose for the flip, ImageEnhance.Brightness / .Color and the HSV round
    trip for the colour steps, in the record's order.  `image` is a PIL image (converted to RGB) or a uint8 array
    [H,W,3] -> PIL RGB image."""
    from PIL import Image, ImageEnhance
    r = _records(params, 1)[0]
    img = image.convert("RGB") if isinstance(image, Image.Image) else Image.fromarray(np.ascontiguousarray(image, np.uint8))
    ops = int(r["ops"])
    if ops & FLIP:
        img = img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    for slot in r["order"]:
        if slot == SLOT_BRIGHTNESS and ops & BRIGHTNESS:
            img = ImageEnhance.Brightness(img).enhance(float(r["brightness"]))
        elif slot == SLOT_SATURATION and ops & SATURATION:
            img = ImageEnhance.Color(img).enhance(float(r["saturation"]))
        elif slot == SLOT_HUE and ops & HUE:
            h, s, v = img.convert("HSV").split()
            h = Image.fromarray(((np.asarray(h).astype(np.int32) + int(r["hue_shift"])) % 256).astype(np.uint8))
            img = Image.merge("HSV", (h, s, v)).convert("RGB")
    return img


def to_tensor(image):
    """T.ToTensor() of a PIL RGB image or uint8 [H,W,3] array -> float32 tensor [3,H,W], uint8 / 255."""
    a = np.asarray(image, dtype=np.float32) / np.float32(255.0)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
