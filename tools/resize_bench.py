#!/usr/bin/env python3
"""Time the Pix3D image path (not part of bench.py) per batch of 8 generated images of Pix3D-like sizes (SIZES below, H x W
from 224 x 224 to 3024 x 4032) brought to 224 x 224: the host path (flip + augment.jitter_pil + resize.resize_pil +
ToTensor per image with Pillow, one thread, as a loader worker runs it) against the device path (the raw images packed into
one uint8 buffer, copied to the GPU and flipped, jittered, resized and converted there in two launches, resize.apply), and
both host-to-device copies: the packed raw batch, and the resized float32 batch the host path would ship.  Prints one JSON
line.

    python tools/resize_bench.py [--rounds 10] [--inner 3] [--warmup 2] [--out resize_bench.json]

Every round takes `inner` samples of each device measurement and one of each host measurement in turn, so that a drift of
the machine falls on all of them alike; a figure is the median over its samples with the 10th and 90th percentile.  Device
times are HIP events around whole calls (Python, the plan made on the host, the copies of the plan and of the 8 parameter
records and the two launches included); host times are a host clock.  The kernels' byte floor is what they have to move
(every source byte in once, the intermediate out and in, 12 bytes out per output pixel) over the 6.3 TB/s a streaming
kernel reaches on the MI355X.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402
import torch        # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
SIZES = ((480, 640), (768, 1024), (1200, 1600), (2000, 3000), (3024, 4032), (375, 500), (1080, 1920), (224, 224))     # H x W
OUT = 224


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def clock_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
            "p90_ms": round(float(np.percentile(ms, 90)), 4), "samples": len(ms)}


def measure(rounds, inner, warmup):
    from list_amd import augment as A, resize as R
    rng = np.random.default_rng(8)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    B = len(images)
    jitter = A.draw_params(B, True, True, torch.Generator().manual_seed(1))
    packed = R.RaggedImages.pack(images)
    on_device = packed.to(DEV)

    def host_path(params=jitter):
        return torch.stack([A.to_tensor(R.resize_pil(A.jitter_pil(images[i], params[i:i + 1]), OUT)) for i in range(B)])

    def host_resize_only():
        return torch.stack([A.to_tensor(R.resize_pil(images[i], OUT)) for i in range(B)])

    as_float = host_path()
    host_runs = {
        "host_flip_jitter_resize_to_tensor": host_path,
        "host_resize_to_tensor_only": host_resize_only,
        "host_pack_uint8": lambda: R.RaggedImages.pack(images),
    }
    device_runs = {
        "device_copy_packed_and_jitter_resize": lambda: R.apply(packed.to(DEV), OUT, OUT, jitter),
        "device_copy_packed_and_jitter_resize_channels_last": lambda: R.apply(packed.to(DEV), OUT, OUT, jitter, channels_last=True),
        "device_copy_packed_and_resize_only": lambda: R.apply(packed.to(DEV), OUT, OUT),
        "device_jitter_resize_alone": lambda: R.apply(on_device, OUT, OUT, jitter),
        "device_resize_alone": lambda: R.apply(on_device, OUT, OUT),
        "copy_packed_uint8": lambda: packed.to(DEV),
        "copy_resized_float32": lambda: as_float.to(DEV),
    }
    for fn in device_runs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in list(host_runs) + list(device_runs)}
    for _ in range(rounds):
        for k, fn in host_runs.items():
            samples[k].append(clock_ms(fn))
        for k, fn in device_runs.items():
            samples[k] += [event_ms(fn) for _ in range(inner)]
    rec = packed.records()
    mid = R.load().list_resize_workspace_bytes(rec.ctypes.data, B, OUT, OUT)
    moved = packed.data.numel() + 2 * mid + 12 * B * OUT * OUT
    r = {"B": B, "sizes_hw": [list(s) for s in SIZES], "out": OUT, "bytes_packed_uint8": packed.data.numel(),
         "bytes_resized_float32": 12 * B * OUT * OUT, "bytes_intermediate": int(mid), "plan_bytes": int(R.plan(packed, OUT, OUT).size),
         "kernels_byte_floor_ms": round(moved / HBM_BYTES_PER_S * 1e3, 5)}
    r.update({k: summary(v) for k, v in samples.items()})
    r["bit_equal_to_the_pillow_host_path"] = bool(torch.equal(R.apply(on_device, OUT, OUT, jitter).cpu(), as_float))
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resize_bench.py measures on the GPU: no device found")
    import __graft_entry__ as ge
    ge.build()
    torch.set_num_threads(1)
    result = {"device": torch.cuda.get_device_name(0), "batch": measure(args.rounds, args.inner, args.warmup)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
