#!/usr/bin/env python3
"""Time the training-image augmentation (not part of bench.py) per batch of 8 images of 224 x 224: the host path
(augment.jitter_pil + ToTensor per image with Pillow, one thread, as a loader worker runs it) against the device path
(the uint8 batch copied to the GPU and flipped, jittered and converted there in one launch, augment.apply), and the
host-to-device copy of the batch as float32 and as uint8.  Prints one JSON line.

    python tools/augment_bench.py [--rounds 20] [--inner 5] [--warmup 3] [--out augment_bench.json]

Every round takes `inner` samples of each measurement in turn, so that a drift of the machine falls on all of them alike;
a figure is the median over rounds x inner samples with its 10th and 90th percentile.  Device times are HIP events around
whole calls (Python, the copy of the 8 parameter records and the launch included); the host path is a host clock.  The
kernel's byte floor is what it has to move (3 bytes in, 12 out per pixel) over the 6.3 TB/s a streaming kernel reaches on
the MI355X: at this size it is far below the cost of a launch.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats`."""
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


def measure(B, S, rounds, inner, warmup):
    from list_amd import augment as A
    rng = np.random.default_rng(B * S)
    images = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8))
    as_float = images.permute(0, 3, 1, 2).float().div(255).contiguous()
    on_device = images.to(DEV)
    jitter = A.draw_params(B, True, True, torch.Generator().manual_seed(1))
    plain = A.identity_params(B)

    def host_path():
        torch.stack([A.to_tensor(A.jitter_pil(images[i].numpy(), jitter[i:i + 1])) for i in range(B)])

    runs = {
        "host_jitter_pil_to_tensor": (clock_ms, host_path),
        "device_copy_u8_and_jitter": (event_ms, lambda: A.apply(images.to(DEV), jitter)),
        "device_copy_u8_and_jitter_channels_last": (event_ms, lambda: A.apply(images.to(DEV), jitter, channels_last=True)),
        "device_copy_u8_and_to_tensor_only": (event_ms, lambda: A.apply(images.to(DEV), plain)),
        "device_jitter_alone": (event_ms, lambda: A.apply(on_device, jitter)),
        "device_to_tensor_alone": (event_ms, lambda: A.apply(on_device, plain)),
        "copy_float32": (event_ms, lambda: as_float.to(DEV)),
        "copy_uint8": (event_ms, lambda: images.to(DEV)),
    }
    for _, fn in runs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (timer, fn) in runs.items():
            samples[k] += [timer(fn) for _ in range(inner)]
    r = {"B": B, "H": S, "W": S, "bytes_in": images.numel(), "bytes_out": 4 * images.numel(),
         "kernel_byte_floor_ms": round(5 * images.numel() / HBM_BYTES_PER_S * 1e3, 5)}
    r.update({k: summary(v) for k, v in samples.items()})
    want = torch.from_numpy(A.apply_cpu(images.numpy(), jitter))
    r["bit_equal_to_apply_cpu"] = bool(torch.equal(A.apply(on_device, jitter).cpu(), want))
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench.py measures on the GPU: no device found")
    import __graft_entry__ as ge
    ge.build()
    torch.set_num_threads(1)
    result = {"device": torch.cuda.get_device_name(0), "batch": measure(8, 224, args.rounds, args.inner, args.warmup)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
