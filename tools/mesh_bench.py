#!/usr/bin/env python3
"""Time mesh extraction (not part of bench.py): mesh.marching_cubes on the device, mesh.marching_cubes_cpu, and
PyMCubes where it is installed, on a 256^3 sphere and on a predict_grid volume of the LIST model (seeded weights).

    python tools/mesh_bench.py [--res 256] [--iters 50] [--out mesh_bench.json]

Device times are CUDA events around whole marching_cubes calls (count kernel, scan, totals read-back -- the one host
synchronisation --, allocation, emit kernel), median of --iters after warm-up.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch        # noqa: E402


def sphere(n, r=0.3):
    a = np.linspace(-0.5, 0.5, n)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return (r - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def predicted_volume(res, dev):
    from oracle import fill, synth
    from list_amd import arguments, utils
    from list_amd.train import _Module
    cfg = arguments.default_config(vox_res=32, train_batch_size=1, mcube_znum=res)
    cfg.device = torch.device(dev)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(dev)
    ex = utils.get_class("network.executors.LIST")(cfg, _Module(net))
    img = torch.from_numpy(synth.uniform(78, (1, 3, 64, 64))).to(dev)
    vol, _, _ = ex.predict_grid(img)
    # seeded weights give no particular shape: the field is moved to its median so that a surface crosses the grid
    return (vol - vol.median()).contiguous()


def time_device(fn, iters, warmup=5):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), out


def time_host(fn, iters=3):
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from list_amd import mesh
    dev = "cuda:0"
    try:
        import mcubes
    except ImportError:
        mcubes = None
    volumes = {"sphere": torch.from_numpy(sphere(args.res)).to(dev), "predict_grid": predicted_volume(args.res, dev)}
    result = {"res": args.res, "device": torch.cuda.get_device_name(0), "fields": {}}
    for name, vol in volumes.items():
        med, best, (v, f) = time_device(lambda: mesh.marching_cubes(vol), args.iters)
        host = vol.cpu().numpy()
        cpu_ms, (cv, cf) = time_host(lambda: mesh.marching_cubes_cpu(host))
        same = v.shape == cv.shape and f.shape == cf.shape and bool(np.array_equal(f.cpu().numpy(), cf)) and \
            float(np.abs(v.cpu().numpy() - cv).max(initial=0.0)) <= 1e-6
        r = {"V": int(v.shape[0]), "F": int(f.shape[0]), "gpu_call_ms_median": round(med, 4),
             "gpu_call_ms_min": round(best, 4), "cpu_numpy_ms": round(cpu_ms, 1), "gpu_equals_cpu": same,
             "volume_read_GBps": round(vol.numel() * 4 / (med * 1e-3) / 1e9, 1)}
        if mcubes is not None:
            r["mcubes_ms"] = round(time_host(lambda: mcubes.marching_cubes(-host, 0.0))[0], 1)
        else:
            r["mcubes_ms"] = "not installed"
        result["fields"][name] = r
        print(name, json.dumps(r), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
