#!/usr/bin/env python3
"""Time the training-data preparation (not part of bench.py): prepare.signed_distance and prepare.farthest_points on
the device against their numpy restatements.

    python tools/prep_bench.py [--points 150000] [--iters 5] [--out prep_bench.json]

Meshes: marching-cubes spheres of about 10k, 100k and 500k faces.  Signed distance of --points query points (3 sigmas
x 50k, the default of a shape), reported as point x face pairs per second; the numpy path runs on a subset of the
points on the smallest mesh.  Farthest point sampling 50k -> 5k for B = 1 and B = 32 clouds; the numpy path for B = 1.
Device times are CUDA events around whole calls, median of --iters after warm-up.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch        # noqa: E402

from mesh_bench import sphere, time_device  # noqa: E402

MESH_RES = (48, 150, 330)        # about 10k, 100k and 500k faces


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cpu-points", type=int, default=2000)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy path")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from list_amd import mesh as M
    from list_amd import prepare as P
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "Q": args.points, "sdf": [], "fps": []}
    rng = np.random.default_rng(0)
    q = torch.from_numpy(rng.uniform(-0.5, 0.5, (args.points, 3)).astype(np.float32)).to(dev)
    for res in MESH_RES:
        v, f = M.marching_cubes(torch.from_numpy(sphere(res, 0.35)).to(dev))
        F = int(f.shape[0])
        med, best, _ = time_device(lambda: P.signed_distance(v, f, q), args.iters, warmup=2)
        r = {"F": F, "ms_median": round(med, 3), "ms_min": round(best, 3),
             "gpairs_per_s": round(args.points * F / (med * 1e-3) / 1e9, 1)}
        if not args.no_cpu and res == MESH_RES[0]:
            vh, fh, qh = v.cpu().numpy(), f.cpu().numpy(), q[:args.cpu_points].cpu().numpy()
            t = time.perf_counter()
            P.signed_distance_cpu(vh, fh, qh)
            dt = time.perf_counter() - t
            r["cpu_mpairs_per_s"] = round(args.cpu_points * F / dt / 1e6, 2)
        result["sdf"].append(r)
        print("sdf", json.dumps(r), flush=True)
    for B in (1, 32):
        c = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 50000, 3)).astype(np.float32)).to(dev)
        med, best, _ = time_device(lambda: P.farthest_points(c, 5000), args.iters, warmup=1)
        r = {"B": B, "N": 50000, "K": 5000, "ms_median": round(med, 3), "ms_min": round(best, 3)}
        if not args.no_cpu and B == 1:
            t = time.perf_counter()
            _, idx = P.farthest_points_cpu(c.cpu().numpy(), 5000)
            r["cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            r["cpu_idx_equal"] = bool(np.array_equal(idx, P.farthest_points(c, 5000)[1].cpu().numpy()))
        result["fps"].append(r)
        print("fps", json.dumps(r), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
