#!/usr/bin/env python3
"""Time the mesh evaluation (not part of bench.py): evaluate.eval_mesh on the device and its numpy restatement, and each
of the three device operations alone (nn_distance, sample_surface, mesh_contains).

    python tools/eval_bench.py [--res 256] [--n-points 100000] [--iters 10] [--out eval_bench.json]

Two pairs: a res^3 marching-cubes sphere against a slightly larger sphere, and the predict_grid mesh of the LIST model
(seeded weights) against a sphere.  Device times are CUDA events around whole calls, median of --iters after warm-up
(eval_mesh includes its uploads, its synchronisations and the Python between the launches).  The CPU path runs once.
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
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

from mesh_bench import predicted_volume, sphere, time_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--n-points", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy path")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from list_amd import evaluate as E
    from list_amd import mesh as M
    dev = "cuda:0"
    n = args.n_points
    gt = M.Mesh(*M.marching_cubes(torch.from_numpy(sphere(args.res, 0.32)).to(dev)))
    preds = {"sphere": M.Mesh(*M.marching_cubes(torch.from_numpy(sphere(args.res)).to(dev))),
             "predict_grid": M.Mesh(*M.marching_cubes(predicted_volume(args.res, dev)))}
    result = {"res": args.res, "n_points": n, "device": torch.cuda.get_device_name(0),
              "gt": {"V": len(gt.vertices), "F": len(gt.faces)}, "pairs": {}}
    for name, pred in preds.items():
        r = {"V": len(pred.vertices), "F": len(pred.faces)}
        med, best, score = time_device(lambda: E.eval_mesh(pred, gt, -0.5, 0.5, n, device=dev), args.iters, warmup=2)
        r.update(eval_mesh_ms_median=round(med, 3), eval_mesh_ms_min=round(best, 3), score=score)
        vt, ft = torch.from_numpy(pred.vertices).to(dev), torch.from_numpy(pred.faces).to(dev)
        pc, _ = E.sample_surface(vt, ft, n)
        pc2, _ = E.sample_surface(torch.from_numpy(gt.vertices).to(dev), torch.from_numpy(gt.faces).to(dev), n, 1)
        q = E.box_samples(10 * n, -0.5, 0.5, 2, dev)
        r["sample_ms"] = round(time_device(lambda: E.sample_surface(vt, ft, n), args.iters)[0], 3)
        r["nn_ms"] = round(time_device(lambda: E.nn_distance(pc, pc2), args.iters)[0], 3)
        r["contains_ms"] = round(time_device(lambda: E.mesh_contains(vt, ft, q), args.iters)[0], 3)
        r["waterproofing_ms"] = round(time_device(lambda: E.implicit_waterproofing(vt, ft, q), args.iters)[0], 3)
        if not args.no_cpu:
            t = time.perf_counter()
            cpu = E.eval_mesh_cpu(pred, gt, -0.5, 0.5, n)
            r["cpu_eval_mesh_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            r["cpu_iou_equal"] = cpu.get("iou") == score.get("iou")
        result["pairs"][name] = r
        print(name, json.dumps(r), flush=True)
    # the inside test at scale: 1M points against a 1M-triangle mesh
    big = M.marching_cubes(torch.from_numpy(sphere(512, 0.45)).to(dev))
    nb = big[1].shape[0]
    q = E.box_samples(1_000_000, -0.5, 0.5, 3, dev)
    result["contains_1M_points"] = {"F": int(nb),
                                    "ms": round(time_device(lambda: E.mesh_contains(*big, q), args.iters)[0], 3)}
    a, b = E.box_samples(100_000, -0.5, 0.5, 4, dev).float(), E.box_samples(100_000, -0.5, 0.5, 5, dev).float()
    result["nn_100k_x_100k_ms"] = round(time_device(lambda: E.nn_distance(a, b), args.iters)[0], 3)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
