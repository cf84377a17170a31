#!/usr/bin/env python3
"""Time the mesh rasteriser (not part of bench.py): render.rasterize_device and render.shade on marching-cubes meshes,
with mesh.marching_cubes of the same volume beside them for scale.

    python tools/render_bench.py [--res 256 128] [--size 224 512] [--iters 30] [--out render_bench.json]

Volumes: tools/components_bench.py's two spheres plus a few dozen small blobs, at each --res.  Cameras: the LIST camera of
a synthetic trans_mat (synthetic.make_trans_mat) and the orthographic view along axis 0.  Times are HIP events around
whole calls after warm-up, median of --iters: the whole rasterize call, shade, and the call cut off after each of its four
launches (list_render_rasterize's step range: clear, + setup and small faces, + large faces, + resolve).  A call is a few
tens of microseconds of host work around kernels of 2 - 14 microseconds, so the cut-off calls show where the CALL's time
goes, not the kernels': for those run this under `rocprofv3 --kernel-trace --stats`.  The byte floor beside them is what
the rasteriser has to move -- 12 V + 12 F bytes of mesh read, 8 H W bytes of keys cleared and 8 H W resolved -- over the
6.3 TB/s a streaming kernel reaches on the MI355X."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch        # noqa: E402

from components_bench import spheres_and_blobs  # noqa: E402
from mesh_bench import time_device              # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def bench_view(v, f, cam, size, iters):
    from list_amd import render as R
    through = {}
    for end in range(1, R.N_STEPS + 1):
        ms = time_device(lambda: R.rasterize_device(v, f, cam, size, size, steps=(0, end)), iters)[0]
        through[f"call_through_{R.STEP_NAMES[end - 1]}_ms"] = round(ms, 4)
    total, best, (face_id, _, stats) = time_device(lambda: R.rasterize_device(v, f, cam, size, size), iters)
    shade_ms = time_device(lambda: R.shade(v, f, face_id, cam, "lambert"), iters)[0]
    V, F = len(v), len(f)
    out = dict(through)
    out.update(rasterize_ms_median=round(total, 4), rasterize_ms_min=round(best, 4), shade_ms=round(shade_ms, 4),
               stats=dict(zip(R.STATS, stats.tolist())), covered_pixels=int((face_id >= 0).sum()),
               floor_bytes={"mesh_read": 12 * V + 12 * F, "keys_cleared": 8 * size * size, "keys_resolved": 8 * size * size},
               byte_floor_ms=round((12 * V + 12 * F + 16 * size * size) / HBM_BYTES_PER_S * 1e3, 5))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--size", type=int, nargs="+", default=[224, 512])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from list_amd import mesh, render as R, synthetic
    dev = "cuda:0"
    cameras = {"list": lambda s: R.Camera.from_transmat(synthetic.make_trans_mat(7, 1)[0]),
               "ortho_axis0": lambda s: R.Camera.orthographic(0, s, s)}
    result = {"device": torch.cuda.get_device_name(0), "cap": R.CAP, "large_groups": R.LARGE_GROUPS, "meshes": {}}
    for res in args.res:
        vol = torch.from_numpy(spheres_and_blobs(res)).to(dev)
        mc_ms, _, (v, f) = time_device(lambda: mesh.marching_cubes(vol), args.iters)
        r = {"V": len(v), "F": len(f), "marching_cubes_ms": round(mc_ms, 4), "views": {}}
        for size in args.size:
            for name, make in cameras.items():
                r["views"][f"{name}_{size}"] = bench_view(v, f, make(size), size, args.iters)
                print(res, f"{name}_{size}", json.dumps(r["views"][f"{name}_{size}"]), flush=True)
        result["meshes"][f"spheres_and_blobs_{res}"] = r
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
