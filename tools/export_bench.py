#!/usr/bin/env python3
"""Time the .obj export (not part of bench.py): utils.write_obj's Python loop -- what Mesh.export ran for every mesh before
objtext.py -- against objtext.write_obj on the device, the device route split into its parts.

    python tools/export_bench.py [--res 128 256] [--repeats 5] [--field predict_grid] [--out export_bench.json]

Meshes: marching cubes of a predict_grid volume of the LIST model with seeded weights (tools/mesh_bench.py's) and of two
spheres plus a few dozen small blobs (tools/components_bench.py's), the ones tools/simplify_bench.py times.  One repeat
runs, in this order, the Python loop into a temporary directory (wall clock, the host copy of the tensors included, as
Mesh.__init__ makes it), objtext.write_obj into the same directory (wall clock, synchronised), then the parts of the
device route on their own: list_objtext_count with its scan and list_objtext_emit (HIP events), the device-to-host copy
and the file write (wall clock).  The repeats interleave the routes; every figure is the median of the repeats, after
one warm-up of the device route.  The loop is slow, so --loop-repeats caps how often it runs (its median is over those).
No time is a pass/fail condition; the two files are compared byte for byte."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch        # noqa: E402

from components_bench import spheres_and_blobs   # noqa: E402
from mesh_bench import predicted_volume          # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def parts(v, f, directory):
    """One run of the device route, part by part -> dict of ms."""
    from list_amd import hip, objtext as O
    lib = O.load()
    V, F, dev = len(v), len(f), v.device
    need = lib.list_objtext_workspace_bytes(V, F)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    vp, fp, st = v.data_ptr(), f.data_ptr(), hip._stream()
    out = {"count_ms": event_ms(lambda: O._check(lib.list_objtext_count(vp, fp, V, F, ws.data_ptr(), need, totals.data_ptr(), st),
                                                  "list_objtext_count"))}
    n = int(totals.tolist()[0])
    text = torch.empty((n,), dtype=torch.uint8, device=dev)
    out["emit_ms"] = event_ms(lambda: O._check(lib.list_objtext_emit(vp, fp, V, F, ws.data_ptr(), need, text.data_ptr(), n, st),
                                               "list_objtext_emit"))
    out["copy_ms"], host = wall_ms(lambda: text.cpu().numpy())

    def write():
        with open(os.path.join(directory, "parts.obj"), "wb") as fh:
            fh.write(memoryview(host))

    out["file_write_ms"] = wall_ms(write)[0]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--field", default="predict_grid", choices=["all", "spheres_and_blobs", "predict_grid"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from list_amd import mesh, objtext as O, utils
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "runs": []}
    for res in args.res:
        volumes = {}
        if args.field in ("all", "spheres_and_blobs"):
            volumes["spheres_and_blobs"] = torch.from_numpy(spheres_and_blobs(res)).to(dev)
        if args.field in ("all", "predict_grid"):
            volumes["predict_grid"] = predicted_volume(res, dev)
        for name, vol in volumes.items():
            v, f = mesh.marching_cubes(vol)
            with tempfile.TemporaryDirectory() as d:
                a, b = os.path.join(d, "loop.obj"), os.path.join(d, "device.obj")
                O.write_obj(b, v, f)                                     # warm-up: workspace, library, page cache
                loop, device, split = [], [], []
                for r in range(args.repeats):
                    if r < args.loop_repeats:
                        loop.append(wall_ms(lambda: utils.write_obj(a, v.cpu().numpy(), f.cpu().numpy()))[0])
                    device.append(wall_ms(lambda: O.write_obj(b, v, f))[0])
                    split.append(parts(v, f, d))
                same = open(a, "rb").read() == open(b, "rb").read()
                run = {"field": name, "res": res, "V": len(v), "F": len(f), "obj_bytes": os.path.getsize(b),
                       "same_bytes": same, "python_loop_ms": round(float(np.median(loop)), 1),
                       "python_loop_us_per_line": round(float(np.median(loop)) * 1e3 / max(len(v) + len(f), 1), 3),
                       "device_route_ms": round(float(np.median(device)), 3)}
                run.update({k: round(float(np.median([s[k] for s in split])), 4) for k in split[0]})
                run["speedup"] = round(run["python_loop_ms"] / run["device_route_ms"], 1)
            result["runs"].append(run)
            print(json.dumps(run), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
