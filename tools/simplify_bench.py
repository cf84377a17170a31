#!/usr/bin/env python3
"""Time the vertex-clustering simplifier (not part of bench.py): simplify.simplify on the device against the host route
-- copy the mesh to the host, simplify.simplify_cpu, copy the result back; the copies are part of that route's time --
with mesh.marching_cubes of the same volume beside them for scale, the faces in and out, and the bytes of the exported
.obj before and after.

    python tools/simplify_bench.py [--res 256 128] [--cells 64 128] [--iters 30] [--field all] [--out simplify_bench.json]

Two volumes: two spheres plus a few dozen small blobs (tools/components_bench.py's) and a predict_grid volume of the
LIST model with seeded weights (tools/mesh_bench.py's).  Device times are CUDA events around whole calls (the read-back
of the totals and the allocations included), median of --iters after warm-up; count and emit are timed the same way
through the C ABI.  No time is a pass/fail condition.  Per-kernel times: run this under `rocprofv3 --kernel-trace
--stats`, one --field at a time."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch        # noqa: E402

from components_bench import spheres_and_blobs                   # noqa: E402
from mesh_bench import predicted_volume, time_device, time_host  # noqa: E402


def host_route(v_dev, f_dev, cells):
    from list_amd import simplify as S
    v, f, _ = S.simplify_cpu(v_dev.cpu().numpy(), f_dev.cpu().numpy(), cells)
    return torch.from_numpy(v).to(v_dev.device), torch.from_numpy(f).to(v_dev.device)


def stages(v, f, cells, iters):
    """Median ms of list_simp_count and list_simp_emit on (v, f)."""
    from list_amd import hip, simplify as S
    lib = S.load()
    V, F, dev = len(v), len(f), v.device
    R, lo, inv, cell = S.grid(cells)
    cR, clo = (ctypes.c_int32 * 3)(*R.tolist()), (ctypes.c_double * 3)(*lo.tolist())
    cinv, ccell = (ctypes.c_double * 3)(*inv.tolist()), (ctypes.c_double * 3)(*cell.tolist())
    need = lib.list_simp_workspace_bytes(V, F, cR)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    vmap = torch.empty((V,), dtype=torch.int32, device=dev)
    totals = torch.empty((len(S.TOTALS),), dtype=torch.int64, device=dev)
    vp, fp, wp, st = v.data_ptr(), f.data_ptr(), ws.data_ptr(), hip._stream()

    def count():
        S._check(lib.list_simp_count(vp, fp, V, F, cR, clo, cinv, wp, need, vmap.data_ptr(), totals.data_ptr(), st),
                 "list_simp_count")

    out = {"workspace_MiB": round(need / 2 ** 20, 1), "count_ms": time_device(count, iters)[0]}
    Vo, Fo = totals.tolist()[:2]
    ov = torch.empty((Vo, 3), dtype=torch.float32, device=dev)
    of = torch.empty((Fo, 3), dtype=torch.int32, device=dev)
    out["emit_ms"] = time_device(lambda: S._check(lib.list_simp_emit(
        fp, V, F, cR, clo, ccell, vmap.data_ptr(), wp, need, ov.data_ptr(), Vo, of.data_ptr(), Fo, st), "list_simp_emit"),
        iters)[0]
    return {k: round(x, 4) for k, x in out.items()}


def obj_bytes(v, f):
    from list_amd import mesh
    with tempfile.TemporaryDirectory() as d:
        return os.path.getsize(mesh.Mesh(v, f).export(os.path.join(d, "m.obj")))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--cells", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--field", default="all", choices=["all", "spheres_and_blobs", "predict_grid"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from list_amd import mesh, simplify as S
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "runs": []}
    for res in args.res:
        volumes = {}
        if args.field in ("all", "spheres_and_blobs"):
            volumes["spheres_and_blobs"] = torch.from_numpy(spheres_and_blobs(res)).to(dev)
        if args.field in ("all", "predict_grid"):
            volumes["predict_grid"] = predicted_volume(res, dev)
        for name, vol in volumes.items():
            mc_ms, _, (v, f) = time_device(lambda: mesh.marching_cubes(vol), args.iters)
            full_obj = obj_bytes(v, f)
            for cells in args.cells:
                med, best, (sv, sf, info) = time_device(lambda: S.simplify(v, f, cells), args.iters)
                host_ms, (hv, hf) = time_host(lambda: host_route(v, f, cells))
                r = {"field": name, "res": res, "cells": cells, "V": len(v), "F": len(f), "V_out": len(sv), "F_out": len(sf),
                     "clusters": info["clusters"], "marching_cubes_ms": round(mc_ms, 4),
                     "simplify_ms_median": round(med, 4), "simplify_ms_min": round(best, 4),
                     "stages": stages(v, f, cells, args.iters), "host_route_ms": round(host_ms, 1),
                     "device_equals_host": bool(torch.equal(sf, hf)) and sv.cpu().numpy().tobytes() == hv.cpu().numpy().tobytes(),
                     "obj_bytes": full_obj, "obj_bytes_out": obj_bytes(sv, sf)}
                result["runs"].append(r)
                print(json.dumps(r), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
