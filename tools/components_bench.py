#!/usr/bin/env python3
"""Time the mesh-component filter (not part of bench.py): components.keep_components(keep=1) on the device against the
host route it replaces -- copy the mesh to the host, scipy.sparse.csgraph.connected_components, compact with numpy;
the copy is part of that route's time -- with mesh.marching_cubes of the same volume beside them for scale.

    python tools/components_bench.py [--res 256] [--iters 30] [--field all] [--out components_bench.json]

Two volumes: two spheres plus a few dozen small blobs, and a predict_grid volume of the LIST model with seeded weights
(tools/mesh_bench.py's).  Device times are CUDA events around whole calls (every read-back and allocation included),
median of --iters after warm-up; the stages (begin / rounds / finish / compact) are timed the same way through the C
ABI.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`, one --field at a time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch        # noqa: E402

from mesh_bench import predicted_volume, time_device, time_host  # noqa: E402


def spheres_and_blobs(n, n_blobs=40, seed=4):
    """float32 [n,n,n], positive inside: two spheres and n_blobs small ones scattered around them."""
    a = np.linspace(-0.5, 0.5, n, dtype=np.float32)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")

    def ball(c, r):
        return (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)

    v = np.maximum(ball((-0.2, -0.05, 0.0), 0.22), ball((0.25, 0.1, 0.05), 0.15))
    rng = np.random.default_rng(seed)
    for _ in range(n_blobs):
        v = np.maximum(v, ball(rng.uniform(-0.45, 0.45, 3), rng.uniform(0.008, 0.02)))
    return v


def host_route(v_dev, f_dev):
    """What a user does today: the mesh to the host, scipy's components, the largest one compacted with numpy."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    v, f = v_dev.cpu().numpy(), f_dev.cpu().numpy()
    V = len(v)
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(V, V)),
                                  directed=False)
    counts = np.bincount(lab[f[:, 0]], minlength=lab.max() + 1)
    best = counts.max()
    smallest = np.full(counts.size, V)
    np.minimum.at(smallest, lab, np.arange(V))
    top = min(np.flatnonzero(counts == best), key=lambda c: smallest[c])      # the tie rule: the lower label
    vkeep = lab == top
    vmap = np.cumsum(vkeep) - 1
    return v[vkeep], vmap[f[vkeep[f[:, 0]]]].astype(np.int32)


def stages(v, f, iters):
    """Median ms of each C-ABI stage on (v, f), and the rounds the labelling took."""
    from list_amd import components as C, hip
    lib = C.load()
    V, F, dev = len(v), len(f), v.device
    ws = torch.empty((lib.list_cc_workspace_bytes(V, F),), dtype=torch.uint8, device=dev)
    changed = torch.empty((C.ROUNDS_PER_READBACK,), dtype=torch.int32, device=dev)
    ids = torch.empty((V,), dtype=torch.int32, device=dev)
    table = torch.empty((3, V), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    fp, wp, wn, st = f.data_ptr(), ws.data_ptr(), ws.numel(), hip._stream()

    def begin():
        C._check(lib.list_cc_begin(fp, V, F, wp, wn, st), "list_cc_begin")

    def rounds():
        C._check(lib.list_cc_rounds(fp, V, F, wp, wn, 0, C.ROUNDS_PER_READBACK, changed.data_ptr(), st), "list_cc_rounds")

    def begin_rounds():
        begin()
        rounds()

    def finish():
        C._check(lib.list_cc_finish(fp, V, F, wp, wn, ids.data_ptr(), table[0].data_ptr(), table[1].data_ptr(),
                                    table[2].data_ptr(), totals.data_ptr(), st), "list_cc_finish")

    out = {"begin_ms": time_device(begin, iters)[0]}
    both = time_device(begin_rounds, iters)[0]
    out["rounds_ms"] = both - out["begin_ms"]                 # a batch of rounds on a fresh parent[]: the labelling
    flags = changed.tolist()
    out["rounds"] = flags.index(0) + 1 if 0 in flags else None
    begin_rounds()
    out["finish_ms"] = time_device(lambda: (begin_rounds(), finish()), iters)[0] - both
    K = int(totals.tolist()[0])
    counts = table[1:, :K].cpu().numpy()
    mask = C.select_components(counts[0], 1, 0)
    keep = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    Vk, Fk = int(counts[1][mask].sum()), int(counts[0][mask].sum())
    ov, of = torch.empty((Vk, 3), dtype=torch.float32, device=dev), torch.empty((Fk, 3), dtype=torch.int32, device=dev)
    out["compact_ms"] = time_device(lambda: C._check(lib.list_cc_compact(
        v.data_ptr(), fp, V, F, ids.data_ptr(), keep.data_ptr(), K, wp, wn, ov.data_ptr(), Vk, of.data_ptr(), Fk, st),
        "list_cc_compact"), iters)[0]
    return {k: (round(x, 4) if isinstance(x, float) else x) for k, x in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--field", default="all", choices=["all", "spheres_and_blobs", "predict_grid"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from list_amd import components as C, mesh
    dev = "cuda:0"
    volumes = {}
    if args.field in ("all", "spheres_and_blobs"):
        volumes["spheres_and_blobs"] = torch.from_numpy(spheres_and_blobs(args.res)).to(dev)
    if args.field in ("all", "predict_grid"):
        volumes["predict_grid"] = predicted_volume(args.res, dev)
    result = {"res": args.res, "device": torch.cuda.get_device_name(0), "fields": {}}
    for name, vol in volumes.items():
        mc_ms, _, (v, f) = time_device(lambda: mesh.marching_cubes(vol), args.iters)
        med, best, (kv, kf, info) = time_device(lambda: C.keep_components(v, f, keep=1), args.iters)
        r = {"V": len(v), "F": len(f), "marching_cubes_ms": round(mc_ms, 4), "keep_components_ms_median": round(med, 4),
             "keep_components_ms_min": round(best, 4), "K": info["K"], "kept_faces": info["kept_faces"],
             "rounds": info["rounds"], "stages": stages(v, f, args.iters)}
        try:
            host_ms, (hv, hf) = time_host(lambda: host_route(v, f))
            r["host_scipy_ms"] = round(host_ms, 1)
            r["device_equals_host"] = kv.cpu().numpy().tobytes() == hv.tobytes() and bool(
                np.array_equal(kf.cpu().numpy(), hf))
        except ImportError:
            r["host_scipy_ms"] = "scipy not installed"
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
