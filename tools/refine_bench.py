#!/usr/bin/env python3
"""Time the coarse-to-fine grid (refine.py, not part of bench.py): LIST.predict_grid dense vs refine=s on one GPU, for
the seeded model (oracle.fill.fill_state(seed=2), its field moved to its median through `level`) and for a
coordinate-only field (fc_* set so that the SDF is the octahedron 0.3 - (|x|+|y|+|z|), a closed surface of a
ShapeNet-like extent), with the share of the grid points queried and the time of the refine kernels on their own.

    python tools/refine_bench.py [--res 256] [--iters 5] [--precision bf16x3] [--out refine_bench.json]

The encoders run once per model (encode is frozen), so the times are those of the grid alone: the queries plus, for
refine=s, the lattice pass, the count (one host synchronisation), emit, the refined queries and the fill.  Median of
--iters after one warm-up, CUDA events around whole predict_grid calls."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch        # noqa: E402


def make_executor(res, precision, dev):
    from oracle import fill, synth
    from list_amd import arguments, utils
    from list_amd.train import _Module
    cfg = arguments.default_config(vox_res=128, train_batch_size=1, mcube_znum=res, precision=precision)
    cfg.device = torch.device(dev)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(dev)
    ex = utils.get_class("network.executors.LIST")(cfg, _Module(net))
    img = torch.from_numpy(synth.uniform(78, (1, 3, 224, 224))).to(dev)
    with torch.no_grad():
        enc = net.encode(img)
    net.encode = lambda *a, **k: enc
    return ex, net, img


def octahedron(net, r=0.3):
    fc = net.sdf_decoder.fc
    with torch.no_grad():
        for name in ("fc_0", "fc_1", "fc_2", "fc_out"):
            fc[name].weight.zero_()
            fc[name].bias.zero_()
        n_in = fc["fc_0"].weight.shape[1]
        for c in range(3):
            fc["fc_0"].weight[2 * c, n_in - 3 + c, 0] = 1.0
            fc["fc_0"].weight[2 * c + 1, n_in - 3 + c, 0] = -1.0
        fc["fc_1"].weight[0, :6, 0] = 1.0
        fc["fc_2"].weight[0, 0, 0] = 1.0
        fc["fc_out"].weight[0, 0, 0] = -0.5
        fc["fc_out"].bias[0] = r
    net.sdf_decoder.invalidate()


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def kernels_alone(vol, R, s, level, iters):
    """count (incl. its read-back) + emit + fill on the lattice of `vol`, with the values read from `vol`."""
    from list_amd import refine as RF
    c = torch.from_numpy(RF.lattice_indices(R, s)).to(vol.device)
    lat = vol[c][:, c][:, :, c].contiguous()
    plan = RF.count(lat, R, s, level)
    _, idx = RF.emit(plan)
    vals = vol.reshape(-1)[idx.long()].contiguous()

    def run():
        p = RF.count(lat, R, s, level)
        RF.emit(p)
        RF.fill(p, lat, vals)
    return timed(run, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--big", type=int, default=512, help="the refined-only resolution (0: skip)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    rows = []
    for field in ("octahedron", "seeded"):
        ex, net, img = make_executor(a.res, a.precision, dev)
        if field == "octahedron":
            octahedron(net)
        level = 0.0
        dense = ex.predict_grid(img)[0]
        if field == "seeded":
            level = float(dense.median())
        t_dense = timed(lambda: ex.predict_grid(img), a.iters)
        row = {"field": field, "res": a.res, "precision": a.precision, "dense_ms": round(t_dense, 2)}
        print(f"{field} {a.res}^3 {a.precision}: dense {t_dense:.2f} ms", flush=True)
        for s in (2, 4, 8):
            t = timed(lambda: ex.predict_grid(img, refine=s, level=level), a.iters)
            st = dict(ex.last_grid_stats)
            vol = ex.predict_grid(img, refine=s, level=level)[0]
            tk = kernels_alone(vol, a.res, s, level, a.iters)
            row[f"s{s}"] = {"ms": round(t, 2), "speedup": round(t_dense / t, 2), "fraction": round(st["fraction"], 4),
                            "refine_kernels_ms": round(tk, 3)}
            print(f"  refine s={s}: {t:.2f} ms ({t_dense / t:.2f}x), {100 * st['fraction']:.2f} % of the points "
                  f"queried, refine kernels alone {tk:.3f} ms", flush=True)
        if a.big:
            exb, netb, imgb = make_executor(a.big, a.precision, dev)
            if field == "octahedron":
                octahedron(netb)
            tb = timed(lambda: exb.predict_grid(imgb, refine=4, level=level), max(1, a.iters // 2))
            row[f"refined_{a.big}_s4"] = {"ms": round(tb, 2), "fraction": round(exb.last_grid_stats["fraction"], 4)}
            print(f"  {a.big}^3 refine s=4: {tb:.2f} ms, {100 * exb.last_grid_stats['fraction']:.2f} % queried",
                  flush=True)
            del exb, netb
            torch.cuda.empty_cache()
        rows.append(row)
        del ex, net
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
