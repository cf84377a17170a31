#!/usr/bin/env python3
"""Time stage 1's Chamfer loss (not part of bench.py): forward + backward of the HIP loss (chamfer.chamfer_distance)
against the torch path (network.executors.chamfer_distance: cdist, min, mean), and the CoarseNet training step
(executor.train + backward + Adam) with each loss.  Prints one JSON line.

    python tools/chamfer_bench.py [--iters 20] [--warmup 3] [--out chamfer_bench.json]

Times are HIP events around whole calls (Python included), median and min of --iters after --warmup calls of the
same shape; peak memory is torch.cuda.max_memory_allocated over one call beyond what was allocated before it.  Per-kernel
times: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch        # noqa: E402

DEV = "cuda:0"


def time_events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def loss_case(B, N, M, iters, warmup):
    from list_amd import chamfer
    from list_amd.network import executors
    g = torch.Generator(device="cpu").manual_seed(B * N + M)
    x = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV).requires_grad_()
    y = (torch.rand(B, M, 3, generator=g) - 0.5).to(DEV)

    def step(fn):
        def run():
            x.grad = None
            (fn(x, y)[0] * 1000).backward()
        return run

    r = {"B": B, "N": N, "M": M}
    for name, fn in (("hip", chamfer.chamfer_distance), ("torch", executors.chamfer_distance)):
        med, best = time_events(step(fn), iters, warmup)
        r[name] = {"fwd_bwd_ms_median": round(med, 4), "fwd_bwd_ms_min": round(best, 4),
                   "peak_mb": round(peak_bytes(step(fn)) / 2 ** 20, 1)}
    with torch.no_grad():
        a, b = float(chamfer.chamfer_distance(x, y)[0]), float(executors.chamfer_distance(x, y)[0])
    r["loss_rel_diff"] = abs(a - b) / abs(b)
    r["speedup"] = round(r["torch"]["fwd_bwd_ms_median"] / r["hip"]["fwd_bwd_ms_median"], 2)
    # the forward kernel's paper bound: 2*B*N*M pairs, 8 packed + 3 scalar vector instructions per 2 pairs
    pairs = 2 * B * N * M
    r["pairs_G"] = round(pairs / 1e9, 3)
    return r


def train_step_case(iters, warmup, B=12, res=224):
    from list_amd import arguments, chamfer, utils
    from list_amd.network import executors
    torch.manual_seed(0)
    cfg = arguments.default_config(model="network.models.CoarseNet",
                                   dataset="datasets.Datasets.SyntheticIM2PointFarthest", img_res=res,
                                   train_batch_size=B, synthetic_len=B)
    model = utils.get_class(cfg.model)(cfg).to(DEV)
    ex = executors.CoarseNet(cfg, model)
    opt = torch.optim.Adam(model.parameters(), lr=cfg.lr, betas=(cfg.beta1, 0.999), weight_decay=cfg.weight_decay)
    batch = next(iter(torch.utils.data.DataLoader(utils.get_class(cfg.dataset)(cfg, "train"), batch_size=B)))
    batch = {k: v.to(DEV) for k, v in batch.items()}
    r = {"B": B, "img_res": res, "points": int(np.prod(cfg.point_degree)), "gt_points": int(batch["pc"].shape[1])}
    for name, fn in (("hip", chamfer.chamfer_distance), ("torch", executors.chamfer_distance)):
        def run():
            opt.zero_grad(set_to_none=True)
            pred, _ = ex.train(batch, calc_loss=False)
            (fn(pred, batch["pc"])[0] * 1000).backward()
            opt.step()
        med, best = time_events(run, iters, warmup)
        r[name] = {"step_ms_median": round(med, 3), "step_ms_min": round(best, 3),
                   "peak_mb": round(peak_bytes(run) / 2 ** 20, 1)}
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chamfer_bench.py measures on the GPU: no device found")
    import __graft_entry__ as ge
    ge.build()
    result = {"device": torch.cuda.get_device_name(0),
              "loss": [loss_case(12, 4096, 5000, args.iters, args.warmup),
                       loss_case(12, 4096, 10000, args.iters, args.warmup)],
              "coarsenet_step": train_step_case(max(5, args.iters // 2), args.warmup)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
