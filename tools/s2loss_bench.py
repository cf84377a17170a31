#!/usr/bin/env python3
"""Time stage 2's loss (not part of bench.py): the torch expressions of network.executors.LIST.calc_loss against the HIP
loss (s2loss.stage2_loss), forward and forward + backward, at the training step's shape (B = 8, R = 128, N = 20 000); and
the host-to-device copy of the occupancy target as float32 and as uint8.  Prints one JSON line.

    python tools/s2loss_bench.py [--iters 20] [--warmup 3] [--out s2loss_bench.json]

Times are HIP events around whole calls (Python included), median and min of --iters after --warmup calls of the same
shape; peak memory is torch.cuda.max_memory_allocated over one call beyond what was allocated before it.  The byte floor
of a pass is what it has to move (forward: occ and its target once; forward + backward: both twice and one gradient,
5 x n_occ x 4 bytes with float32 targets) over the 6.3 TB/s a streaming kernel reaches on the MI355X.  Per-kernel times:
run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import torch        # noqa: E402

from chamfer_bench import peak_bytes, time_events  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12


def loss_case(B, R, N, iters, warmup):
    from list_amd import arguments, s2loss
    from list_amd.network import executors
    g = torch.Generator(device="cpu").manual_seed(B * R + N)
    occ = torch.sigmoid(4 * torch.randn(B, 1, R, R, R, generator=g)).to(DEV).requires_grad_()
    occ_gt = (torch.rand(B, 1, R, R, R, generator=g) < 0.05).float().to(DEV)
    sdf_pred = (0.3 * torch.randn(B, N, generator=g)).to(DEV).requires_grad_()
    sdf_gt = (0.3 * torch.randn(B, N, generator=g)).to(DEV)
    ex = {name: executors.LIST(arguments.default_config(stage2_loss=name), None) for name in ("torch", "hip")}
    targets = {"f32": occ_gt, "u8": occ_gt.to(torch.uint8)}

    def fwd(name, t):
        def run():
            with torch.no_grad():
                ex[name].calc_loss((occ, sdf_pred), (targets[t], sdf_gt))
        return run

    def fwd_bwd(name, t):
        def run():
            occ.grad = sdf_pred.grad = None
            loss = ex[name].calc_loss((occ, sdf_pred), (targets[t], sdf_gt))
            (loss["occ_loss"] + loss["sdf_loss"]).backward()
        return run

    n_occ = occ.numel()
    r = {"B": B, "R": R, "N": N, "n_occ": n_occ}
    for name in ("torch", "hip"):
        for t in ("f32", "u8"):
            fm, fb = time_events(fwd(name, t), iters, warmup)
            sm, sb = time_events(fwd_bwd(name, t), iters, warmup)
            r[f"{name}_{t}"] = {"fwd_ms_median": round(fm, 4), "fwd_ms_min": round(fb, 4),
                                "fwd_bwd_ms_median": round(sm, 4), "fwd_bwd_ms_min": round(sb, 4),
                                "fwd_peak_mb": round(peak_bytes(fwd(name, t)) / 2 ** 20, 1),
                                "fwd_bwd_peak_mb": round(peak_bytes(fwd_bwd(name, t)) / 2 ** 20, 1)}
    with torch.no_grad():
        a = ex["hip"].calc_loss((occ, sdf_pred), (occ_gt, sdf_gt))
        b = ex["torch"].calc_loss((occ, sdf_pred), (occ_gt, sdf_gt))
    r["rel_diff"] = {k: abs(float(a[k]) - float(b[k])) / abs(float(b[k])) for k in s2loss.KEYS}
    for t, gt_bytes in (("f32", 4), ("u8", 1)):
        floor_fwd = n_occ * (4 + gt_bytes) / HBM_BYTES_PER_S * 1e3
        floor_all = n_occ * (2 * (4 + gt_bytes) + 4) / HBM_BYTES_PER_S * 1e3
        h = r[f"hip_{t}"]
        r[f"floor_{t}"] = {"fwd_ms": round(floor_fwd, 4), "fwd_bwd_ms": round(floor_all, 4),
                           "fwd_floor_fraction": round(floor_fwd / h["fwd_ms_median"], 3),
                           "fwd_bwd_floor_fraction": round(floor_all / h["fwd_bwd_ms_median"], 3)}
        r[f"speedup_{t}"] = {"fwd": round(r[f"torch_{t}"]["fwd_ms_median"] / h["fwd_ms_median"], 2),
                             "fwd_bwd": round(r[f"torch_{t}"]["fwd_bwd_ms_median"] / h["fwd_bwd_ms_median"], 2)}
    return r


def copy_case(B, R, iters, warmup):
    """The loader's occupancy target to the device, as executor.train does it (.to(dev) of a pageable host tensor, and of
    a pinned one as a DataLoader with pin_memory hands it over)."""
    host = (torch.rand(B, 1, R, R, R) < 0.05)
    r = {}
    for name, dtype in (("f32", torch.float32), ("u8", torch.uint8)):
        t = host.to(dtype)
        pinned = t.pin_memory()
        med, best = time_events(lambda: t.to(DEV), iters, warmup)
        pmed, pbest = time_events(lambda: pinned.to(DEV, non_blocking=True), iters, warmup)
        r[name] = {"mb": round(t.numel() * t.element_size() / 2 ** 20, 1), "pageable_ms_median": round(med, 3),
                   "pageable_ms_min": round(best, 3), "pinned_ms_median": round(pmed, 3), "pinned_ms_min": round(pbest, 3)}
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("s2loss_bench.py measures on the GPU: no device found")
    import __graft_entry__ as ge
    ge.build()
    result = {"device": torch.cuda.get_device_name(0), "loss": loss_case(8, 128, 20000, args.iters, args.warmup),
              "occ_gt_copy": copy_case(8, 128, max(5, args.iters // 2), args.warmup)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
