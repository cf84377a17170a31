"""Event timing shared by the bench tools of the opt-in stages (voxenc_bench.py, imgenc_bench.py)."""
import numpy as np
import torch


def time_events(fn, iters, warmup):
    """Median milliseconds of fn() between two HIP events over `iters` calls, after `warmup` calls."""
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
    return float(np.median(ms))


def interleaved(fns, iters, warmup, rounds):
    """{name: the smallest time_events median over `rounds` rounds}, the candidates taking turns within a round."""
    best = {k: float("inf") for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            best[k] = min(best[k], time_events(fn, iters, warmup))
    return best
