"""Inputs of the stage-2 loss tests (test_s2loss_cpu.py, test_s2loss_gpu.py)."""
import numpy as np


def case(n_occ, B, N, seed=0, soft=False):
    """occ in (0, 1) with a few saturated elements, 0 / 1 targets (or soft ones), SDF values around 0.5."""
    rng = np.random.default_rng(seed)
    occ = rng.uniform(1e-4, 1 - 1e-4, n_occ).astype(np.float32)
    occ[rng.integers(0, n_occ, max(1, n_occ // 50))] = 0.0
    occ[rng.integers(0, n_occ, max(1, n_occ // 50))] = 1.0
    gt = rng.uniform(0, 1, n_occ).astype(np.float32) if soft else (rng.uniform(0, 1, n_occ) < 0.3).astype(np.float32)
    pred = rng.normal(0.4, 0.3, (B, N)).astype(np.float32)
    sdf = rng.normal(0.4, 0.3, (B, N)).astype(np.float32)
    return occ, gt, pred, sdf
