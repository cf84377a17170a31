"""GPU: the Chamfer loss in HIP (include/list_loss.h, chamfer.*) against its numpy restatement and the torch path;
CoarseNet's executor step and train.py's stage 1 on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_chamfer_cpu import clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()


def _CH():
    from list_amd import chamfer
    return chamfer


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _with_duplicates(x, y, seed):
    """Copies of points inside each cloud and across the two, so that ties decide indices."""
    rng = np.random.default_rng(seed)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    for b in range(B):
        k = max(1, M // 10)
        y[b, rng.integers(0, M, k)] = y[b, rng.integers(0, M, k)]
        x[b, rng.integers(0, N, max(1, N // 10))] = y[b, rng.integers(0, M, max(1, N // 10))]
        x[b, rng.integers(0, N, max(1, N // 20))] = x[b, rng.integers(0, N, max(1, N // 20))]
    return x, y


def _torch_path(x, y):
    from list_amd.network import executors
    return executors.chamfer_distance(x, y)[0]


@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (2, 777, 3001), (3, 5000, 257), (12, 4096, 5000), (4, 4096, 10000)])
def test_nearest_and_loss_against_numpy(B, N, M):
    CH = _CH()
    x, y = _with_duplicates(*clouds(B, N, M, seed=N ^ M), seed=B)
    near = CH.nearest_sq_cpu(x, y)
    got = [t.cpu().numpy() for t in CH.nearest_sq(_t(x), _t(y))]
    for g, w in zip(got, near):
        np.testing.assert_array_equal(g, w)
    loss = float(CH.chamfer_distance(_t(x), _t(y))[0])
    want = float(CH.chamfer_distance_cpu(x, y, nearest=near))
    assert abs(loss - want) <= 1e-6 * abs(want)
    if B * N * M <= 4 * 4096 * 10000:
        ref = float(_torch_path(_t(x), _t(y)))
        assert abs(loss - ref) <= 1e-5 * abs(ref)


def _grads(x, y, scale=1.0, y_grad=True, dtype=torch.float32):
    CH = _CH()
    tx = _t(x).to(dtype).requires_grad_()
    ty = _t(y).to(dtype).requires_grad_(y_grad)
    loss = CH.chamfer_distance(tx, ty)[0] * scale
    loss.backward()
    return loss, tx.grad, ty.grad


def _close(got, want, tol=1e-6):
    got = got.detach().cpu().double().numpy()
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    assert err <= tol, err


@pytest.mark.parametrize("B,N,M", [(2, 777, 3001), (12, 4096, 5000)])
def test_grads_against_numpy(B, N, M):
    CH = _CH()
    x, y = _with_duplicates(*clouds(B, N, M, seed=7), seed=3)
    near = CH.nearest_sq_cpu(x, y)
    _, gx, gy = _grads(x, y, scale=1000.0)                     # CoarseNet.calc_loss's scale
    wx, wy = CH.chamfer_grad_cpu(x, y, grad_loss=1000.0, nearest=near)
    _close(gx, wx)
    _close(gy, wy)
    # y without requires_grad: only grad_x is computed, and it is the same
    _, gx2, gy2 = _grads(x, y, scale=1000.0, y_grad=False)
    assert gy2 is None
    assert torch.equal(gx, gx2)
    # float64 inputs: float32 arithmetic, gradients in float64
    loss64, gx64, _ = _grads(x, y, dtype=torch.float64)
    assert loss64.dtype == torch.float64 and gx64.dtype == torch.float64
    _close(gx64, CH.chamfer_grad_cpu(x, y, nearest=near)[0])


def test_grads_match_torch_autograd():
    x, y = clouds(3, 500, 700, seed=21)
    _, gx, gy = _grads(x, y, scale=1000.0)
    tx, ty = _t(x).double().requires_grad_(), _t(y).double().requires_grad_()
    (_torch_path(tx, ty) * 1000.0).backward()
    _close(gx, tx.grad.cpu().numpy(), 1e-5)
    _close(gy, ty.grad.cpu().numpy(), 1e-5)


def test_pileup():
    CH = _CH()
    # every y point nearest to one x point (an untrained decoder's worst case): a 5000-long CSR segment
    x, y = clouds(2, 4096, 5000, seed=1)
    x[:, 17] = 0.0
    y *= 1e-3
    near = CH.nearest_sq_cpu(x, y)
    assert np.all(near[3] == 17)
    _, gx, gy = _grads(x, y, scale=1000.0)
    wx, wy = CH.chamfer_grad_cpu(x, y, grad_loss=1000.0, nearest=near)
    _close(gx, wx)
    _close(gy, wy)
    # every x point at one spot: all x tie, every y picks index 0 and every x the same y
    x = np.zeros((2, 4096, 3), np.float32) + np.float32(0.25)
    y = clouds(2, 4096, 5000, seed=2)[1]
    near = CH.nearest_sq_cpu(x, y)
    got = [t.cpu().numpy() for t in CH.nearest_sq(_t(x), _t(y))]
    for g, w in zip(got, near):
        np.testing.assert_array_equal(g, w)
    _, gx, gy = _grads(x, y)
    wx, wy = CH.chamfer_grad_cpu(x, y, nearest=near)
    _close(gx, wx)
    _close(gy, wy)


def test_two_runs_are_bitwise_equal():
    x, y = clouds(12, 4096, 5000, seed=4)
    x[:, :300] = 0.0                                            # a long segment as well
    a = _grads(x, y, scale=1000.0)
    b = _grads(x, y, scale=1000.0)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_memory_beyond_inputs_and_outputs():
    CH = _CH()
    x, y = clouds(12, 4096, 10000, seed=6)
    tx, ty = _t(x).requires_grad_(), _t(y).requires_grad_()
    torch.cuda.synchronize()
    from list_amd import hip
    hip.release_workspaces()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = CH.chamfer_distance(tx, ty)[0] * 1000
    loss.backward()
    torch.cuda.synchronize()
    grads = tx.grad.numel() * 4 + ty.grad.numel() * 4
    extra = torch.cuda.max_memory_allocated() - base - grads
    assert extra < 64 << 20, extra
    tx.grad = ty.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    (_torch_path(tx, ty) * 1000).backward()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base > 2 << 30


def test_nan_coordinate_gives_nan_loss():
    CH = _CH()
    x, y = clouds(2, 300, 400, seed=8)
    x[1, 5, 2] = np.nan
    loss, gx, _ = _grads(x, y)
    assert torch.isnan(loss)
    d2_xy, idx_xy, d2_yx, idx_yx = CH.nearest_sq(_t(x), _t(y))
    assert torch.isnan(d2_xy[1, 5]) and int(idx_xy[1, 5]) == 0
    assert int(idx_yx.min()) >= 0 and int(idx_yx.max()) < 300 and int(idx_xy.max()) < 400
    y[0, 3, 0] = np.nan
    assert torch.isnan(CH.chamfer_distance(_t(x), _t(y))[0])


def test_bad_inputs_raise_before_any_launch():
    CH = _CH()
    x = torch.zeros(2, 5, 3, device=DEV)
    for a, b in [(x, torch.zeros(3, 5, 3, device=DEV)), (x, torch.zeros(2, 5, 2, device=DEV)),
                 (x, torch.zeros(2, 0, 3, device=DEV)), (x, torch.zeros(2, 5, 3))]:
        with pytest.raises(ValueError):
            CH.chamfer_distance(a, b)
        with pytest.raises(ValueError):
            CH.nearest_sq(a, b)


def test_non_contiguous_inputs():
    CH = _CH()
    x, y = clouds(2, 300, 500, seed=12)
    tx = _t(np.ascontiguousarray(x.transpose(0, 2, 1))).transpose(1, 2)
    assert not tx.is_contiguous()
    assert float(CH.chamfer_distance(tx, _t(y))[0]) == float(CH.chamfer_distance(_t(x), _t(y))[0])


def _coarse_executor(B, res):
    from list_amd import arguments, utils
    from list_amd.network import executors
    torch.manual_seed(0)
    cfg = arguments.default_config(model="network.models.CoarseNet",
                                   dataset="datasets.Datasets.SyntheticIM2PointFarthest", img_res=res,
                                   train_batch_size=B, synthetic_len=B)
    model = utils.get_class(cfg.model)(cfg).to(DEV)
    ds = utils.get_class(cfg.dataset)(cfg, "train")
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=B)))
    return executors.CoarseNet(cfg, model), batch


def test_coarsenet_step_matches_the_torch_path():
    CH = _CH()
    from list_amd.network import executors
    ex, batch = _coarse_executor(2, 128)
    ex.model.train()
    pred, losses = ex.train(batch)                              # the HIP loss: pred is on the GPU
    gt = batch["pc"].to(DEV)
    params = [p for p in ex.model.point_decoder.parameters() if p.requires_grad]
    got = torch.autograd.grad(losses["chamfer_loss"], params, retain_graph=True, allow_unused=True)
    # the loss against the torch path (in float64: in float32 its |x|^2 + |y|^2 - 2 x.y form loses the small distances
    # of an untrained decoder's clustered points)
    ref = executors.chamfer_distance(pred.detach().double(), gt.double())[0] * 1000
    assert abs(float(losses["chamfer_loss"].detach()) - float(ref)) <= 1e-5 * abs(float(ref))
    # the decoder's gradients against the header's gradient (numpy) carried through the same graph.  (Against any
    # other arithmetic they differ by ~1e-3 of their largest: among clustered points the nearest of a target is a near
    # tie, and a different winner takes that target's whole reverse term.)
    p, y = pred.detach().cpu().numpy(), gt.cpu().numpy()
    gp, _ = CH.chamfer_grad_cpu(p, y, grad_loss=1000.0)
    want = torch.autograd.grad(pred, params, grad_outputs=_t(gp), allow_unused=True)
    assert any(g is not None for g in got)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert float((g.double() - w.double()).abs().max()) <= 1e-4 * max(float(w.abs().max()), 1e-12)


def test_train_py_coarsenet_one_step_on_the_gpu(tmp_path):
    out = str(tmp_path) + "/"
    cmd = [sys.executable, os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "train.py"),
           "--model", "network.models.CoarseNet", "--dataset", "datasets.Datasets.SyntheticIM2PointFarthest",
           "--max_steps", "1", "--epochs", "1", "--synthetic_len", "12", "--output_dir", out, "-e", "coarse"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(out + "coarse/checkpoints/best_model_train.pt.tar")
