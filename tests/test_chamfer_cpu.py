"""CPU: the numpy restatement of the Chamfer loss (chamfer.*_cpu) against the torch path of CoarseNet and torch autograd;
the C ABI of include/list_loss.h (symbols, host arithmetic, refusals before any HIP call); chamfer.chamfer_distance on
CPU tensors."""

import numpy as np
import pytest
import torch

from list_amd import chamfer as CH
from list_amd.network import executors


def clouds(B, N, M, seed=0, spread=0.5):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-spread, spread, (B, N, 3)).astype(np.float32),
            rng.uniform(-spread, spread, (B, M, 3)).astype(np.float32))


def brute(x, y):
    """Plain loops over the float32 pairs: (d2, idx) of every x point."""
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    d2 = np.empty((B, N), np.float32)
    idx = np.empty((B, N), np.int32)
    for b in range(B):
        for i in range(N):
            best, bi = np.float32(np.inf), 0
            for j in range(M):
                d = x[b, i] - y[b, j]
                v = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if v < best:
                    best, bi = v, j
            d2[b, i] = np.nan if np.isnan(x[b, i]).any() else best
            idx[b, i] = bi
    return d2, idx


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (2, 7, 19), (3, 25, 11), (1, 40, 300)])
def test_nearest_sq_cpu_matches_plain_loops(B, N, M):
    x, y = clouds(B, N, M, seed=N + M)
    d2_xy, idx_xy, d2_yx, idx_yx = CH.nearest_sq_cpu(x, y, rows=16)
    bd, bi = brute(x, y)
    np.testing.assert_array_equal(d2_xy, bd)
    np.testing.assert_array_equal(idx_xy, bi)
    bd, bi = brute(y, x)
    np.testing.assert_array_equal(d2_yx, bd)
    np.testing.assert_array_equal(idx_yx, bi)


def test_nearest_sq_cpu_ties_and_nan():
    x = np.array([[[0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [5, 5, 5]]], np.float32)
    y = np.array([[[2, 2, 2], [0, 0, 0], [0, 0, 0], [np.nan, 1, 1], [1, 1, 1]]], np.float32)
    d2_xy, idx_xy, d2_yx, idx_yx = CH.nearest_sq_cpu(x, y, rows=2)
    assert idx_xy[0, 0] == 1 and d2_xy[0, 0] == 0                # duplicated points: the smallest index wins
    assert idx_xy[0, 1] == 4 and d2_xy[0, 1] == 0
    assert np.isnan(d2_xy[0, 2]) and idx_xy[0, 2] == 0           # a NaN source: NaN, index 0
    assert idx_xy[0, 3] == 0 and d2_xy[0, 3] == 27               # the NaN target never wins
    assert np.isnan(d2_yx[0, 3]) and idx_yx[0, 3] == 0
    assert idx_yx[0, 1] == 0 and idx_yx[0, 2] == 0
    assert np.isnan(CH.chamfer_distance_cpu(x, y))


@pytest.mark.parametrize("B,N,M", [(1, 5, 9), (2, 25, 25), (3, 17, 8), (4, 1, 25)])
def test_loss_cpu_matches_the_torch_path_direct_form(B, N, M):
    x, y = clouds(B, N, M, seed=B * N * M)
    want = float(executors.chamfer_distance(torch.from_numpy(x), torch.from_numpy(y))[0])
    got = float(CH.chamfer_distance_cpu(x, y))
    assert abs(got - want) <= 1e-6 * abs(want)


def test_loss_cpu_matches_the_torch_path_at_the_training_shape():
    x, y = clouds(2, 4096, 5000, seed=3)
    want = float(executors.chamfer_distance(torch.from_numpy(x), torch.from_numpy(y))[0])
    near = CH.nearest_sq_cpu(x, y)
    got = float(CH.chamfer_distance_cpu(x, y, nearest=near))
    assert abs(got - want) <= 1e-5 * abs(want)
    # the fixed float64 order against a plain float64 mean
    plain = near[0].astype(np.float64).mean(1).mean() + near[2].astype(np.float64).mean(1).mean()
    assert abs(got - plain) <= 1e-7 * plain


@pytest.mark.parametrize("g", [1.0, 1000.0])
def test_grad_cpu_matches_torch_autograd(g):
    x, y = clouds(3, 21, 13, seed=11)
    tx, ty = torch.from_numpy(x.astype(np.float64)).requires_grad_(), torch.from_numpy(y.astype(np.float64)).requires_grad_()
    (executors.chamfer_distance(tx, ty)[0] * g).backward()
    gx, gy = CH.chamfer_grad_cpu(x, y, grad_loss=g)
    np.testing.assert_allclose(gx, tx.grad.numpy(), rtol=1e-5, atol=1e-7 * g)
    np.testing.assert_allclose(gy, ty.grad.numpy(), rtol=1e-5, atol=1e-7 * g)


def test_grad_cpu_pileup_sums_every_source():
    x, y = clouds(1, 10, 3000, seed=5)
    x[0, 4] = 0.0
    y[0] *= 1e-3                                 # every y point nearest to x[0, 4]
    _, idx_xy, _, idx_yx = near = CH.nearest_sq_cpu(x, y)
    assert np.all(idx_yx == 4)
    gx, _ = CH.chamfer_grad_cpu(x, y, nearest=near)
    want = 2 / 10 * (x[0, 4].astype(np.float64) - y[0, idx_xy[0, 4]]) + 2 / 3000 * (x[0, 4] - y[0].astype(np.float64)).sum(0)
    np.testing.assert_allclose(gx[0, 4], want, rtol=1e-6)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return CH.load()


def test_library_exports_the_loss_symbols(lib):
    from list_amd import hip
    assert sorted(CH.LOSS_EXPORTS) == sorted(
        ["list_chamfer_workspace_bytes", "list_chamfer_fwd", "list_chamfer_bwd", "list_loss_last_error"])
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9


def _a(n):
    return (n + 255) // 256 * 256


def test_workspace_bytes_is_host_arithmetic(lib):
    for B, N, M in [(12, 4096, 5000), (12, 4096, 10000), (1, 1, 1), (3, 777, 3001)]:
        want = (_a(8 * B * (N + M)) + _a(16 * B) + 2 * _a(4 * B * N) + _a(4 * B * M)
                + 2 * _a(4 * B * M) + _a(4 * B * N))
        assert lib.list_chamfer_workspace_bytes(B, N, M) == want
    assert lib.list_chamfer_workspace_bytes(12, 4096, 10000) < 8 << 20
    for bad in [(0, 5, 5), (2, 0, 5), (2, 5, 0), (-1, 5, 5), (2, 1 << 31, 5), (4, 1 << 30, 5)]:
        assert lib.list_chamfer_workspace_bytes(*bad) == 0
        assert lib.list_loss_last_error()


def test_refusals_come_before_any_hip_call(lib):
    fake = 256                                    # never dereferenced: every refusal below is a host check
    ws = lib.list_chamfer_workspace_bytes(2, 10, 20)
    fwd = lambda B, N, M, x=fake, w=fake, wb=ws, loss=fake: lib.list_chamfer_fwd(
        x, fake, B, N, M, fake, fake, fake, fake, loss, w, wb, None)
    bwd = lambda B, N, M, gx=fake, gy=fake, g=fake, wb=ws, idx=fake: lib.list_chamfer_bwd(
        fake, fake, B, N, M, idx, fake, g, gx, gy, fake, wb, None)
    assert fwd(0, 10, 20) == -2 and b"B = 0" in lib.list_loss_last_error()
    assert fwd(2, 0, 20) == -2 and b"N = 0" in lib.list_loss_last_error()
    assert fwd(2, 10, -3) == -2 and b"M = -3" in lib.list_loss_last_error()
    assert fwd(4, 1 << 30, 5) == -2 and b"INT32_MAX" in lib.list_loss_last_error()
    assert fwd(2, 10, 20, x=None) == -1 and b"NULL" in lib.list_loss_last_error()
    assert fwd(2, 10, 20, loss=None) == -1
    assert fwd(2, 10, 20, w=None) == -1
    assert fwd(2, 10, 20, wb=ws - 1) == -3 and b"workspace" in lib.list_loss_last_error()
    assert bwd(0, 10, 20) == -2
    assert bwd(2, 10, 20, g=None) == -1 and b"NULL" in lib.list_loss_last_error()
    assert bwd(2, 10, 20, idx=None) == -1
    assert bwd(2, 10, 20, gx=None, gy=None) == -1 and b"both NULL" in lib.list_loss_last_error()
    assert bwd(2, 10, 20, wb=ws - 1) == -3 and b"workspace" in lib.list_loss_last_error()


# ---- chamfer.chamfer_distance on CPU tensors ------------------------------------------------------------------------------
def test_chamfer_distance_on_cpu_is_the_torch_path():
    x, y = clouds(2, 30, 40, seed=9)
    tx, ty = torch.from_numpy(x).requires_grad_(), torch.from_numpy(y).requires_grad_()
    loss, normals = CH.chamfer_distance(tx, ty)
    assert normals is None
    want = executors.chamfer_distance(torch.from_numpy(x), torch.from_numpy(y))[0]
    assert float(loss.detach()) == float(want)
    loss.backward()
    assert tx.grad is not None and ty.grad is not None and torch.isfinite(tx.grad).all()
    # CoarseNet.calc_loss on CPU tensors is unchanged: the executor's torch path, x 1000
    ex = executors.CoarseNet.__new__(executors.CoarseNet)
    ex.loss_fn = executors.chamfer_distance
    assert float(ex.calc_loss(torch.from_numpy(x), torch.from_numpy(y))) == float(want * 1000)


def test_chamfer_distance_refuses_bad_clouds():
    x = torch.zeros(2, 5, 3)
    for a, b in [(x, torch.zeros(3, 5, 3)), (x, torch.zeros(2, 5, 2)), (torch.zeros(2, 5, 4), x),
                 (torch.zeros(2, 0, 3), x), (x, torch.zeros(2, 0, 3)), (torch.zeros(0, 5, 3), torch.zeros(0, 5, 3)),
                 (torch.zeros(5, 3), x), (x.long(), x)]:
        with pytest.raises(ValueError):
            CH.chamfer_distance(a, b)
    with pytest.raises(ValueError):
        CH.nearest_sq(x, x)                      # the device function: not on CPU tensors
