"""GPU: the coarse-to-fine SDF grid (include/list_refine.h, list_amd.refine, LIST.predict_grid(refine=s)) -- each
kernel against its numpy restatement bit for bit, the meshing guarantee through the real network, exactness of every
queried point against the dense grid, determinism, test.py --refine_stride and the sharded passes on RCCL."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def _rf():
    from list_amd import refine
    return refine


def _random_lattice(K, seed):
    """A smooth field with a surface, noise and a few NaN corners."""
    rng = np.random.default_rng(seed)
    a = np.linspace(-1, 1, K)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    v = (0.6 - np.sqrt(x * x + y * y + z * z) + 0.05 * rng.standard_normal((K, K, K))).astype(np.float32)
    v.reshape(-1)[rng.choice(v.size, max(1, v.size // 500), replace=False)] = np.nan
    return v


# ---- 1. each kernel against the numpy restatement -------------------------------------------------------------------
@pytest.mark.parametrize("R", [37, 64, 101, 256])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_kernels_match_the_numpy_restatement(R, s):
    RF = _rf()
    K, NB = RF.dims(R, s)
    lat = _random_lattice(K, R * 10 + s)
    band = RF.default_band(R, s) * 0.25
    level = 0.02
    t = torch.from_numpy(lat).to(DEV)
    plan = RF.count(t, R, s, level, band)
    act, dil = RF.classify_cpu(lat, level, band)
    ga, gd = plan.masks()
    assert torch.equal(ga.cpu(), torch.from_numpy(act.astype(np.uint8)))
    assert torch.equal(gd.cpu(), torch.from_numpy(dil.astype(np.uint8)))
    coords, idx = RF.refined_points_cpu(dil, R, s)
    assert plan.n == len(idx) and 0 < plan.n <= R ** 3 - K ** 3
    gc, gi = RF.emit(plan)
    assert np.array_equal(gi.cpu().numpy(), idx) and np.array_equal(gc.cpu().numpy(), coords)
    # the coordinates are the dense grid's, bit for bit
    from list_amd import utils
    dense_pts = utils.grid_points_on_device(-0.5, 0.5, R, DEV)
    assert torch.equal(gc, dense_pts[gi.long()])
    vals = np.random.default_rng(5).standard_normal(plan.n).astype(np.float32)
    vol = RF.fill(plan, t, torch.from_numpy(vals).to(DEV))
    want = RF.fill_cpu(lat, vals, idx, R, s)
    assert np.array_equal(vol.cpu().numpy(), want, equal_nan=True)
    plan2 = RF.count(t, R, s, level, band)                   # deterministic
    assert plan2.n == plan.n and torch.equal(RF.emit(plan2)[1], gi)


def test_small_grids_and_refusals():
    RF = _rf()
    from list_amd import hip
    for R, s in [(2, 2), (2, 8), (3, 8), (5, 4)]:
        K, _ = RF.dims(R, s)
        lat = np.zeros((K, K, K), np.float32)
        lat[0, 0, 0] = 1.0
        t = torch.from_numpy(lat).to(DEV)
        plan = RF.count(t, R, s, 0.0, 0.0)
        _, dil = RF.classify_cpu(lat, 0.0, 0.0)
        c, i = RF.refined_points_cpu(dil, R, s)
        assert plan.n == len(i) == R ** 3 - K ** 3
        vals = np.arange(plan.n, dtype=np.float32)
        got = RF.fill(plan, t, torch.from_numpy(vals).to(DEV)).cpu().numpy()
        assert np.array_equal(got, RF.fill_cpu(lat, vals, i, R, s))
    with pytest.raises(hip.ListError) as e:
        RF.count(torch.zeros(3, 3, 3, device=DEV), 1291, 4)
    assert "INT32_MAX" in str(e.value)
    lib = RF.load()
    need = lib.list_refine_workspace_bytes(64, 4)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lat = torch.zeros(17, 17, 17, device=DEV)
    tot = torch.empty(1, dtype=torch.int64, device=DEV)
    assert lib.list_refine_count(lat.data_ptr(), 64, 4, 0.0, 0.1, ws.data_ptr(), need - 1, tot.data_ptr(), None) == -3
    assert b"workspace" in lib.list_refine_last_error()


# ---- the network ------------------------------------------------------------------------------------------------------
def _executor(precision="bf16x3", mcube_znum=40, vox_res=32):
    from oracle import fill, synth
    from list_amd import arguments, utils
    from list_amd.train import _Module
    cfg = arguments.default_config(vox_res=vox_res, train_batch_size=1, mcube_znum=mcube_znum, test_pointnum=5000,
                                   precision=precision)
    cfg.device = torch.device(DEV)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(DEV)
    ex = utils.get_class("network.executors.LIST")(cfg, _Module(net))
    img = torch.from_numpy(synth.uniform(78, (1, 3, 64, 64))).to(DEV)
    with torch.no_grad():
        enc = net.encode(img)
    net.encode = lambda *a, **k: enc                # MIOpen is not run-to-run deterministic: one set of maps
    return ex, net, img


def _octahedron(net, r=0.3):
    """fc_* set so that the SDF is r - (|x|+|y|+|z|) of the query, built from ReLU units on the three coordinate
    features (the last columns of fc_0; the decoder sees the query permuted and scaled by 2)."""
    fc = net.sdf_decoder.fc
    with torch.no_grad():
        for name in ("fc_0", "fc_1", "fc_2", "fc_out"):
            fc[name].weight.zero_()
            fc[name].bias.zero_()
        n_in = fc["fc_0"].weight.shape[1]
        for c in range(3):
            fc["fc_0"].weight[2 * c, n_in - 3 + c, 0] = 1.0        # relu(q_c)
            fc["fc_0"].weight[2 * c + 1, n_in - 3 + c, 0] = -1.0   # relu(-q_c)
        fc["fc_1"].weight[0, :6, 0] = 1.0                          # |q0| + |q1| + |q2|
        fc["fc_2"].weight[0, 0, 0] = 1.0
        fc["fc_out"].weight[0, 0, 0] = -0.5
        fc["fc_out"].bias[0] = r
    net.sdf_decoder.invalidate()


def _exact_points(R, s, stats_idx):
    """bool [R^3]: the lattice points and the refined points."""
    RF = _rf()
    c = RF.lattice_indices(R, s)
    m = np.zeros((R, R, R), bool)
    m[np.ix_(c, c, c)] = True
    m = m.reshape(-1)
    m[stats_idx] = True
    return m


def _no_sign_change_in_inactive_bricks(dense, R, s, act, level):
    RF = _rf()
    c = RF.lattice_indices(R, s)
    for b in zip(*np.nonzero(~act)):
        box = dense[tuple(slice(c[b[a]], c[b[a] + 1] + 1) for a in range(3))]
        inside = box > level
        if inside.any() and not inside.all():
            return False
    return True


def _check_exact(dense, vol, R, s, level, band=None):
    """Lattice and refined points of vol equal dense bit for bit; returns the active mask and the refined indices."""
    RF = _rf()
    c = RF.lattice_indices(R, s)
    lat = dense[np.ix_(c, c, c)]
    act, dil = RF.classify_cpu(lat, level, RF.default_band(R, s) if band is None else band)
    _, idx = RF.refined_points_cpu(dil, R, s)
    exact = _exact_points(R, s, idx)
    assert np.array_equal(vol.reshape(-1)[exact], dense.reshape(-1)[exact])
    return act, dil, idx, exact


@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
@pytest.mark.parametrize("R,s", [(40, 2), (64, 4), (70, 8)])
def test_octahedron_mesh_equals_the_dense_mesh(precision, R, s):
    from list_amd import mesh
    ex, net, img = _executor(precision, mcube_znum=R)
    _octahedron(net)
    dense = ex.predict_grid(img)[0]
    vol = ex.predict_grid(img, refine=s)[0]
    st = ex.last_grid_stats
    d, v = dense.cpu().numpy(), vol.cpu().numpy()
    act, _, idx, _ = _check_exact(d, v, R, s, 0.0)
    assert st["refined"] == len(idx) and st["fraction"] < 1.0
    assert _no_sign_change_in_inactive_bricks(d, R, s, act, 0.0)
    v0, f0 = mesh.marching_cubes(dense)
    v1, f1 = mesh.marching_cubes(vol)
    assert len(f0) > 100
    assert torch.equal(v0, v1) and torch.equal(f0, f1)


@pytest.mark.parametrize("R,s", [(40, 4), (64, 4), (64, 2), (48, 8)])
def test_seeded_model_exact_points_and_sides(R, s):
    """R = 40: the standard path (fewer than 4 x 137^2 points); R >= 48: the projected-perceptual path."""
    ex, net, img = _executor("bf16x3", mcube_znum=R)
    dense = ex.predict_grid(img)[0]
    level = float(dense.median())
    vol = ex.predict_grid(img, refine=s, level=level)[0]
    d, v = dense.cpu().numpy(), vol.cpu().numpy()
    act, dil, idx, exact = _check_exact(d, v, R, s, level)
    assert 0 < len(idx)
    RF = _rf()
    c = RF.lattice_indices(R, s)
    lat = d[np.ix_(c, c, c)]
    filled = ~exact.reshape(R, R, R)
    assert np.isfinite(v[filled]).all()
    for b in zip(*np.nonzero(~act)):
        ext = tuple(slice(c[b[a]], c[b[a] + 1] + 1) for a in range(3))
        side = lat[b[0], b[1], b[2]] > level
        box = v[ext][filled[ext]]
        assert ((box > level) == side).all()


def test_two_runs_identical_and_refine_none_is_dense():
    ex, net, img = _executor("bf16x3", mcube_znum=56)
    dense = ex.predict_grid(img)[0]
    assert torch.equal(ex.predict_grid(img, refine=None)[0], dense)
    a = ex.predict_grid(img, refine=4, level=float(dense.median()))[0]
    b = ex.predict_grid(img, refine=4, level=float(dense.median()))[0]
    assert torch.equal(a, b)


def test_list_test_uses_the_configured_stride():
    ex, net, img = _executor("bf16x3", mcube_znum=48)
    _octahedron(net)
    ex.refine_stride = 4
    pred, _ = ex.test({"rgb_image": img})
    assert ex.last_grid_stats is not None and ex.last_grid_stats["fraction"] < 1.0
    ex.refine_stride = None
    dense_pred, _ = ex.test({"rgb_image": img})
    assert np.array_equal(pred[0].vertices, dense_pred[0].vertices)
    assert np.array_equal(pred[0].faces, dense_pred[0].faces)


def test_test_py_refine_stride(tmp_path):
    out = str(tmp_path / "out") + "/"
    cmd = [sys.executable, os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "test.py"),
           "--model", "network.models.LIST", "--dataset", "datasets.Datasets.SyntheticIM2SDF", "-e", "rf",
           "--output_dir", out, "--mcube_znum", "48", "--vox_res", "32", "--refine_stride", "4", "--save_volume",
           "--testlist_file", ""]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "% of the 110592 grid points (stride 4)" in r.stdout, r.stdout[-3000:]
    objs = [f for f in os.listdir(os.path.join(out, "rf", "test_objs", "synthetic")) if f.endswith("_pred.obj")]
    vols = [f for f in os.listdir(os.path.join(out, "rf", "test_objs", "synthetic")) if f.endswith("_sdf.npy")]
    assert len(objs) == 2 and len(vols) == 2
    v = np.load(os.path.join(out, "rf", "test_objs", "synthetic", vols[0]))
    assert v.shape == (48, 48, 48) and v.dtype == np.float32


def test_sharded_refined_grid_on_a_one_rank_rccl_group():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_child_refine_shard.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["backend"] == "nccl" and d["world"] == 1
    assert d["equal"] and d["stats_equal"] and d["refined"] > 0, d
