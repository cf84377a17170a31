"""GPU: the mesh evaluation in HIP (include/list_eval.h, evaluate.*) against its numpy restatement and cKDTree;
LIST.eval / LIST.test(eval_pred=True) and test.py --eval_pred end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_eval_cpu import KEYS, SHAPES, _chi2_ok, _field, _on_faces, mc_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def _E():
    from list_amd import evaluate
    return evaluate


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nn_brute(src, dst):
    d2 = ((src[:, None, :].astype(np.float32) - dst[None, :, :].astype(np.float32)) ** 2)
    d2 = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
    return np.argmin(d2, axis=1)                                  # first minimum: the smallest j


@pytest.mark.parametrize("N,M", [(1000, 1000), (777, 3001), (5000, 257), (1, 1), (300, 1), (4097, 513)])
def test_nn_distance(N, M):
    E = _E()
    rng = np.random.default_rng(N * 7 + M)
    src = rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)
    dst = rng.uniform(-0.5, 0.5, (M, 3)).astype(np.float32)
    d, i = E.nn_distance(_t(src), _t(dst))
    ref_d, _ = E.nn_distance_cpu(src, dst)
    np.testing.assert_allclose(d.cpu().numpy(), ref_d, rtol=1e-6, atol=1e-12)
    np.testing.assert_array_equal(i.cpu().numpy(), _nn_brute(src, dst))


def test_nn_distance_duplicates():
    E = _E()
    rng = np.random.default_rng(1)
    base = rng.uniform(-0.5, 0.5, (100, 3)).astype(np.float32)
    dst = np.concatenate([base, base, base[:50]])                   # every point three or two times
    src = np.concatenate([base, base + np.float32(1e-3)])
    d, i = E.nn_distance(_t(src), _t(dst))
    np.testing.assert_array_equal(i.cpu().numpy(), _nn_brute(src, dst))
    assert np.all(d.cpu().numpy()[:100] == 0) and np.all(i.cpu().numpy()[:100] == np.arange(100))


def test_nn_distance_large():
    E = _E()
    rng = np.random.default_rng(2)
    src = rng.uniform(-0.5, 0.5, (1_000_000, 3)).astype(np.float32)
    dst = rng.uniform(-0.5, 0.5, (100_000, 3)).astype(np.float32)
    d, i = E.nn_distance(_t(src), _t(dst))
    ref_d, ref_i = E.nn_distance_cpu(src, dst)
    np.testing.assert_allclose(d.cpu().numpy(), ref_d, rtol=1e-6, atol=1e-12)
    got_i = i.cpu().numpy()
    diff = np.flatnonzero(got_i != ref_i)                        # only where two dst points are equally near
    if diff.size:
        assert diff.size < 10
        np.testing.assert_array_equal(got_i[diff], _nn_brute(src[diff], dst))


MESHES = {name: (lambda name=name: mc_mesh(name, 48)) for name in SHAPES}
MESHES["sphere256"] = lambda: mc_mesh("sphere", 256)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_mesh_contains_bit_exact(name):
    E = _E()
    v, f = MESHES[name]()
    q = E.box_samples_cpu(200_000, -0.5, 0.5, seed=11)
    # points on the grid of the hash's cells and on the mesh's vertices too: the ties of the strict rules
    q = np.concatenate([q, v[::7].astype(np.float64), np.stack(np.meshgrid(*[np.linspace(-0.31, 0.31, 24)] * 3,
                                                                           indexing="ij"), -1).reshape(-1, 3)])
    vt, ft, qt = _t(v), _t(f), _t(q)
    for rot in (None, E.rotation_matrix((0.3, -1.1, 2.0)), E.rotation_matrix(E.EULER_RETRIES[0])):
        ci, hi = E.mesh_contains(vt, ft, qt, rot=rot)
        ri, rh = E.mesh_contains_cpu(v, f, q, rot=rot)
        np.testing.assert_array_equal(ci.cpu().numpy(), ri)
        np.testing.assert_array_equal(hi.cpu().numpy(), rh)
    o, h = E.implicit_waterproofing(vt, ft, qt)
    ro, rh = E.implicit_waterproofing_cpu(v, f, q)
    np.testing.assert_array_equal(o.cpu().numpy(), ro)
    np.testing.assert_array_equal(h.cpu().numpy(), rh)


def test_waterproofing_open_mesh_bit_exact():
    E = _E()
    v, f = mc_mesh("sphere", 40)
    f_open = f[~np.all(v[f][:, :, 2] > 0.27, axis=1)]
    rng = np.random.default_rng(0)
    q = np.concatenate([np.c_[rng.uniform(-0.03, 0.03, (200, 2)), rng.uniform(-0.2, 0.2, 200)],
                        E.box_samples_cpu(50000, -0.5, 0.5, 1)])
    _, h0 = E.mesh_contains(_t(v), _t(f_open), _t(q))
    assert h0.cpu().numpy()[:200].all()
    o, h = E.implicit_waterproofing(_t(v), _t(f_open), _t(q))
    ro, rh = E.implicit_waterproofing_cpu(v, f_open, q)
    np.testing.assert_array_equal(o.cpu().numpy(), ro)
    np.testing.assert_array_equal(h.cpu().numpy(), rh)
    assert o.cpu().numpy()[:200].all()


def test_wide_triangles_bit_exact():
    """A closed box of 12 triangles: every triangle spans the whole hash (the wide list)."""
    E = _E()
    v = np.array([[x, y, z] for x in (-0.3, 0.3) for y in (-0.2, 0.25) for z in (-0.35, 0.3)], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    q = _E().box_samples_cpu(100_000, -0.5, 0.5, 4)
    for res in (512, 37):
        ci, hi = E.mesh_contains(_t(v), _t(f), _t(q), hash_res=res)
        ri, rh = E.mesh_contains_cpu(v, f, q, hash_res=res)
        np.testing.assert_array_equal(ci.cpu().numpy(), ri)
        np.testing.assert_array_equal(hi.cpu().numpy(), rh)
    inside = np.all((q > [-0.3, -0.2, -0.35]) & (q < [0.3, 0.25, 0.3]), axis=1)
    np.testing.assert_array_equal(ri, inside)


def test_sample_surface():
    E = _E()
    v, f = mc_mesh("torus", 64)
    f = np.concatenate([[[0, 0, 1]], f, [[7, 7, 7]]]).astype(np.int32)
    n = 300_000
    p, fi = E.sample_surface(_t(v), _t(f), n, seed=5)
    p2, fi2 = E.sample_surface(_t(v), _t(f), n, seed=5)
    assert torch.equal(p, p2) and torch.equal(fi, fi2)
    p, fi = p.cpu().numpy(), fi.cpu().numpy().astype(np.int64)
    rp, rfi = E.sample_surface_cpu(v, f, n, seed=5)
    same = fi == rfi
    assert same.mean() >= 0.9999
    np.testing.assert_allclose(p[same], rp[same], rtol=0, atol=1e-6)
    assert not np.isin(fi, [0, len(f) - 1]).any()
    dist, inside = _on_faces(v, f, p.astype(np.float64), fi)
    assert dist < 1e-6 and inside
    assert _chi2_ok(v, f, fi, n)


def test_uniform_torch_matches_numpy():
    E = _E()
    c = torch.arange(100_000, dtype=torch.int64, device=DEV)
    np.testing.assert_array_equal(E._uniform_torch(123, c).cpu().numpy(),
                                  E.uniform_cpu(123, np.arange(100_000, dtype=np.uint64)))


@pytest.mark.parametrize("pair", [("sphere", "sphere"), ("torus", "two_spheres"), ("sphere", "torus")])
def test_eval_mesh_gpu_vs_cpu(pair):
    E = _E()
    from list_amd import mesh as M
    mp, mg = M.Mesh(*mc_mesh(pair[0], 64)), M.Mesh(*mc_mesh(pair[1], 48))
    n = 20000
    g = E.eval_mesh(mp, mg, -0.5, 0.5, n_points=n, seed=1, device=DEV)
    c = E.eval_mesh_cpu(mp, mg, -0.5, 0.5, n_points=n, seed=1)
    assert set(g) == set(c) == KEYS | {"iou"}
    assert g["iou"] == c["iou"]
    for k in KEYS:
        if k.startswith(("precision", "recall")):
            assert abs(g[k] - c[k]) * n <= 3, (k, g[k], c[k])        # a few points within fp32 rounding of p
    for k in ("completeness", "accuracy", "completeness2", "accuracy2", "chamfer_l2"):
        assert g[k] == pytest.approx(c[k], rel=1e-3), k


def test_error_paths():
    E = _E()
    from list_amd import hip
    v = _t(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32))
    flat = _t(np.array([[0, 1, 2]], dtype=np.int32))
    empty = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    q = _t(np.zeros((5, 3)))
    for call in (lambda: E.nn_distance(v, v[:0]), lambda: E.sample_surface(v, empty, 10),
                 lambda: E.mesh_contains(v, empty, q), lambda: E.mesh_contains(v, flat, q),
                 lambda: E.sample_surface(v, _t(np.array([[0, 0, 1]], dtype=np.int32)), 10),
                 lambda: E.mesh_contains(v, _t(np.array([[0, 1, 3]], dtype=np.int32)), q, hash_res=0)):
        with pytest.raises(hip.ListError) as e:
            call()
        assert e.value.code == hip.ERR_SHAPE
    # out-of-range faces are never read: they are skipped like degenerate ones
    bad = _t(np.array([[0, 1, 3], [0, 2, 99], [-1, 2, 3], [1, 2, 3]], dtype=np.int32))
    p, fi = E.sample_surface(v, bad, 1000)
    assert set(fi.cpu().numpy().tolist()) <= {0, 3}
    torch.cuda.synchronize()


def _seeded_executor(res=64):
    from oracle import fill
    from list_amd import arguments, utils
    from list_amd.train import _Module
    cfg = arguments.default_config(vox_res=32, train_batch_size=1, mcube_znum=res)
    cfg.device = torch.device(DEV)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(DEV)
    return utils.get_class("network.executors.LIST")(cfg, _Module(net))


def test_list_test_eval_pred():
    from oracle import synth
    from list_amd import mesh as M
    ex = _seeded_executor()
    gt = M.Mesh(*mc_mesh("sphere", 48))
    img = torch.from_numpy(synth.uniform(78, (1, 3, 64, 64)))
    # the seeded weights give no particular shape: score the sphere against itself through eval, and the model's
    # prediction through test() -- whatever its mesh, the dict must be complete and finite, or {} for no surface
    d = ex.eval(gt, gt)
    assert set(d) == KEYS | {"iou"} and d["iou"] == 1.0
    (pred, _, _), score = ex.test({"rgb_image": img, "gt_mesh": gt}, eval_pred=True)
    if len(pred.vertices) >= 10:
        assert set(score) == KEYS | {"iou"}
        assert all(np.isfinite(v) for k, v in score.items() if k != "iou")
    else:
        assert score == {}
    with pytest.raises(ValueError):
        ex.eval(gt, None)


def test_test_py_eval_pred(tmp_path):
    from oracle import dataset_fixture as DF
    from list_amd import mesh as M
    shapes = ["1006be65e7bc937e9141f9b58470d646"]
    image_dir, h5_dir = DF.write_tree(str(tmp_path / "data"), shapes)
    from PIL import Image
    from oracle import synth
    for cam in range(DF.N_VIEWS):                   # the encoders want more than the fixture's 20^2 pixels
        a = (synth.uniform(90 + cam, (64, 64, 4)) * 256).astype(np.uint8)
        Image.fromarray(a, "RGBA").save(os.path.join(image_dir, DF.CAT, shapes[0], "easy", f"{cam:02d}.png"))
    split_dir = tmp_path / "splits"
    split_dir.mkdir()
    (split_dir / f"{DF.CAT}_test.lst").write_text(shapes[0] + "\n")
    mesh_dir = str(tmp_path / "mesh") + "/"
    os.makedirs(os.path.join(mesh_dir, DF.CAT, shapes[0]))
    M.Mesh(*mc_mesh("sphere", 32)).export(os.path.join(mesh_dir, DF.CAT, shapes[0], "isosurf_scaled.obj"))
    testlist = tmp_path / "testlist.lst"
    testlist.write_text(f"{DF.CAT} {shapes[0]} 0\n{DF.CAT} {shapes[0]} 1\n")
    out = str(tmp_path / "out") + "/"
    cmd = [sys.executable, os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "test.py"),
           "--model", "network.models.LIST", "--dataset", "datasets.Datasets.FileIM2SDF", "-e", "ev",
           "--image_dir", image_dir, "--h5_dir", h5_dir, "--split_dir", str(split_dir) + "/", "--mesh_dir", mesh_dir, "--catlist", DF.CAT,
           "--testlist_file", str(testlist), "--output_dir", out, "--mcube_znum", "48", "--vox_res", "32",
           "--eval_pred"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    csv_path = os.path.join(out, "ev", "test_objs", DF.CAT + ".csv")
    assert os.path.exists(csv_path), r.stdout[-3000:]
    rows = open(csv_path).read().strip().splitlines()
    assert rows[0].split(",")[:2] == ["", "ID"]
    assert rows[-1].split(",")[1] == "Mean"
    assert len(rows) == 4, rows
    assert "Mean" in r.stdout
