"""GPU: the training-data preparation in HIP (include/list_data.h, prepare.*) against its numpy restatement; the
`python -m list_amd.prepare` command line end to end, read back through the file-backed datasets."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_prepare_cpu import box_mesh, dataset_over, icosphere, write_meshes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def _P():
    from list_amd import prepare
    return prepare


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _second_gap(v, f, p):
    """The gap between the nearest and the second-nearest face distance of every point: every face's distance as
    signed_distance_cpu measures it for that face alone (fp32 d2, one sqrt; an invalid face is infinitely far), all
    faces of a chunk of points at once."""
    from list_amd import prepare as P
    v, f, p = np.asarray(v, np.float32), np.asarray(f, np.int32).reshape(-1, 3), np.asarray(p, np.float32)
    if len(f) < 2:
        return np.full(len(p), np.inf)
    ok = np.all((f >= 0) & (f < len(v)), axis=1)
    t = v[np.where(ok[:, None], f, 0)]
    a, b, c = ([t[None, :, j, k] for k in range(3)] for j in range(3))
    ab, ac, bc = ([y[k] - x[k] for k in range(3)] for x, y in ((a, b), (a, c), (b, c)))
    n = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
    flat = (n[0] == 0) & (n[1] == 0) & (n[2] == 0)
    gap = np.empty(len(p))
    chunk = max(1, (1 << 19) // len(f))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(0, len(p), chunk):
            px, py, pz = (p[s:s + chunk, k:k + 1] for k in range(3))
            d2 = P._tri_d2(px, py, pz, a, b, c, ab, ac)
            e = np.minimum(np.minimum(P._seg_d2(px, py, pz, a, ab), P._seg_d2(px, py, pz, a, ac)),
                           P._seg_d2(px, py, pz, b, bc))
            d2 = np.where(flat, e, d2)
            d2 = np.where(ok[None, :] & ~np.isnan(d2), d2, np.float32(np.inf))
            d = np.partition(np.sqrt(d2).astype(np.float64), 1, axis=1)
            gap[s:s + chunk] = d[:, 1] - d[:, 0]
    return gap


def _check_sdf(v, f, p, check_faces=True, ref=None):
    """ref: (sdf, face_idx, winding, second gap) of signed_distance_cpu for these points, when the caller shares it."""
    P = _P()
    sdf, fi, w = P.signed_distance(_t(v), _t(f), _t(p), with_winding=True)
    sdf, fi, w = sdf.cpu().numpy(), fi.cpu().numpy(), w.cpu().numpy()
    rs, rf, rw = ref[:3] if ref else P.signed_distance_cpu(v, f, p, with_winding=True)
    np.testing.assert_allclose(np.abs(sdf), np.abs(rs), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(w, rw, atol=1e-4)
    far = np.abs(rw - 0.5) > 1e-3
    np.testing.assert_array_equal(np.sign(sdf[far]), np.sign(rs[far]))
    if check_faces:
        sep = (ref[3] if ref else _second_gap(v, f, p)) > 1e-6
        np.testing.assert_array_equal(fi[sep], rf[sep])
    return sdf, fi, w


@pytest.mark.parametrize("Q,sub", [(1000, 2), (777, 1), (1, 0), (4097, 1), (600000, 2), (1100000, 1)])
def test_signed_distance_icosphere(Q, sub):
    v, f = icosphere(sub, 0.35)
    rng = np.random.default_rng(Q)
    p = rng.uniform(-0.6, 0.6, (Q, 3)).astype(np.float32)
    if Q > 5000:                                       # 2 and 4 points per lane: distances on a subset
        P = _P()
        sdf, fi, _ = P.signed_distance(_t(v), _t(f), _t(p))
        sel = rng.choice(Q, 3000, replace=False)
        rs, rf, _ = P.signed_distance_cpu(v, f, p[sel])
        np.testing.assert_allclose(sdf.cpu().numpy()[sel], rs, rtol=1e-6, atol=1e-7)
        return
    _check_sdf(v, f, p, check_faces=len(f) <= 400)


# list_data_signed_distance: R = 4 when ceil(Q / 1024) >= 1024, else R = 2 when ceil(Q / 512) >= 1024, else R = 1
SDF_BORDERS = {523_776: 1, 523_777: 2, 1_047_552: 2, 1_047_553: 4}


@pytest.fixture(scope="module")
def border_reference():
    """The 20-face icosphere, max(SDF_BORDERS) points and their host answers, computed once: a border Q takes a prefix."""
    from list_amd import evaluate as E
    v, f = icosphere(0, 0.35)
    p = E.box_samples_cpu(max(SDF_BORDERS), -0.6, 0.6, 7).astype(np.float32)
    return v, f, p, _P().signed_distance_cpu(v, f, p, with_winding=True) + (_second_gap(v, f, p),)


@pytest.mark.parametrize("Q", sorted(SDF_BORDERS))
def test_signed_distance_dispatch_borders(border_reference, Q):
    """sdf_kernel<R> where R changes: Q = 523 776 -> R = 1 and 1 047 552 -> R = 2 (2046 full workgroups each),
    523 777 -> R = 2 and 1 047 553 -> R = 4 (1024 workgroups, the last with one point and every other slot past Q).
    |sdf|, winding, sign and face index of every point."""
    assert (4 if -(-Q // 1024) >= 1024 else 2 if -(-Q // 512) >= 1024 else 1) == SDF_BORDERS[Q]
    v, f, p, ref = border_reference
    sdf, fi, w = _check_sdf(v, f, p[:Q], ref=tuple(r[:Q] for r in ref))
    assert sdf.shape == fi.shape == w.shape == (Q,)
    gap = ref[3][:Q]
    # a point nearest to an edge or a corner has two faces at the same distance: the face is checked on the others
    assert np.count_nonzero(gap > 1e-6) > Q // 4 and np.count_nonzero(ref[0][:Q] < 0) > Q // 50


def test_signed_distance_single_face_and_odd_tiles():
    rng = np.random.default_rng(3)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    _check_sdf(v, np.array([[0, 1, 2]], np.int32), rng.uniform(-1, 1, (513, 3)).astype(np.float32))
    # F = 257: one face past a tile; a random triangle soup
    v = rng.uniform(-0.5, 0.5, (300, 3)).astype(np.float32)
    f = rng.integers(0, 300, (257, 3)).astype(np.int32)
    _check_sdf(v, f, rng.uniform(-0.6, 0.6, (600, 3)).astype(np.float32))


def test_signed_distance_bad_and_flat_faces():
    v, f = box_mesh()
    rng = np.random.default_rng(4)
    extra = np.array([[0, 1, 99], [-1, 2, 3], [0, 0, 0], [1, 1, 2], [0, 1, 8]], np.int32)   # out of range, flat
    v = np.concatenate([v, np.array([[0.25, -0.5, -0.5]], np.float32)])                      # 8: on edge 0-1
    f2 = np.concatenate([f[:6], extra, f[6:]])
    p = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
    p[:8] = v[:8]                                    # on vertices
    sdf, fi, _ = _check_sdf(v, f2, p)
    assert np.all(np.isfinite(sdf)) and np.all(fi >= 0) and not np.any(np.isin(fi, [6, 7]))


def test_signed_distance_bit_identical_runs():
    v, f = icosphere(3, 0.3)
    p = _t(np.random.default_rng(5).uniform(-0.5, 0.5, (20000, 3)).astype(np.float32))
    P = _P()
    a = [x.cpu().numpy() for x in P.signed_distance(_t(v), _t(f), p, with_winding=True)]
    b = [x.cpu().numpy() for x in P.signed_distance(_t(v), _t(f), p, with_winding=True)]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("sigma", [0.0, 0.003, 0.07])
def test_boundary_samples_bit_identical(sigma):
    P = _P()
    p = np.random.default_rng(6).uniform(-0.5, 0.5, (30001, 3)).astype(np.float32)
    got = P.boundary_samples(_t(p), sigma, seed=11).cpu().numpy()
    assert got.tobytes() == P.boundary_samples_cpu(p, sigma, seed=11).tobytes()


@pytest.mark.parametrize("B,N,K", [(1, 1, 1), (1, 1000, 1000), (3, 5000, 300), (32, 2048, 64), (1, 17000, 500),
                                   (3, 50000, 200), (1, 65536, 20)])
def test_farthest_points_equal(B, N, K):
    P = _P()
    rng = np.random.default_rng(B * N + K)
    c = rng.uniform(-0.5, 0.5, (B, N, 3)).astype(np.float32)
    pts, idx = P.farthest_points(_t(c), K)
    rp, ri = P.farthest_points_cpu(c, K)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(pts.cpu().numpy(), rp)


def test_farthest_points_duplicates():
    P = _P()
    rng = np.random.default_rng(8)
    base = rng.uniform(-0.5, 0.5, (40, 3)).astype(np.float32)
    c = np.stack([np.concatenate([base, base, base[:20]]), np.repeat(base[:5], 20, axis=0)[:100]])
    for K in (50, 100):
        _, idx = P.farthest_points(_t(c), K)
        np.testing.assert_array_equal(idx.cpu().numpy(), P.farthest_points_cpu(c, K)[1])


def test_error_paths_raise_with_the_library_message():
    from list_amd import hip
    P = _P()
    v, _ = box_mesh()
    with pytest.raises(hip.ListError, match="0 faces"):
        P.signed_distance(_t(v), _t(np.zeros((0, 3), np.int32)), _t(v))
    with pytest.raises(hip.ListError, match="K = 11"):
        P.farthest_points(_t(np.zeros((10, 3), np.float32)), 11)


def test_cli_on_the_gpu_matches_the_numpy_path(tmp_path):
    P = _P()
    src = tmp_path / "raw"
    shapes = write_meshes(str(src))
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "list_amd.prepare", "--input_dir", str(src) + "/", "--output_dir", str(out),
           "--categories", *sorted({c for c, _ in shapes}), "--file_path_glob", "/*/model.obj",
           "--num_points", "6000", "--n_farthest", "5000", "--device", DEV]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prepared 2, skipped 0, failed 1" in r.stdout, r.stdout + r.stderr
    ds_sdf, ds_pf = dataset_over(tmp_path, str(out) + "/sampled_points/", shapes)
    assert len(ds_sdf) == 2 and len(ds_pf) == 2
    for i in range(2):
        it = ds_sdf[i]
        assert it["points"].shape[1] == 3 and np.all(np.isfinite(it["values"].numpy()))
    # one shape again on the numpy path: the same files within the tolerances
    cat, shape = shapes[0]
    cpu_dir = tmp_path / "cpu"
    P.prepare_shape(str(src / cat / shape / "model.obj"), str(cpu_dir), str(cpu_dir), 6000, n_farthest=5000,
                    device=None)
    gpu = np.load(str(out / "sampled_points" / cat / shape / "sampled_points.npz"))
    cpu = np.load(str(cpu_dir / "sampled_points.npz"))
    assert sorted(gpu.files) == sorted(cpu.files)
    same = np.all(gpu["grid_points"] == cpu["grid_points"], axis=1)
    assert same.mean() > 0.999
    for key in gpu.files:
        if key.startswith("query"):
            g, c = gpu[key][same], cpu[key][same]
            np.testing.assert_array_equal(g[:, :3], c[:, :3])
            np.testing.assert_allclose(np.abs(g[:, 3]), np.abs(c[:, 3]), rtol=1e-6, atol=1e-7)
            _, _, w = P.signed_distance_cpu(*_mesh(cpu_dir), c[:, :3], with_winding=True)
            far = np.abs(w - 0.5) > 1e-3
            np.testing.assert_array_equal(np.sign(g[far, 3]), np.sign(c[far, 3]))
    if same.all():
        g, c = (np.load(str(d / "farthest_pointclouds.npz"))["points_5000"]
                for d in (out / "sampled_points" / cat / shape, cpu_dir))
        np.testing.assert_array_equal(g, c)
    # a second run skips every prepared shape
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "prepared 0, skipped 2, failed 1" in r.stdout, r.stdout + r.stderr


def _mesh(d):
    from list_amd import evaluate as E
    m = E.load_mesh(os.path.join(str(d), "isosurf_scaled.obj"))
    return m.vertices, m.faces
