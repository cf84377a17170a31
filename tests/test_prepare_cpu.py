"""CPU: the numpy restatement of the training-data preparation (prepare.*_cpu) against analytic fields and plain
loops; prepare_shape's files read back through the file-backed datasets; the new C-ABI symbols."""
import os

import numpy as np
import pytest

from list_amd import prepare as P


# ---- generated meshes (shared with test_prepare_gpu.py) -----------------------------------------------------------------


def box_mesh(lo=-0.5, hi=0.5):
    """The 12-triangle axis-aligned box, outward normals."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def icosphere(sub, r=0.5):
    """An icosahedron subdivided `sub` times, projected on the sphere of radius r, outward normals."""
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(sub):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    v, f = (np.array(v) * r).astype(np.float32), np.array(f, np.int32)
    t = v.astype(np.float64)[f]
    if np.einsum("fi,fi->f", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() < 0:
        f = f[:, ::-1].copy()
    return v, f


def write_meshes(root):
    """Two shapes (a sphere and an off-centre box, as .obj) of oracle/dataset_fixture.py's category, plus one file that
    does not load -> [(cat, shape)] of the good ones."""
    from list_amd.mesh import Mesh
    from oracle import dataset_fixture as DF
    good = [(DF.CAT, "sphere_a"), (DF.CAT, "box_b")]
    v, f = icosphere(2, 0.35)
    meshes = [(v * np.float32(3) + np.float32(1), f), box_mesh(0.2, 1.4)]
    for (cat, shape), (v, f) in zip(good, meshes):
        os.makedirs(os.path.join(root, cat, shape), exist_ok=True)
        Mesh(v, f).export(os.path.join(root, cat, shape, "model.obj"))
    os.makedirs(os.path.join(root, DF.CAT, "broken_c"), exist_ok=True)
    with open(os.path.join(root, DF.CAT, "broken_c", "model.obj"), "w") as fh:
        fh.write("v 0 0 0\nf 1 2 x\n")
    return good


def dataset_over(tmp_path, h5_dir, shapes):
    """FileIM2SDF / FileIM2PointFarthest over prepared files, with oracle/dataset_fixture.py's images and a split list."""
    from list_amd import arguments
    from list_amd.datasets import Datasets as D
    from oracle import dataset_fixture as DF
    image_dir, _ = DF.write_tree(os.path.join(str(tmp_path), "fixture"), [s for _, s in shapes])
    split = os.path.join(str(tmp_path), "split")
    os.makedirs(split, exist_ok=True)
    with open(os.path.join(split, f"{DF.CAT}_train.lst"), "w") as fh:
        fh.write("\n".join(s for _, s in shapes) + "\n")
    cfg = arguments.default_config(cuda=False, split_dir=split + "/", **DF.config_fields(image_dir, h5_dir))
    return D.FileIM2SDF(cfg, "train"), D.FileIM2PointFarthest(cfg, "train")


def box_sdf(p, h=0.5):
    q = np.abs(p.astype(np.float64)) - h
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)


# ---- signed distance ------------------------------------------------------------------------------------------------
def test_signed_distance_cube_matches_the_box_sdf():
    v, f = box_mesh()
    p = np.random.default_rng(0).uniform(-1, 1, (3000, 3)).astype(np.float32)
    sdf, fi, w = P.signed_distance_cpu(v, f, p, with_winding=True)
    assert sdf.dtype == np.float32 and fi.dtype == np.int32
    np.testing.assert_allclose(sdf, box_sdf(p), atol=1e-6, rtol=0)
    inside = np.all(np.abs(p) < 0.5, axis=1)
    np.testing.assert_allclose(w[inside], 1.0, atol=1e-9)
    np.testing.assert_allclose(w[~inside], 0.0, atol=1e-9)


def test_signed_distance_icosphere_against_the_sphere():
    r = 0.4
    v, f = icosphere(4, r)                              # 5120 faces: the facet sag is below 1e-3 * r
    p = np.random.default_rng(1).uniform(-0.6, 0.6, (1500, 3)).astype(np.float32)
    sdf, _, _ = P.signed_distance_cpu(v, f, p)
    exact = np.linalg.norm(p.astype(np.float64), axis=1) - r
    np.testing.assert_allclose(sdf, exact, atol=1.5e-3)
    far = np.abs(exact) > 2e-3
    np.testing.assert_array_equal(np.sign(sdf[far]), np.sign(exact[far]))


def test_signed_distance_on_vertices_edges_faces_and_flat_faces():
    v, f = box_mesh()
    on = np.concatenate([v, (v[f[:, 0]] + v[f[:, 1]]) / 2, (v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) / 3])
    sdf, fi, _ = P.signed_distance_cpu(v, f, on)
    assert np.all(sdf[:8 + 12] == 0) and np.all(np.abs(sdf) < 1e-7) and np.all(fi >= 0)   # centroids round in float32
    # zero-area faces (a repeated corner, three collinear corners) and an out-of-range face: never a NaN, the edges
    # measure them, the bad one is skipped
    v2 = np.concatenate([v, np.array([[0.5, 0.5, 0.5], [2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)])
    f2 = np.array([[8, 8, 8], [9, 10, 11], [0, 1, 50]], np.int32)
    p = np.array([[3, 1, 0], [5, 0, 0], [0.5, 0.5, 1.5], [3, 0, 0]], np.float32)
    sdf, fi, w = P.signed_distance_cpu(v2, f2, p, with_winding=True)
    assert np.all(np.isfinite(sdf)) and np.all(np.isfinite(w)) and np.all(w == 0)
    np.testing.assert_allclose(sdf, [1, 1, 1, 0], atol=1e-7)
    np.testing.assert_array_equal(fi, [1, 1, 0, 1])
    # no valid face at all
    sdf, fi, _ = P.signed_distance_cpu(v, np.array([[0, 1, 99]], np.int32), p)
    assert np.all(np.isinf(sdf) & (sdf > 0)) and np.all(fi == -1)
    with pytest.raises(Exception, match="0 faces"):
        P.signed_distance_cpu(v, np.zeros((0, 3), np.int32), p)


def test_winding_number_of_an_open_cube():
    v, f = box_mesh()
    top = np.all(v[f][:, :, 2] == 0.5, axis=1)        # remove the two triangles of the +z face
    p = np.array([[0, 0, -0.4], [0, 0, -0.2], [0.3, 0.3, -0.3], [0, 0, -0.9], [2, 0, 0]], np.float32)
    sdf, _, w = P.signed_distance_cpu(v, f[~top], p, with_winding=True)
    assert np.all(w[:3] > 0.5) and np.all(sdf[:3] < 0)     # away from the opening: still inside
    assert np.all(w[3:] < 0.5) and np.all(sdf[3:] > 0)
    assert np.all(np.abs(w[:3] - 1) < 0.3)


# ---- boundary samples -----------------------------------------------------------------------------------------------
def test_boundary_samples_pure_normal_and_identity():
    p = np.random.default_rng(2).uniform(-0.5, 0.5, (40000, 3)).astype(np.float32)
    a, b = P.boundary_samples_cpu(p, 0.01, 7), P.boundary_samples_cpu(p.copy(), 0.01, 7)
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert P.boundary_samples_cpu(p, 0.01, 8).tobytes() != a.tobytes()
    assert P.boundary_samples_cpu(p, 0.0, 7).tobytes() == p.tobytes()
    n = ((a.astype(np.float64) - p) / np.float64(np.float32(0.01))).ravel()
    assert abs(n.mean()) < 0.02 and abs(n.var() - 1) < 0.03 and abs((n ** 3).mean()) < 0.05
    assert abs((n ** 4).mean() - 3) < 0.1
    # chi^2 over 20 equiprobable bins of the standard normal
    from scipy.stats import chi2, norm
    edges = norm.ppf(np.linspace(0, 1, 21))
    counts = np.histogram(n, bins=edges)[0]
    expect = len(n) / 20
    assert ((counts - expect) ** 2 / expect).sum() < chi2.ppf(0.999, 19)


# ---- farthest points ------------------------------------------------------------------------------------------------
def _fps_loop(c, k):
    n = len(c)
    m = [float("inf")] * n
    out = [0]
    for _ in range(1, k):
        s = c[out[-1]]
        for j in range(n):
            d = c[j] - s
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if d2 < m[j]:
                m[j] = d2
        best = 0
        for j in range(1, n):
            if m[j] > m[best]:
                best = j
        out.append(best)
    return out


def test_farthest_points_matches_a_plain_loop():
    rng = np.random.default_rng(3)
    c = rng.uniform(-0.5, 0.5, (2, 300, 3)).astype(np.float32)
    c[1, 150:] = c[1, :150]                                  # duplicates: ties go to the smaller index
    pts, idx = P.farthest_points_cpu(c, 300)
    for b in range(2):
        assert idx[b].tolist() == _fps_loop(c[b], 300)
        np.testing.assert_array_equal(pts[b], c[b][idx[b]])
    q = np.repeat(c[0, :3], 4, axis=0)                       # 3 distinct points, K = N
    assert P.farthest_points_cpu(q, 12)[1].tolist() == _fps_loop(q, 12)
    with pytest.raises(Exception, match="K = 13"):
        P.farthest_points_cpu(q, 13)


# ---- files ----------------------------------------------------------------------------------------------------------
def test_scale_mesh_centres_and_normalises():
    v, f = box_mesh(0.2, 1.4)
    v = v * np.array([1, 2, 0.5], np.float32)
    v = np.concatenate([v, np.array([[100, 100, 100]], np.float32)])     # unreferenced: not in the bounds
    m = P.scale_mesh(v, f)
    used = m.vertices[:8].astype(np.float64)
    lo, hi = used.min(axis=0), used.max(axis=0)
    np.testing.assert_allclose((hi + lo) / 2, 0, atol=1e-7)
    assert abs((hi - lo).max() - 1) < 1e-6
    np.testing.assert_array_equal(m.faces, f)


def test_prepare_shape_writes_what_the_datasets_read(tmp_path):
    shapes = write_meshes(str(tmp_path / "raw"))
    out = tmp_path / "sampled_points"
    for cat, shape in shapes:
        files = P.prepare_shape(str(tmp_path / "raw" / cat / shape / "model.obj"),
                                str(tmp_path / "isosurface" / cat / shape), str(out / cat / shape), num_points=6000,
                                n_farthest=5000, seed=1, device=None)
        from list_amd import evaluate as E
        m = E.load_mesh(files["mesh"])
        lo, hi = m.vertices.min(axis=0).astype(np.float64), m.vertices.max(axis=0).astype(np.float64)
        np.testing.assert_allclose((hi + lo) / 2, 0, atol=1e-6)
        assert abs((hi - lo).max() - 1) < 1e-6
        sp = np.load(files["sampled_points"])
        assert sorted(sp.files) == ["grid_points", "query_points_sigma_0.003", "query_points_sigma_0.01",
                                    "query_points_sigma_0.07"]
        assert sp["grid_points"].shape == (6000, 3) and sp["grid_points"].dtype == np.float32
        for s in P.SIGMAS:
            q = sp[f"query_points_sigma_{s}"]
            assert q.shape == (6000, 4) and q.dtype == np.float32
        fp = np.load(files["farthest_pointclouds"])
        assert fp.files == ["points_5000"] and fp["points_5000"].shape == (5000, 3)
        assert fp["points_5000"].dtype == np.float32
    ds_sdf, ds_pf = dataset_over(tmp_path, str(out) + "/", shapes)
    assert len(ds_sdf) == 2 and len(ds_pf) == 2
    for i, (_, shape) in enumerate(shapes):
        it = ds_sdf[i]
        p, val = it["points"].numpy().astype(np.float64), it["values"].numpy()
        if shape.startswith("sphere"):              # vertices on a sphere whose radius scale_mesh set; facet sag < 2%
            from list_amd import evaluate as E
            cat = shapes[i][0]
            r = np.linalg.norm(E.load_mesh(str(tmp_path / "isosurface" / cat / shape / "isosurf_scaled.obj")).vertices,
                               axis=1).max()
            exact, margin = np.linalg.norm(p, axis=1) - r, 0.02 * r
        else:
            exact, margin = box_sdf(p), 5e-3
        far = np.abs(exact) > margin
        assert far.sum() > 20                        # ~200 samples per item, most of them near the surface
        np.testing.assert_array_equal(np.sign(val[far]), np.sign(exact[far]))
        assert it["occ"].shape[0] == 1 and ds_pf[i]["pc"].shape == (5000, 3)


def test_cli_reports_a_bad_mesh_and_skips_existing_output(tmp_path):
    shapes = write_meshes(str(tmp_path / "raw"))
    argv = ["--input_dir", str(tmp_path / "raw") + "/", "--output_dir", str(tmp_path / "out"), "--categories",
            shapes[0][0], "--file_path_glob", "/*/model.obj", "--num_points", "600", "--n_farthest", "100",
            "--device", "cpu"]
    import contextlib
    import io
    buf, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
        assert P.main(argv) == 0
        assert P.main(argv) == 0
    out = buf.getvalue()
    assert "prepared 2, skipped 0, failed 1" in out and "prepared 0, skipped 2, failed 1" in out
    assert "broken_c" in err.getvalue()
    for cat, shape in shapes:
        assert os.path.exists(tmp_path / "out" / "isosurface" / cat / shape / "isosurf_scaled.obj")
        assert os.path.exists(tmp_path / "out" / "sampled_points" / cat / shape / "farthest_pointclouds.npz")


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_data_symbols():
    import __graft_entry__ as ge
    ge.build()
    lib = P.load()
    assert lib.list_data_signed_distance_workspace_bytes(1000) == 80 * 1000
    assert lib.list_data_signed_distance_workspace_bytes(0) == 0 and b"0 faces" in lib.list_data_last_error()
    # argument checks come before any HIP call
    assert lib.list_data_farthest_points(None, 1, 10, 11, None, None) == -2
    assert b"K = 11" in lib.list_data_last_error()
    assert lib.list_data_farthest_points(None, 1, 70000, 5, None, None) == -2
    assert lib.list_data_signed_distance(None, 8, None, 0, None, 1, None, 0, None, None, None, None) == -2
