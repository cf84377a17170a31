"""CPU: the numpy restatement of the vertex-clustering simplifier (simplify.simplify_cpu) by hand, against a plain Python
loop with fractions.Fraction, and by its properties on marching-cubes meshes; csrc/simplify_math.h compiled for the host
against the numpy rule; the C ABI of include/list_simplify.h; refusals, the parser's flag, Mesh.simplify.  Every
comparison is exact: integers, or floats as bytes."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H        # noqa: E402
import _simplify_cases as SC     # noqa: E402

HAND = SC.hand_cases()


def _S():
    from list_amd import simplify
    return simplify


@pytest.fixture(scope="module")
def mc_meshes():
    """name -> (verts, faces) of the CPU marching cubes of SC.FIELDS, read-only."""
    from list_amd import mesh
    out = {}
    for name, field in SC.FIELDS.items():
        v, f = mesh.marching_cubes_cpu(field())
        v.setflags(write=False)
        f.setflags(write=False)
        out[name] = (v, f)
    return out


# ---- by hand ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HAND))
def test_hand_worked_cases(name):
    c = HAND[name]
    SC.check_case(c, _S().simplify_cpu(c["verts"], c["faces"], c["cells"], c["bb_min"], c["bb_max"]))


def test_hand_worked_cases_through_simplify_and_other_dtypes():
    """simplify sends host inputs to the restatement; lists, int64 faces and float64 vertices are converted."""
    S = _S()
    c = HAND["quad_sheet"]
    SC.check_case(c, S.simplify(c["verts"].astype(np.float64), c["faces"].astype(np.int64).tolist(), c["cells"],
                                c["bb_min"], c["bb_max"]))
    import torch
    SC.check_case(c, S.simplify(torch.from_numpy(c["verts"]), torch.from_numpy(c["faces"]), c["cells"], c["bb_min"],
                                c["bb_max"]))


def test_one_cell_and_slabs_empty_the_mesh(mc_meshes):
    """cells = 1: one cluster.  (1,1,4): four slabs, and no triangle of the sphere has its corners in three of them."""
    S = _S()
    v, f = mc_meshes["sphere32"]
    for cells, K in ((1, 1), ((1, 1, 4), 4)):
        ov, of, info = S.simplify_cpu(v, f, cells)
        assert ov.shape == (0, 3) and of.shape == (0, 3) and info["clusters"] == K
        assert info["degenerate_faces"] == len(f) and (info["vertex_map"] == -1).all()


# ---- the independent oracle -----------------------------------------------------------------------------------------
def check_against_oracle(v, f, cells, lo, hi):
    ov, of, info = _S().simplify_cpu(v, f, cells, lo, hi)
    rv, rf, rmap, rtot = SC.oracle(v, f, cells, lo, hi)
    assert ov.tobytes() == rv.tobytes() and ov.shape == rv.shape
    assert np.array_equal(of, rf) and info["vertex_map"].tolist() == rmap
    for k, x in rtot.items():
        assert info[k] == x, k
    return ov, of, info


@pytest.mark.parametrize("seed,V,F,cells,lo,hi", [
    (1, 400, 900, 4, -0.5, 0.5), (2, 400, 900, (3, 5, 2), -0.5, 0.5), (3, 1000, 3000, 8, (-0.5, -0.6, -0.7), (0.5, 0.7, 0.9)),
    (4, 50, 200, 1024, -0.5, 0.5), (5, 3000, 6000, 2, -0.3, 0.3), (6, 7, 3, 3, 0.0, 1.0 / 3.0), (7, 2000, 4000, (1, 7, 1), -1e-3, 1e3)])
def test_restatement_equals_the_fraction_loop_on_random_meshes(seed, V, F, cells, lo, hi):
    v, f = SC.random_mesh(V, F, seed)
    _, _, info = check_against_oracle(v, f, cells, lo, hi)
    if V >= 8 and F >= 8:
        assert info["invalid_verts"] >= 1 and info["invalid_faces"] >= 1


def test_restatement_equals_the_fraction_loop_on_a_sphere(mc_meshes):
    """... and there the counts are what they are for this sphere (r = 0.3 at the origin, 32^3 samples of [-0.5, 0.5]^3:
    1608 vertices, 3212 faces).  The issue quotes 1744 / 3484 -> 108 / 212 and 350 / 696 for its prototype's sphere without
    giving its radius or centre; no centred sphere on this grid has 1744 vertices (the counts step 1704, 1800 around
    r = 0.31), so the counts pinned here are those of the suite's own sphere, each confirmed by the Fraction loop."""
    v, f = mc_meshes["sphere32"]
    assert (len(v), len(f)) == (1608, 3212)
    for cells, want in ((8, (104, 204)), (16, (320, 636))):
        ov, of, _ = check_against_oracle(v, f, cells, -0.5, 0.5)
        assert (len(ov), len(of)) == want


# ---- properties on marching-cubes meshes ------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [8, 16])
@pytest.mark.parametrize("name", list(SC.FIELDS))
def test_properties_on_marching_cubes_meshes(mc_meshes, name, cells):
    S = _S()
    v, f = mc_meshes[name]
    assert (SC.edge_uses(f) == 2).all()                                       # the input is closed
    ov, of, info = S.simplify_cpu(v, f, cells)
    assert info["invalid_verts"] == 0 and info["invalid_faces"] == 0
    assert info["n_faces"] + info["degenerate_faces"] == len(f)
    # a vertex map sends a closed surface to a mod-2 cycle
    uses = SC.edge_uses(of)
    assert (uses % 2 == 0).all()
    same, opposite = SC.oriented_duplicates_and_opposites(of)
    if name == "shell64":
        assert opposite > 0 and same == 0 and uses.max() >= 4                 # the two sheets fold onto each other
    else:
        assert (uses == 2).all() and same == 0 and opposite == 0
    # vertex and representative share a cell
    vmap = info["vertex_map"]
    m = vmap >= 0
    cell = 1.0 / cells
    bound = cell + float(np.spacing(np.float32(0.5)))
    d = np.abs(v[m].astype(np.float64) - ov[vmap[m]].astype(np.float64))
    print(f"{name} cells={cells}: {len(v)} -> {len(ov)} vertices, {len(f)} -> {len(of)} faces, "
          f"max |v - p| = {d.max() / cell:.3f} cells")
    assert (d <= bound).all()
    assert len(ov) <= info["clusters"] <= min(len(v), cells ** 3)
    assert (np.bincount(vmap[m], minlength=len(ov)) >= 1).all() and of.min() >= 0 and of.max() == len(ov) - 1
    # the order of the input vertices does not matter; the faces follow the input face order
    pv, pf, perm = SC.permuted(v, f, seed=cells)
    qv, qf, qinfo = S.simplify_cpu(pv, pf, cells)
    assert qv.tobytes() == ov.tobytes() and np.array_equal(qf, of)
    assert np.array_equal(qinfo["vertex_map"], vmap[perm])


# ---- the shared header on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return SC.build_host(tmp_path_factory.mktemp("simplify_host"))


@pytest.mark.parametrize("cells,lo,hi", [(8, -0.5, 0.5), ((3, 1024, 7), (-0.5, -0.25, 0.0), (0.5, 0.3, 1e-3)), (1, -1.0, 2.0),
                                         (1000, 0.1, 0.7), (1024, -0.5, 0.5)])
def test_header_on_the_host_equals_the_numpy_rule(host_exe, tmp_path, cells, lo, hi):
    """Keys, q and p of csrc/simplify_math.h -- the code the kernels run -- exactly equal to simplify.py's, on random
    doubles and on the edges: cell boundaries and their float32 neighbours, lo, hi, far outside, zeros, denormals,
    non-finite values; sums at both ends of their range and with every kind of remainder."""
    S = _S()
    R, lo3, inv, cell = S.grid(cells, lo, hi)
    hi3 = np.broadcast_to(np.asarray(hi, dtype=np.float64), (3,))
    rng = np.random.default_rng(int(R.sum()))
    n = 4000
    v = (lo3 + (hi3 - lo3) * rng.uniform(-0.2, 1.2, (n, 3))).astype(np.float32)
    edges = []
    for a in range(3):
        b = (lo3[a] + np.arange(0, R[a] + 1, max(1, R[a] // 64)) * cell[a]).astype(np.float32)      # cell boundaries
        col = np.concatenate([b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf)),
                              np.float32([lo3[a], hi3[a], 0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38, np.nan, np.inf, -np.inf])])
        e = np.tile(v[:1], (len(col), 1))
        e[:, a] = col
        edges.append(e)
    v = np.concatenate([v] + edges).astype(np.float32)
    K = 3000
    cn = rng.integers(1, 2 ** 31 - 1, K)
    cn[:200] = rng.integers(1, 9, 200)
    cn[200], cn[201], cn[202] = 1, 2 ** 31 - 1, 3
    frac = rng.random((K, 3))
    frac[:50], frac[50:100] = 0.0, 1.0
    cS = np.minimum((cn[:, None] * (frac * 2.0 ** 30)).astype(np.int64) + rng.integers(0, 2, (K, 3)), cn[:, None] * 2 ** 30)
    ci = np.stack([rng.integers(0, R[a], K) for a in range(3)], axis=1).astype(np.int32)
    valid, i, q, key, pts = SC.run_host(host_exe, tmp_path, v, R, lo3, inv, cell, cS, cn, ci)
    rvalid, ri, rq, rkey = S.vertex_cells(v, R, lo3, inv)
    assert np.array_equal(valid != 0, rvalid) and (~rvalid).sum() >= 9
    assert np.array_equal(i[rvalid], ri[rvalid]) and np.array_equal(q[rvalid], rq[rvalid])
    assert np.array_equal(key[rvalid].astype(np.int64), rkey[rvalid])
    assert q[rvalid].min() == 0 and q[rvalid].max() == 2 ** 30 and rkey[rvalid].max() < 2 ** 30
    assert pts.tobytes() == S.cluster_points(cS, cn.astype(np.int64), ci.astype(np.int64), lo3, cell).tobytes()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    import __graft_entry__ as ge
    ge.build()
    from list_amd import hip
    S = _S()
    names, exported = H.declared("list_simplify.h"), H.exported(hip.LIB_PATH)
    assert names == sorted(S.SIMPLIFY_EXPORTS)
    assert {n for n in exported if n.startswith("list_simp_")} == set(names)
    taken = tuple(p for _, _, prefixes in H.SECTIONS.values() if prefixes for p in prefixes)
    assert not any(n.startswith(taken) for n in names)
    assert not set(names) & set(hip.EXPORTS) and not any(n.startswith("list_simp_") for n in hip.EXPORTS)
    raw, lib = ctypes.CDLL(hip.LIB_PATH), S.load()
    for name in names:
        assert hasattr(raw, name) and getattr(lib, name) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9
    text = open(os.path.join(H.ROOT, "include", "list_simplify.h")).read()
    assert f"#define LIST_SIMP_MAX_CELLS {S.MAX_CELLS}" in text and f"#define LIST_SIMP_N_TOTALS {len(S.TOTALS)}" in text


def test_refusals_without_gpu():
    """Argument checks come before any HIP call, each with its text; other sections' error texts stay as they were."""
    from list_amd import hip, mesh
    S = _S()
    lib = S.load()
    assert mesh.load().list_mc_workspace_bytes(1, 1, 1) == 0
    before = lib.list_mesh_last_error()
    cells = (ctypes.c_int32 * 3)(4, 4, 4)
    d3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    one = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    assert lib.list_simp_workspace_bytes(-1, 3, cells) == 0 and b"INT32_MAX" in lib.list_simp_last_error()
    assert lib.list_simp_workspace_bytes(3, 2 ** 31, cells) == 0
    assert lib.list_simp_workspace_bytes(3, 3, None) == 0 and b"NULL" in lib.list_simp_last_error()
    for bad in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert lib.list_simp_workspace_bytes(3, 3, (ctypes.c_int32 * 3)(*bad)) == 0
        assert b"[1, 1024]" in lib.list_simp_last_error()
    need = 1 << 20
    buf = ctypes.create_string_buffer(64)                                       # never dereferenced: every call is refused
    p = ctypes.addressof(buf)
    assert lib.list_simp_count(p, None, 10, 20, cells, d3, one, p, need, p, p, None) == hip.ERR_ARG
    assert b"NULL" in lib.list_simp_last_error()
    assert lib.list_simp_count(p, p, 10, 20, cells, d3, one, None, need, p, p, None) == hip.ERR_ARG
    assert lib.list_simp_count(None, p, 10, 20, cells, d3, one, p, need, p, p, None) == hip.ERR_ARG
    assert lib.list_simp_count(p, p, 10, 20, cells, d3, one, p, need, p, None, None) == hip.ERR_ARG
    assert lib.list_simp_count(p, p, 10, 2 ** 31, cells, d3, one, p, need, p, p, None) == hip.ERR_SHAPE
    assert lib.list_simp_count(p, p, 10, 20, (ctypes.c_int32 * 3)(4, 4, 2000), d3, one, p, need, p, p, None) == hip.ERR_SHAPE
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        inv = (ctypes.c_double * 3)(1.0, bad, 1.0)
        assert lib.list_simp_count(p, p, 10, 20, cells, d3, inv, p, need, p, p, None) == hip.ERR_ARG
        assert b"axis 1" in lib.list_simp_last_error()
        assert lib.list_simp_emit(p, 10, 20, cells, d3, inv, p, p, need, p, 5, p, 5, None) == hip.ERR_ARG
    lo = (ctypes.c_double * 3)(0.0, 0.0, float("nan"))
    assert lib.list_simp_count(p, p, 10, 20, cells, lo, one, p, need, p, p, None) == hip.ERR_ARG
    assert lib.list_simp_emit(p, 10, 20, cells, d3, one, p, p, need, p, 11, p, 5, None) == hip.ERR_ARG
    assert lib.list_simp_emit(p, 10, 20, cells, d3, one, p, p, need, p, 5, p, 21, None) == hip.ERR_ARG
    assert lib.list_simp_emit(p, 10, 20, cells, d3, one, p, p, need, None, 5, p, 5, None) == hip.ERR_ARG
    assert lib.list_simp_emit(p, 10, 20, cells, d3, one, None, p, need, p, 5, p, 5, None) == hip.ERR_ARG
    assert lib.list_mesh_last_error() == before
    # the Python layer: cells, bounds, dtypes and shapes, each with its text
    v, f = HAND["one_face"]["verts"], HAND["one_face"]["faces"]
    for bad in (0, -3, 1025, (4, 4), (4, 0, 4), 2.5, True, "8", (4, 4, 4, 4)):
        with pytest.raises(ValueError, match="cells"):
            S.simplify(v, f, bad)
    for lo, hi in ((0.0, 0.0), (0.5, -0.5), (float("nan"), 1.0), (0.0, float("inf")), ((0, 0, 1), (1, 1, 1)), (-1e308, 1e308)):
        with pytest.raises(ValueError, match="bb_m"):
            S.simplify(v, f, 4, lo, hi)
    with pytest.raises(ValueError, match="verts of shape"):
        S.simplify(v[:, :2], f, 4)
    with pytest.raises(ValueError, match="faces of shape"):
        S.simplify(v, f.reshape(-1), 4)
    with pytest.raises(TypeError, match="integers"):
        S.simplify(v, f.astype(np.float32), 4)


def test_parser_defaults():
    from list_amd import arguments
    assert arguments.default_config().mesh_simplify == 0
    assert arguments.get_args(["--mesh_simplify", "64"]).mesh_simplify == 64


def test_mesh_simplify_round_trips_through_obj(tmp_path, mc_meshes):
    from list_amd import mesh
    S = _S()
    v, f = mc_meshes["sphere32"]
    m = mesh.Mesh(v, f)
    small, info = m.simplify(8, return_info=True)
    rv, rf, rinfo = S.simplify_cpu(v, f, 8)
    assert isinstance(small, mesh.Mesh) and info["clusters"] == rinfo["clusters"]
    assert small.vertices.tobytes() == rv.tobytes() and np.array_equal(small.faces, rf)
    assert len(m.simplify((8, 8, 8), -0.5, 0.5).faces) == len(rf)
    lines = open(small.export(str(tmp_path / "small.obj"))).read().splitlines()
    ov = np.array([[np.float32(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")], dtype=np.float32)
    of = np.array([[int(x) - 1 for x in l.split()[1:]] for l in lines if l.startswith("f ")], dtype=np.int32)
    assert ov.tobytes() == small.vertices.tobytes() and np.array_equal(of, small.faces)
    assert os.path.getsize(tmp_path / "small.obj") < os.path.getsize(m.export(str(tmp_path / "full.obj"))) // 8
    # one vertex per cell already: simplifying again on the same grid changes nothing
    again = mesh.Mesh(ov, of).simplify(8)
    assert again.vertices.tobytes() == ov.tobytes() and np.array_equal(again.faces, of)
