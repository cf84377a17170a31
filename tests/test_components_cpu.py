"""CPU: the numpy restatement of the mesh-component filter (components.label_cpu / keep_components_cpu /
select_components) against scipy's connected components and by hand; the C ABI of include/list_components.h; the
parser's flags; Mesh.keep_components.  Every comparison is of integers or of copied floats: exact equality."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H        # noqa: E402
import _components_cases as CC   # noqa: E402

CASES = CC.label_cases()


def _components():
    from list_amd import components
    return components


def scipy_labels(faces, V):
    """(used bool [V], label int64 [V]: the smallest vertex index of the vertex's component) from scipy."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = faces.astype(np.int64)
    g = f[((f >= 0) & (f < V)).all(axis=1)]
    used = np.zeros(V, dtype=bool)
    used[g.ravel()] = True
    rows, cols = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(rows.size), (rows, cols)), shape=(V, V)), directed=False)
    smallest = np.full(lab.max(initial=-1) + 1, V, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(V))
    return used, smallest[lab] if V else np.zeros(0, dtype=np.int64)


def check_against_scipy(faces, V):
    C = _components()
    lab = C.label_cpu(faces, V)
    used, smallest = scipy_labels(faces, V)
    assert lab.ids.dtype == np.int32 and lab.ids.shape == (V,)
    assert np.array_equal(lab.ids >= 0, used)
    K = len(lab.roots)
    assert np.array_equal(lab.roots, np.unique(smallest[used]))               # the minima, in increasing order
    assert np.array_equal(lab.roots[lab.ids[used]], smallest[used])           # the same partition, labelled by its minima
    f = faces.astype(np.int64)
    valid = ((f >= 0) & (f < V)).all(axis=1)
    assert lab.invalid_faces == int((~valid).sum())
    assert np.array_equal(lab.n_faces, np.bincount(lab.ids[f[valid, 0]], minlength=K))
    assert np.array_equal(lab.n_verts, np.bincount(lab.ids[used], minlength=K))
    assert lab.n_faces.sum() == valid.sum() and lab.n_verts.sum() == used.sum()
    return lab


@pytest.mark.parametrize("name", list(CASES))
def test_label_cpu_matches_scipy(name):
    faces, V = CASES[name]
    lab = check_against_scipy(faces, V)
    if name.startswith("strip"):
        assert len(lab.roots) == 1 and lab.roots[0] == 0 and lab.n_faces[0] == len(faces) and lab.n_verts[0] == V
    if name == "many_small":
        assert len(lab.roots) == 700 and lab.n_faces.min() >= 1 and lab.n_faces.max() <= 7


def test_label_cpu_matches_scipy_on_a_marching_cubes_sphere():
    from list_amd import mesh
    v, f = mesh.marching_cubes_cpu(CC.sphere_field(64, 0.3, (0, 0, 0)))
    lab = check_against_scipy(f, len(v))
    assert len(lab.roots) == 1 and lab.n_faces[0] == len(f) and lab.n_verts[0] == len(v)


def test_label_cpu_small_meshes_by_hand():
    C = _components()
    lab = C.label_cpu(*CC.SMALL["no_faces"])
    assert lab.ids.tolist() == [-1] * 5 and len(lab.roots) == 0 and lab.invalid_faces == 0 and lab.rounds == 0
    lab = C.label_cpu(*CC.SMALL["two_sharing_a_vertex"])
    assert lab.ids.tolist() == [0] * 5 and lab.n_faces.tolist() == [2] and lab.n_verts.tolist() == [5]
    lab = C.label_cpu(*CC.SMALL["two_disjoint"])
    assert lab.ids.tolist() == [0, 0, 0, 1, 1, 1] and lab.roots.tolist() == [0, 3] and lab.n_faces.tolist() == [1, 1]
    lab = C.label_cpu(*CC.irregular())
    assert lab.invalid_faces == 5 and (lab.ids[[10, 11, 12, 13, 14, 30]] == -1).all()
    assert lab.n_verts[lab.ids[7]] == 1 and lab.n_faces[lab.ids[7]] == 1      # (7,7,7): a component of one node
    assert lab.n_faces[lab.ids[0]] == 3                                       # the duplicate counts
    lab = C.label_cpu(np.array([[0, 1, 2]]), 0)                               # no vertex: every face is invalid
    assert len(lab.ids) == 0 and len(lab.roots) == 0 and lab.invalid_faces == 1


def test_select_components():
    sel = _components().select_components
    n = [5, 9, 5, 1, 9, 5]
    assert sel(n, "all").tolist() == [True] * 6
    assert sel(n, "all", 5).tolist() == [True, True, True, False, True, True]
    assert sel(n, 1).tolist() == [False, True, False, False, False, False]          # the tie of 9s: the lower id
    assert sel(n, 3).tolist() == [True, True, False, False, True, False]            # ... and of the 5s
    assert sel(n, 4).tolist() == [True, True, True, False, True, False]
    assert sel(n, 100).tolist() == [True] * 6                                        # k > K
    assert sel(n, 100, 2).tolist() == [True, True, True, False, True, True]
    assert sel(n, 2, 6).tolist() == [False, True, False, False, True, False]         # min_faces first, then the top k
    assert sel(n, 3, 10).tolist() == [False] * 6 and sel(n, "all", 10).tolist() == [False] * 6
    assert sel([], 2).shape == (0,) and sel([], "all").dtype == bool
    for bad in (0, -1, 1.5, "largest", True):
        with pytest.raises(ValueError):
            sel(n, bad)
    for bad in (-1, 0.5):
        with pytest.raises(ValueError):
            sel(n, "all", bad)


def test_compaction_order_and_remapping_by_hand():
    """Six triangles: component A = {9, 1, 5, 7} (2 faces), B = {0, 3, 8} (1 face), C = {2, 4, 6, 10, 11} (3 faces);
    the faces interleaved."""
    C = _components()
    verts = (np.arange(36, dtype=np.float32).reshape(12, 3) + np.float32(0.1)) * np.float32(1.7)
    verts[5, 1] = np.float32("nan")
    verts[7, 0] = -0.0
    faces = np.array([[9, 1, 5], [2, 4, 6], [0, 3, 8], [6, 10, 11], [5, 7, 9], [11, 2, 4]], dtype=np.int32)
    lab = C.label_cpu(faces, 12)
    assert lab.roots.tolist() == [0, 1, 2] and lab.n_faces.tolist() == [1, 2, 3] and lab.n_verts.tolist() == [3, 4, 5]
    assert lab.ids.tolist() == [0, 1, 2, 0, 2, 1, 2, 1, 0, 1, 2, 2]
    v, f, info = C.keep_components_cpu(verts, faces, keep=2)                  # C and A stay
    kept = [1, 2, 4, 5, 6, 7, 9, 10, 11]
    assert v.tobytes() == verts[kept].tobytes()
    assert f.dtype == np.int32 and f.tolist() == [[6, 0, 3], [1, 2, 4], [4, 7, 8], [3, 5, 6], [8, 1, 2]]
    assert info["K"] == 3 and info["kept"].tolist() == [1, 2] and info["dropped_faces"] == 1
    assert info["dropped_verts"] == 3 and info["invalid_faces"] == 0 and info["unused_verts"] == 0
    v, f, info = C.keep_components_cpu(verts, faces, keep=1)
    assert v.tobytes() == verts[[2, 4, 6, 10, 11]].tobytes() and f.tolist() == [[0, 1, 2], [2, 3, 4], [4, 0, 1]]
    v, f, info = C.keep_components_cpu(verts, faces, keep="all", min_faces=2)
    assert info["kept"].tolist() == [1, 2] and len(v) == 9 and len(f) == 5
    v, f, info = C.keep_components_cpu(verts, faces)                           # everything stays as it is
    assert v.tobytes() == verts.tobytes() and np.array_equal(f, faces)
    v, f, info = C.keep_components_cpu(verts, faces, keep=1, min_faces=4)
    assert v.shape == (0, 3) and f.shape == (0, 3) and info["dropped_faces"] == 6
    # invalid faces and unused vertices go, whatever is kept
    v, f, info = C.keep_components_cpu(verts, np.concatenate([faces[:1], [[0, 12, 1]], faces[4:5]]).astype(np.int32))
    assert info["invalid_faces"] == 1 and info["unused_verts"] == 8 and f.tolist() == [[3, 0, 1], [1, 2, 3]]
    assert v.tobytes() == verts[[1, 5, 7, 9]].tobytes()
    # keep_components sends host inputs to the same code
    v2, f2, _ = C.keep_components(verts, faces.astype(np.int64), keep=2)
    v1, f1, _ = C.keep_components_cpu(verts, faces, keep=2)
    assert v2.tobytes() == v1.tobytes() and np.array_equal(f1, f2)


def test_three_spheres_keep_one_is_the_big_sphere_alone():
    from list_amd import mesh
    C = _components()
    big, small, blob = CC.three_spheres(40)
    field = np.maximum(np.maximum(big, small), blob)
    # first: the three surfaces share no cell, and on every corner of a cell the big surface cuts the field IS s_big --
    # otherwise the equality below would not hold for marching_cubes_cpu itself
    cuts = [CC.cut_cells(s) for s in (big, small, blob)]
    assert all(c.any() for c in cuts)
    assert not (cuts[0] & cuts[1]).any() and not (cuts[0] & cuts[2]).any() and not (cuts[1] & cuts[2]).any()
    corner = np.zeros(big.shape, dtype=bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        corner[dx:39 + dx, dy:39 + dy, dz:39 + dz] |= cuts[0]
    assert np.array_equal(field[corner], big[corner])
    assert np.array_equal(CC.cut_cells(field), cuts[0] | cuts[1] | cuts[2])
    v, f = mesh.marching_cubes_cpu(field)
    lab = C.label_cpu(f, len(v))
    assert len(lab.roots) == 3 and lab.invalid_faces == 0 and (lab.ids >= 0).all()
    v1, f1, info = C.keep_components_cpu(v, f, keep=1)
    bv, bf = mesh.marching_cubes_cpu(big)
    assert v1.tobytes() == bv.tobytes() and np.array_equal(f1, bf)
    assert info["K"] == 3 and len(info["kept"]) == 1
    # min_faces between the blob's count and the small sphere's drops the blob only
    n_blob, n_small = len(mesh.marching_cubes_cpu(blob)[1]), len(mesh.marching_cubes_cpu(small)[1])
    assert sorted(lab.n_faces.tolist()) == sorted([n_blob, n_small, len(bf)]) and n_blob < n_small < len(bf)
    v2, f2, info = C.keep_components_cpu(v, f, min_faces=(n_blob + n_small) // 2)
    sv, sf = mesh.marching_cubes_cpu(np.maximum(big, small))
    assert v2.tobytes() == sv.tobytes() and np.array_equal(f2, sf) and info["dropped_faces"] == n_blob


def test_header_table_and_library_agree():
    import __graft_entry__ as ge
    ge.build()
    from list_amd import hip
    C = _components()
    names, exported = H.declared("list_components.h"), H.exported(hip.LIB_PATH)
    assert names == sorted(C.COMPONENTS_EXPORTS)
    assert {n for n in exported if n.startswith("list_cc_")} == set(names)
    taken = tuple(p for _, _, prefixes in H.SECTIONS.values() if prefixes for p in prefixes)
    assert not any(n.startswith(taken) for n in names)
    assert not set(names) & set(hip.EXPORTS) and not any(n.startswith("list_cc_") for n in hip.EXPORTS)
    raw, lib = ctypes.CDLL(hip.LIB_PATH), C.load()
    for name in names:
        assert hasattr(raw, name) and getattr(lib, name) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9
    text = open(os.path.join(H.ROOT, "include", "list_components.h")).read()
    assert f"#define LIST_CC_MAX_ROUNDS {C.MAX_ROUNDS}" in text and C.MAX_ROUNDS % C.ROUNDS_PER_READBACK == 0


def test_refusals_without_gpu():
    """Argument checks come before any HIP call: sizes, NULL pointers and the round cap, each with its text; other
    sections' error texts stay as they were.  (The workspace's size comes from hipCUB, which asks the device: the GPU
    tests check it.)"""
    from list_amd import hip, mesh
    C = _components()
    lib = C.load()
    assert mesh.load().list_mc_workspace_bytes(1, 1, 1) == 0
    before = lib.list_mesh_last_error()
    assert lib.list_cc_workspace_bytes(-1, 3) == 0 and b"INT32_MAX" in lib.list_cc_last_error()
    assert lib.list_cc_workspace_bytes(2 ** 31, 3) == 0
    need = 1 << 20
    buf = ctypes.create_string_buffer(64)                                       # never dereferenced: every call is refused
    p = ctypes.addressof(buf)
    assert lib.list_cc_begin(None, 1000, 2000, p, need, None) == hip.ERR_ARG and b"NULL" in lib.list_cc_last_error()
    assert lib.list_cc_begin(p, 1000, 2 ** 31, p, need, None) == hip.ERR_SHAPE
    assert lib.list_cc_rounds(p, 1000, 2000, p, need, C.MAX_ROUNDS - 7, 8, p, None) == hip.ERR_UNSUPPORTED
    assert b"cap of 64 rounds" in lib.list_cc_last_error()
    assert lib.list_cc_rounds(p, 1000, 2000, p, need, 0, 0, p, None) == hip.ERR_ARG
    assert lib.list_cc_rounds(p, 1000, 2000, p, need, 0, 8, None, None) == hip.ERR_ARG
    assert lib.list_cc_finish(p, 1000, 2000, p, need, p, p, p, p, None, None) == hip.ERR_ARG
    assert lib.list_cc_compact(p, p, 1000, 2000, p, p, 1001, p, need, p, 10, p, 10, None) == hip.ERR_ARG
    assert lib.list_cc_compact(p, p, 1000, 2000, p, p, 5, p, need, p, 1001, p, 10, None) == hip.ERR_ARG
    assert lib.list_cc_compact(p, p, 1000, 2000, p, p, 5, p, need, None, 10, p, 10, None) == hip.ERR_ARG
    assert lib.list_mesh_last_error() == before


def test_parser_defaults():
    from list_amd import arguments
    cfg = arguments.default_config()
    assert cfg.mesh_components == 0 and cfg.mesh_min_faces == 0
    cfg = arguments.get_args(["--mesh_components", "2", "--mesh_min_faces", "30"])
    assert cfg.mesh_components == 2 and cfg.mesh_min_faces == 30


def test_mesh_keep_components_round_trips_through_obj(tmp_path):
    from list_amd import mesh
    big, small, blob = CC.three_spheres(40)
    m = mesh.Mesh(*mesh.marching_cubes_cpu(np.maximum(np.maximum(big, small), blob)))
    kept, info = m.keep_components(keep=1, return_info=True)
    assert isinstance(kept, mesh.Mesh) and info["K"] == 3
    bv, bf = mesh.marching_cubes_cpu(big)
    assert kept.vertices.tobytes() == bv.tobytes() and np.array_equal(kept.faces, bf)
    assert len(m.keep_components().faces) == len(m.faces)                     # the default keeps everything
    lines = open(kept.export(str(tmp_path / "kept.obj"))).read().splitlines()
    v = np.array([[np.float32(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")], dtype=np.float32)
    f = np.array([[int(x) - 1 for x in l.split()[1:]] for l in lines if l.startswith("f ")], dtype=np.int32)
    assert v.tobytes() == kept.vertices.tobytes() and np.array_equal(f, kept.faces)
    again = mesh.Mesh(v, f).keep_components(keep=1)                           # one component already: a fixed point
    assert again.vertices.tobytes() == v.tobytes() and np.array_equal(again.faces, f)
