"""GPU: the mesh-component filter in HIP (include/list_components.h, components.label / keep_components) against its
numpy restatement (label_cpu / keep_components_cpu, themselves held to scipy in test_components_cpu.py).  Everything
compared is an integer or a copied float: exact equality, no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _components_cases as CC   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = CC.label_cases()


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def _components():
    from list_amd import components
    return components


def some_verts(V, seed=3):
    """float32 [V,3] with a NaN, an infinity and a negative zero among them: compaction copies bits."""
    v = np.random.default_rng(seed).standard_normal((V, 3)).astype(np.float32)
    if V >= 3:
        v[0, 0], v[V // 2, 1], v[V - 1, 2] = np.float32("nan"), -0.0, np.float32("-inf")
    return v


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_label(faces, V):
    """Device labels of (faces, V) == the numpy restatement's, field by field; returns the device Labels."""
    C = _components()
    got, ref = C.label(dev(faces), V), C.label_cpu(faces, V)
    assert got.ids.dtype == torch.int32 and got.ids.is_cuda and got.ids.shape == (V,)
    assert np.array_equal(got.ids.cpu().numpy(), ref.ids), "per-vertex ids"
    assert np.array_equal(got.roots.cpu().numpy(), ref.roots), "roots"
    assert np.array_equal(got.n_faces.cpu().numpy(), ref.n_faces), "face counts"
    assert np.array_equal(got.n_verts.cpu().numpy(), ref.n_verts), "vertex counts"
    assert got.invalid_faces == ref.invalid_faces
    assert 0 <= got.rounds <= C.MAX_ROUNDS
    return got


def check_keep(verts, faces, keep="all", min_faces=0):
    """Device keep_components == the numpy restatement's: vertices as bytes, faces, and the info."""
    C = _components()
    v, f, info = C.keep_components(dev(verts), dev(faces), keep=keep, min_faces=min_faces)
    rv, rf, rinfo = C.keep_components_cpu(verts, faces, keep=keep, min_faces=min_faces)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert v.cpu().numpy().tobytes() == rv.tobytes(), "output vertices"
    assert np.array_equal(f.cpu().numpy(), rf), "output faces"
    for k in ("K", "kept_faces", "kept_verts", "dropped_faces", "dropped_verts", "unused_verts", "invalid_faces"):
        assert info[k] == rinfo[k], k
    assert np.array_equal(info["kept"], rinfo["kept"])
    return v, f, info


@pytest.mark.parametrize("name", list(CC.SMALL))
def test_small_meshes(name):
    faces, V = CC.SMALL[name]
    lab = check_label(faces, V)
    verts = some_verts(V)
    check_keep(verts, faces)
    check_keep(verts, faces, keep=1)
    if name == "no_faces":
        assert lab.rounds == 0 and lab.ids.tolist() == [-1] * 5
        v, f, info = check_keep(verts[:0], faces)                             # and no vertices either
        assert v.shape == (0, 3) and f.shape == (0, 3) and info["K"] == 0
    if name == "two_disjoint":
        v, f, info = check_keep(verts, faces, keep=1)                         # a tie: the lower id, vertices 0 1 2
        assert f.tolist() == [[0, 1, 2]] and v.cpu().numpy().tobytes() == verts[:3].tobytes()


@pytest.mark.parametrize("order", CC.STRIP_ORDERS)
@pytest.mark.parametrize("F", CC.STRIP_LENGTHS)
def test_strip_label_travels_its_whole_length(F, order):
    C = _components()
    faces, V = CASES[f"strip_{F}_{order}"]
    lab = check_label(faces, V)
    print(f"strip F={F} {order}: {lab.rounds} rounds (cap {C.MAX_ROUNDS})")
    assert lab.rounds <= C.MAX_ROUNDS                   # inside the cap (past it the library refuses and label raises)
    assert lab.roots.tolist() == [0] and lab.n_faces.tolist() == [F] and lab.n_verts.tolist() == [V]
    check_keep(some_verts(V), faces, keep=1)


def test_many_small_components():
    faces, V = CASES["many_small"]
    lab = check_label(faces, V)
    assert len(lab.roots) == 700
    verts = some_verts(V)
    counts = lab.n_faces.cpu().numpy()
    assert (np.bincount(counts)[1:8] > 50).all()                              # many equal counts: the ties matter
    for keep, min_faces in ((3, 0), (50, 0), ("all", 4), (50, 4), (1000, 0), (3, 8)):
        v, f, info = check_keep(verts, faces, keep=keep, min_faces=min_faces)
    assert len(f) == 0 and info["dropped_faces"] == len(faces)


def test_many_components_past_the_grid_stride():
    """600 k faces and 900 k vertices: more than the 2048 workgroups x 256 threads the kernels launch, so every
    thread takes several items, in 150 k components."""
    faces, V = CC.many_small(150000, seed=11)
    assert len(faces) > 2048 * 256 and V > 2048 * 256
    lab = check_label(faces, V)
    assert len(lab.roots) == 150000
    check_keep(some_verts(V), faces, keep=1000, min_faces=3)


def test_irregular_faces_and_vertices():
    faces, V = CC.irregular()
    lab = check_label(faces, V)
    assert lab.invalid_faces == 5 and (lab.ids.cpu().numpy()[[10, 11, 12, 13, 14, 30]] == -1).all()
    verts = some_verts(V)
    v, f, info = check_keep(verts, faces)
    assert info["invalid_faces"] == 5 and info["unused_verts"] == 6 and len(v) == V - 6 and len(f) == len(faces) - 5
    check_keep(verts, faces, keep=2)
    check_keep(verts, faces, min_faces=2)
    bad = np.array([[-1, 0, 1], [0, 1, V], [CC.INT32_MAX, 0, 0]], dtype=np.int32)    # nothing but invalid faces
    lab = check_label(bad, V)
    assert lab.invalid_faces == 3 and len(lab.roots) == 0
    v, f, info = check_keep(verts, bad)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_one_component_holding_every_face():
    """marching_cubes of a 64^3 sphere: every face adds to one counter."""
    from list_amd import mesh
    C = _components()
    v, f = mesh.marching_cubes(dev(CC.sphere_field(64, 0.3, (0, 0, 0))))
    lab = C.label(f, len(v))
    assert lab.roots.tolist() == [0] and lab.n_faces.tolist() == [len(f)] and lab.n_verts.tolist() == [len(v)]
    assert lab.invalid_faces == 0 and int(lab.ids.min()) == 0 and int(lab.ids.max()) == 0
    check_label(f.cpu().numpy(), len(v))
    kv, kf, info = C.keep_components(v, f, keep=1)
    assert torch.equal(kv, v) and torch.equal(kf, f) and info["K"] == 1 and info["dropped_faces"] == 0


def test_three_spheres_end_to_end_on_the_device():
    from list_amd import mesh
    C = _components()
    big, small, blob = CC.three_spheres(40)
    field = np.maximum(np.maximum(big, small), blob)
    v, f = mesh.marching_cubes(dev(field))
    kv, kf, info = C.keep_components(v, f, keep=1)
    bv, bf = mesh.marching_cubes(dev(big))
    assert info["K"] == 3 and torch.equal(kf, bf)
    assert kv.cpu().numpy().tobytes() == bv.cpu().numpy().tobytes()
    # min_faces between the blob's face count and the small sphere's drops the blob only
    n_blob, n_small = len(mesh.marching_cubes(dev(blob))[1]), len(mesh.marching_cubes(dev(small))[1])
    assert n_blob < n_small < len(bf)
    kv, kf, info = C.keep_components(v, f, min_faces=(n_blob + n_small) // 2)
    sv, sf = mesh.marching_cubes(dev(np.maximum(big, small)))
    assert torch.equal(kf, sf) and kv.cpu().numpy().tobytes() == sv.cpu().numpy().tobytes()
    assert len(info["kept"]) == 2 and info["dropped_faces"] == n_blob
    check_keep(v.cpu().numpy(), f.cpu().numpy(), keep=2)


def test_determinism_and_face_order():
    C = _components()
    faces, V = CASES["many_small"]
    verts = some_verts(V)
    a, b = C.label(dev(faces), V), C.label(dev(faces), V)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    r1, r2 = (C.keep_components(dev(verts), dev(faces), keep=50) for _ in range(2))
    assert r1[0].cpu().numpy().tobytes() == r2[0].cpu().numpy().tobytes() and torch.equal(r1[1], r2[1])
    for name in ("many_small", "strip_3001_permuted", "irregular"):
        faces, V = CASES[name]
        shuffled = faces[np.random.default_rng(9).permutation(len(faces))]
        a, b = C.label(dev(faces), V), C.label(dev(shuffled), V)
        assert torch.equal(a.ids, b.ids) and torch.equal(a.roots, b.roots) and torch.equal(a.n_faces, b.n_faces)


def test_inputs_streams_and_workspace():
    """Non-contiguous tensors are copied, other dtypes and shapes refused; a side stream; the workspace is a function
    of (V, F) and a smaller one is refused."""
    from list_amd import hip
    C = _components()
    faces, V = CASES["many_small"]
    verts = some_verts(V)
    ref = C.keep_components_cpu(verts, faces, keep=5)
    ft = dev(np.ascontiguousarray(faces.T)).t()                                # non-contiguous [F,3]
    vt = dev(np.concatenate([verts, verts], axis=1))[:, :3]                    # non-contiguous [V,3]
    assert not ft.is_contiguous() and not vt.is_contiguous()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        v, f, _ = C.keep_components(vt, ft, keep=5)
    s.synchronize()
    assert v.cpu().numpy().tobytes() == ref[0].tobytes() and np.array_equal(f.cpu().numpy(), ref[1])
    with pytest.raises(RuntimeError):
        C.label(dev(faces).long(), V)
    with pytest.raises(RuntimeError):
        C.keep_components(dev(verts).double(), dev(faces))
    with pytest.raises(RuntimeError):
        C.keep_components(dev(verts), torch.from_numpy(faces))                # one on the device, one on the host
    with pytest.raises(hip.ListError) as e:
        C.label(dev(faces).reshape(-1), V)
    assert e.value.code == hip.ERR_SHAPE
    with pytest.raises(hip.ListError) as e:
        C.keep_components(dev(verts)[:, :2], dev(faces))
    assert e.value.code == hip.ERR_SHAPE
    with pytest.raises(ValueError):
        C.keep_components(dev(verts), dev(faces), keep=0)
    lib = C.load()
    need = lib.list_cc_workspace_bytes(1000, 2000)
    assert need >= 5 * 4 * 1000 + 2 * 4 * 2000 + 1000 and lib.list_cc_workspace_bytes(1000, 2000) == need
    assert lib.list_cc_workspace_bytes(0, 0) > 0 and lib.list_cc_workspace_bytes(2000, 4000) > need
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    f = dev(np.zeros((2000, 3), dtype=np.int32))
    assert lib.list_cc_begin(f.data_ptr(), 1000, 2000, ws.data_ptr(), need - 1, None) == hip.ERR_WORKSPACE
    assert b"list_cc_workspace_bytes" in lib.list_cc_last_error()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def list_run():
    """A LIST model with seeded weights and its predicted 40^3 volume, moved to its median so that a surface crosses
    the grid whatever the weights (as test_mesh_gpu.py does)."""
    from oracle import fill, synth
    from list_amd import arguments, utils
    from list_amd.train import _Module

    def executor(argv):
        cfg = arguments.get_args(["--vox_res", "32", "--train_batch_size", "1", "--mcube_znum", "40",
                                  "--test_pointnum", "5000"] + argv)
        cfg.device = torch.device(DEV)
        return utils.get_class("network.executors.LIST")(cfg, _Module(net)), cfg

    cfg = arguments.default_config(vox_res=32, train_batch_size=1, mcube_znum=40, test_pointnum=5000)
    cfg.device = torch.device(DEV)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(DEV)
    img = torch.from_numpy(synth.uniform(78, (1, 3, 64, 64))).to(DEV)
    ex, _ = executor([])
    vol, occ, vox_feat = ex.predict_grid(img)
    vol = vol - float(vol.median())
    return executor, img, (vol, occ, vox_feat)


def test_executor_filters_the_mesh_before_it_leaves_the_device(list_run):
    from list_amd import mesh
    C = _components()
    executor, img, grid = list_run
    ex0, cfg0 = executor([])
    assert cfg0.mesh_components == 0 and cfg0.mesh_min_faces == 0
    ex0.predict_grid = lambda *a, **k: grid
    base = ex0.test({"rgb_image": img})[0][0]
    cv, cf = mesh.marching_cubes(grid[0], 0.0, -0.5, 0.5)
    assert ex0.last_components is None                                        # the defaults run no new code ...
    assert base.vertices.tobytes() == cv.cpu().numpy().tobytes() and np.array_equal(base.faces, cf.cpu().numpy())
    K = C.label_cpu(base.faces, len(base.vertices))
    assert len(K.roots) >= 1
    for argv, keep, min_faces in ((["--mesh_components", "1"], 1, 0), (["--mesh_min_faces", "20"], "all", 20),
                                  (["--mesh_components", "2", "--mesh_min_faces", "3"], 2, 3)):
        ex, cfg = executor(argv)
        ex.predict_grid = lambda *a, **k: grid
        got = ex.test({"rgb_image": img})[0][0]
        rv, rf, rinfo = C.keep_components_cpu(base.vertices, base.faces, keep=keep, min_faces=min_faces)
        assert isinstance(got, mesh.Mesh)
        assert got.vertices.tobytes() == rv.tobytes() and np.array_equal(got.faces, rf), argv
        assert ex.last_components["K"] == rinfo["K"] == len(K.roots)
        assert ex.last_components["dropped_faces"] == rinfo["dropped_faces"]
    from list_amd import arguments, utils
    with pytest.raises(ValueError):
        bad = arguments.default_config(mesh_components=-1)
        utils.get_class("network.executors.LIST")(bad, ex0.model)
