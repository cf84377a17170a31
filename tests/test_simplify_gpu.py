"""GPU: the vertex-clustering simplifier in HIP (include/list_simplify.h, simplify.simplify) against its numpy
restatement (simplify.simplify_cpu, itself held to hand-worked cases and a Fraction loop in test_simplify_cpu.py).
Everything compared is an integer or a float as its bytes: exact equality, no tolerance."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _simplify_cases as SC     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HAND = SC.hand_cases()
TOTALS = ("n_verts", "n_faces", "clusters", "invalid_verts", "invalid_faces", "degenerate_faces")


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def _S():
    from list_amd import simplify
    return simplify


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(result):
    v, f, info = result
    info = dict(info)
    info["vertex_map"] = info["vertex_map"].cpu().numpy()
    return v.cpu().numpy(), f.cpu().numpy(), info


def check(verts, faces, cells, lo=-0.5, hi=0.5):
    """Device simplify == the numpy restatement: output vertices as bytes, faces, vertex_map and all six totals.
    Returns the device result on the host."""
    S = _S()
    got = S.simplify(dev(verts), dev(faces), cells, lo, hi)
    assert got[0].is_cuda and got[1].is_cuda and got[2]["vertex_map"].is_cuda
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2]["vertex_map"].dtype == torch.int32
    v, f, info = host(got)
    rv, rf, rinfo = S.simplify_cpu(verts, faces, cells, lo, hi)
    for k in TOTALS:
        assert info[k] == rinfo[k], (k, info[k], rinfo[k])
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(info["vertex_map"], rinfo["vertex_map"]), "vertex_map"
    assert np.array_equal(f, rf), "output faces"
    assert v.tobytes() == rv.tobytes(), "output vertices"
    return v, f, info


@pytest.mark.parametrize("name", list(HAND))
def test_hand_worked_cases(name):
    """... which include V = 0, F = 0 and one face."""
    c = HAND[name]
    SC.check_case(c, check(c["verts"], c["faces"], c["cells"], c["bb_min"], c["bb_max"]))


def test_pile_up_in_one_cell():
    """100 000 vertices in one cell: one accumulator takes every add, and its run crosses many waves and workgroups."""
    v, f, cells, lo, hi = SC.pile_up()
    ov, of, info = check(v, f, cells, lo, hi)
    assert info["clusters"] == 4 and info["n_verts"] == 4 and info["n_faces"] == 2 and info["degenerate_faces"] == 50
    assert np.bincount(info["vertex_map"] + 1).max() == 100000


def test_many_clusters_of_one_vertex():
    """150 000 lattice vertices, one per cell of a 1024^3 grid: every run has length 1."""
    v, f, cells, lo, hi = SC.lattice()
    ov, of, info = check(v, f, cells, lo, hi)
    assert info["clusters"] == len(v) == 150000 and info["n_verts"] == len(v) and info["n_faces"] == len(f)


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
@pytest.mark.parametrize("before", [63, 64, 511, 512])
@pytest.mark.parametrize("length", [63, 64, 65, 257])
def test_run_lengths_at_wave_boundaries(length, before, order):
    """A run of `length` vertices that starts at sorted position `before`: at a wave's first lane (64), one before it
    (63), and the same at the edge of a wave's range of 512 positions (512, 511)."""
    v, f, cells, lo, hi = SC.runs(length, before, order)
    ov, of, info = check(v, f, cells, lo, hi)
    assert info["clusters"] == before + 71 and np.bincount(info["vertex_map"] + 1).max() == length


def test_anisotropic_cells():
    v, f = SC.random_mesh(20000, 60000, seed=8)
    ov, of, info = check(v, f, (3, 1024, 7))
    assert info["n_faces"] > 0 and info["invalid_verts"] >= 1 and info["invalid_faces"] >= 1
    check(v, f, (1024, 1, 2), (-0.5, -0.6, -0.7), (0.5, 0.7, 0.9))


@pytest.fixture(scope="module")
def mc_meshes():
    """name -> (verts, faces) of mesh.marching_cubes of SC.FIELDS on the device."""
    from list_amd import mesh
    return {name: mesh.marching_cubes(dev(field())) for name, field in SC.FIELDS.items()}


@pytest.mark.parametrize("cells", [8, 16])
@pytest.mark.parametrize("name", list(SC.FIELDS))
def test_marching_cubes_meshes_on_the_device(mc_meshes, name, cells):
    S = _S()
    v, f = mc_meshes[name]
    got = host(S.simplify(v, f, cells))
    ref = S.simplify_cpu(v.cpu().numpy(), f.cpu().numpy(), cells)
    assert got[0].tobytes() == ref[0].tobytes() and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2]["vertex_map"], ref[2]["vertex_map"])
    for k in TOTALS:
        assert got[2][k] == ref[2][k], k
    assert got[2]["n_faces"] > 0 and (SC.edge_uses(got[1]) % 2 == 0).all()


def test_chain_components_simplify_rasterize():
    """Three spheres through marching cubes, keep_components(keep=1), simplify and rasterize on the device == the same
    chain of restatements from the marching-cubes mesh on."""
    from list_amd import components, mesh, render
    S = _S()
    v, f = mesh.marching_cubes(dev(SC.three_spheres(40)))
    kv, kf, cinfo = components.keep_components(v, f, keep=1)
    sv, sf, sinfo = S.simplify(kv, kf, 12)
    cam = render.Camera.orthographic(0, 64, 64)
    face_id, depth, stats = render.rasterize(sv, sf, cam, 64, 64)
    hv, hf, hcinfo = components.keep_components_cpu(v.cpu().numpy(), f.cpu().numpy(), keep=1)
    rv, rf, rinfo = S.simplify_cpu(hv, hf, 12)
    rid, rdepth, rstats = render.rasterize_cpu(rv, rf, cam, 64, 64)
    assert cinfo["K"] == hcinfo["K"] == 3 and 0 < sinfo["n_faces"] < len(kf)
    assert sv.cpu().numpy().tobytes() == rv.tobytes() and np.array_equal(sf.cpu().numpy(), rf)
    assert np.array_equal(face_id.cpu().numpy(), rid) and depth.cpu().numpy().tobytes() == rdepth.tobytes()
    assert stats == rstats and (rid >= 0).any()


@pytest.fixture(scope="module")
def list_run():
    """A LIST model with seeded weights and its predicted 40^3 volume, moved to its median so that a surface crosses
    the grid whatever the weights (as test_components_gpu.py does)."""
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


def test_executor_simplifies_the_mesh_before_it_leaves_the_device(list_run):
    from list_amd import arguments, components, mesh, utils
    S = _S()
    executor, img, grid = list_run
    ex0, cfg0 = executor([])
    assert cfg0.mesh_simplify == 0 and ex0.mesh_simplify == 0
    mv, mf = mesh.marching_cubes(grid[0], 0.0, -0.5, 0.5)
    fv, ff = ex0.filter_mesh(mv, mf)
    assert fv is mv and ff is mf and ex0.last_simplify is None                 # 0 runs no new code: the same objects
    ex0.predict_grid = lambda *a, **k: grid
    base = ex0.test({"rgb_image": img})[0][0]
    assert base.vertices.tobytes() == mv.cpu().numpy().tobytes() and np.array_equal(base.faces, mf.cpu().numpy())
    ex, cfg = executor(["--mesh_simplify", "16"])
    ex.predict_grid = lambda *a, **k: grid
    got = ex.test({"rgb_image": img})[0][0]
    rv, rf, rinfo = S.simplify_cpu(base.vertices, base.faces, 16, cfg.bb_min, cfg.bb_max)
    assert isinstance(got, mesh.Mesh) and 0 < len(rf) < len(base.faces)
    assert got.vertices.tobytes() == rv.tobytes() and np.array_equal(got.faces, rf)
    for k in TOTALS:
        assert ex.last_simplify[k] == rinfo[k], k
    assert np.array_equal(ex.last_simplify["vertex_map"].cpu().numpy(), rinfo["vertex_map"])
    # the component filter comes first, on the full-resolution mesh
    ex, cfg = executor(["--mesh_simplify", "16", "--mesh_components", "1"])
    ex.predict_grid = lambda *a, **k: grid
    got = ex.test({"rgb_image": img})[0][0]
    kv, kf, _ = components.keep_components_cpu(base.vertices, base.faces, keep=1)
    rv, rf, _ = S.simplify_cpu(kv, kf, 16)
    assert got.vertices.tobytes() == rv.tobytes() and np.array_equal(got.faces, rf)
    assert ex.last_components["K"] >= 1 and ex.last_simplify["n_faces"] == len(rf)
    with pytest.raises(ValueError):
        utils.get_class("network.executors.LIST")(arguments.default_config(mesh_simplify=2000), ex0.model)


def test_undersized_outputs_are_skipped_not_written():
    """n_out_verts and n_out_faces one short, inside guard-banded buffers: nothing at or past the stated size is
    written, everything before it is."""
    from list_amd import hip
    S = _S()
    lib = S.load()
    v, f = SC.random_mesh(3000, 9000, seed=12)
    rv, rf, rinfo = S.simplify_cpu(v, f, 6)
    Vo, Fo = len(rv), len(rf)
    assert Vo > 2 and Fo > 2
    dv, df = dev(v), dev(f)
    V, F = len(v), len(f)
    R, lo, inv, cell = S.grid(6)
    cR, clo = (ctypes.c_int32 * 3)(*R.tolist()), (ctypes.c_double * 3)(*lo.tolist())
    cinv, ccell = (ctypes.c_double * 3)(*inv.tolist()), (ctypes.c_double * 3)(*cell.tolist())
    need = lib.list_simp_workspace_bytes(V, F, cR)
    assert need > 0 and lib.list_simp_workspace_bytes(V, F, cR) == need and lib.list_simp_workspace_bytes(0, 0, cR) > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    vmap = torch.empty((V,), dtype=torch.int32, device=DEV)
    totals = torch.empty((6,), dtype=torch.int64, device=DEV)
    st = hip._stream()
    assert lib.list_simp_count(dv.data_ptr(), df.data_ptr(), V, F, cR, clo, cinv, ws.data_ptr(), need - 1, vmap.data_ptr(),
                               totals.data_ptr(), st) == hip.ERR_WORKSPACE
    assert b"list_simp_workspace_bytes" in lib.list_simp_last_error()
    S._check(lib.list_simp_count(dv.data_ptr(), df.data_ptr(), V, F, cR, clo, cinv, ws.data_ptr(), need, vmap.data_ptr(),
                                 totals.data_ptr(), st), "list_simp_count")
    assert totals.tolist()[:2] == [Vo, Fo]
    G = 64                                                                     # guard rows on both sides
    ov = torch.full((Vo + 2 * G, 3), -7.0, dtype=torch.float32, device=DEV)
    of = torch.full((Fo + 2 * G, 3), -7, dtype=torch.int32, device=DEV)
    S._check(lib.list_simp_emit(df.data_ptr(), V, F, cR, clo, ccell, vmap.data_ptr(), ws.data_ptr(), need,
                                ov[G:].data_ptr(), Vo - 1, of[G:].data_ptr(), Fo - 1, st), "list_simp_emit")
    torch.cuda.synchronize()
    ov, of = ov.cpu().numpy(), of.cpu().numpy()
    assert ov[G:G + Vo - 1].tobytes() == rv[:Vo - 1].tobytes() and np.array_equal(of[G:G + Fo - 1], rf[:Fo - 1])
    assert (ov[:G] == -7).all() and (ov[G + Vo - 1:] == -7).all()
    assert (of[:G] == -7).all() and (of[G + Fo - 1:] == -7).all()


def test_inputs_streams_and_determinism():
    """Non-contiguous tensors are copied, other dtypes, shapes and devices refused; a side stream; two runs agree."""
    from list_amd import hip
    S = _S()
    v, f = SC.random_mesh(5000, 15000, seed=13)
    ref = S.simplify_cpu(v, f, 9)
    ft = dev(np.ascontiguousarray(f.T)).t()
    vt = dev(np.concatenate([v, v], axis=1))[:, :3]
    assert not ft.is_contiguous() and not vt.is_contiguous()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = S.simplify(vt, ft, 9)
        b = S.simplify(vt, ft, 9)
    s.synchronize()
    for got in (a, b):
        assert got[0].cpu().numpy().tobytes() == ref[0].tobytes() and np.array_equal(got[1].cpu().numpy(), ref[1])
    with pytest.raises(RuntimeError):
        S.simplify(dev(v).double(), dev(f), 9)
    with pytest.raises(RuntimeError):
        S.simplify(dev(v), dev(f).long(), 9)
    with pytest.raises(RuntimeError):
        S.simplify(dev(v), torch.from_numpy(f), 9)
    with pytest.raises(hip.ListError) as e:
        S.simplify(dev(v)[:, :2], dev(f), 9)
    assert e.value.code == hip.ERR_SHAPE
    with pytest.raises(hip.ListError) as e:
        S.simplify(dev(v), dev(f).reshape(-1), 9)
    assert e.value.code == hip.ERR_SHAPE
    with pytest.raises(ValueError):
        S.simplify(dev(v), dev(f), 0)
    with pytest.raises(ValueError):
        S.simplify(dev(v), dev(f), 9, 0.5, -0.5)
