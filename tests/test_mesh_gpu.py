"""GPU: marching cubes in HIP (include/list_mesh.h, mesh.marching_cubes) against its numpy restatement
(mesh.marching_cubes_cpu) and against the analytic surfaces of closed fields; LIST.test() meshing on the device."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def _mesh():
    from list_amd import mesh
    return mesh


def _grid(shape, lo=-0.5, hi=0.5):
    axes = [np.linspace(lo, hi, n, dtype=np.float64) for n in shape]
    return np.meshgrid(*axes, indexing="ij")


def sphere(shape, r=0.3, c=(0.0, 0.0, 0.0)):
    x, y, z = _grid(shape)
    return r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)


def torus(n, R=0.25, r=0.1):
    x, y, z = _grid((n, n, n))
    return (r - np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z)).astype(np.float32)


def two_spheres(n):
    return np.maximum(sphere((n,) * 3, 0.15, (-0.22, 0, 0)), sphere((n,) * 3, 0.15, (0.22, 0.05, 0)))


def nonfinite(n):
    v = sphere((n,) * 3).astype(np.float32)
    rng = np.random.default_rng(7)
    flat = v.reshape(-1)
    near = np.flatnonzero(np.abs(flat) < 2.0 / n)             # on the surface, where the values matter
    for val in (np.nan, np.inf, -np.inf):
        flat[rng.choice(near, 40, replace=False)] = val
    flat[rng.choice(flat.size, 40, replace=False)] = np.nan
    return v


FIELDS = {
    "sphere32": lambda: sphere((32,) * 3),
    "sphere64": lambda: sphere((64,) * 3),
    "sphere128": lambda: sphere((128,) * 3),
    "sphere256": lambda: sphere((256,) * 3),
    "torus": lambda: torus(96),
    "two_spheres": lambda: two_spheres(80),
    "noncubic": lambda: sphere((40, 57, 70), 0.3, (0.03, -0.02, 0.01)),
    "all_positive": lambda: np.full((33, 20, 17), 1.0),
    "all_negative": lambda: np.full((16, 31, 9), -1.0),
    "nonfinite": lambda: nonfinite(48),
}
EULER = {"sphere32": 2, "sphere64": 2, "sphere128": 2, "sphere256": 2, "torus": 0, "two_spheres": 4, "noncubic": 2}


def canonical(v, f):
    """Vertices sorted lexicographically, faces renumbered, rotated to start at their smallest index, then sorted."""
    order = np.lexsort(v.T[::-1])
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    g = inv[f.astype(np.int64)]
    k = np.argmin(g, axis=1)
    g = np.stack([g[np.arange(len(g)), (k + s) % 3] for s in range(3)], axis=1)
    return v[order], g[np.lexsort(g.T[::-1])]


def topology(v, f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    _, ucnt = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    vol = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)
    return len(v) - len(ucnt) + len(f), ucnt, dcnt, vol


@pytest.mark.parametrize("name", list(FIELDS))
def test_marching_cubes_matches_cpu_and_is_deterministic(name):
    mesh = _mesh()
    vol = np.ascontiguousarray(FIELDS[name](), dtype=np.float32)
    t = torch.from_numpy(vol).to(DEV)
    v, f = mesh.marching_cubes(t)
    v2, f2 = mesh.marching_cubes(t)
    torch.cuda.synchronize()
    assert v.device == t.device and v.dtype == torch.float32 and f.dtype == torch.int32
    assert torch.equal(v, v2) and torch.equal(f, f2), "two runs differ"
    v, f = v.cpu().numpy(), f.cpu().numpy()
    cv, cf = mesh.marching_cubes_cpu(vol)
    assert v.shape == cv.shape and f.shape == cf.shape, (v.shape, cv.shape, f.shape, cf.shape)
    assert np.isfinite(v).all()
    if name.startswith("all_"):
        assert v.shape == (0, 3) and f.shape == (0, 3)
        return
    a, af = canonical(v, f)
    b, bf = canonical(cv, cf)
    assert np.abs(a - b).max() <= 1e-6 and np.array_equal(af, bf)
    assert np.abs(v - cv).max() <= 1e-6 and np.array_equal(f, cf)      # and in the documented (raster) order
    assert f.min() >= 0 and f.max() < len(v)
    if name in EULER:
        chi, ucnt, dcnt, enclosed = topology(v, f)
        assert ucnt.min() == 2 and ucnt.max() == 2, "an edge not shared by exactly two triangles"
        assert dcnt.max() == 1, "inconsistent winding"
        assert chi == EULER[name]
        assert enclosed > 0


def test_sphere_geometry_at_128():
    mesh = _mesh()
    r = 0.3
    v, f = mesh.marching_cubes(torch.from_numpy(sphere((128,) * 3, r).astype(np.float32)).to(DEV))
    v, f = v.cpu().numpy(), f.cpu().numpy()
    _, _, _, enclosed = topology(v, f)
    assert abs(enclosed / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - r).max() < 1e-3


def test_level_bounds_and_layout():
    """A non-zero level, per-axis bounds, a non-contiguous input and a side stream give the oracle's mesh."""
    mesh = _mesh()
    vol = sphere((30, 44, 36)).astype(np.float32)
    base = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 0, 1))).to(DEV)
    t = base.permute(1, 2, 0)                                   # non-contiguous view of vol
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        v, f = mesh.marching_cubes(t, level=0.05, bb_min=(-1.0, 0.0, 2.0), bb_max=(1.0, 3.0, 2.5))
    s.synchronize()
    cv, cf = mesh.marching_cubes_cpu(vol, 0.05, (-1.0, 0.0, 2.0), (1.0, 3.0, 2.5))
    assert np.abs(v.cpu().numpy() - cv).max() <= 1e-6 and np.array_equal(f.cpu().numpy(), cf)
    assert cv[:, 0].min() >= -1.0 and cv[:, 1].min() >= 0.0 and cv[:, 2].min() >= 2.0


def test_shape_errors():
    from list_amd import hip
    mesh = _mesh()
    with pytest.raises(hip.ListError) as e:
        mesh.marching_cubes(torch.zeros((1, 8, 8), device=DEV))
    assert e.value.code == hip.ERR_SHAPE
    with pytest.raises(RuntimeError):
        mesh.marching_cubes(torch.zeros((8, 8, 8), dtype=torch.float64, device=DEV))


def test_list_test_meshes_on_device_without_mcubes(monkeypatch, tmp_path):
    """executors.LIST.test -> Mesh from the device, with PyMCubes and trimesh hidden; save() writes an OBJ with the
    same vertex / face counts."""
    from oracle import fill, synth
    from list_amd import arguments, mesh, utils
    from list_amd.train import _Module
    monkeypatch.setitem(sys.modules, "mcubes", None)
    monkeypatch.setitem(sys.modules, "trimesh", None)
    cfg = arguments.default_config(vox_res=32, train_batch_size=1, mcube_znum=40, test_pointnum=5000)
    cfg.device = torch.device(DEV)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(DEV)
    ex = utils.get_class("network.executors.LIST")(cfg, _Module(net))
    img = torch.from_numpy(synth.uniform(78, (1, 3, 64, 64))).to(DEV)
    vol, occ, vox_feat = ex.predict_grid(img)
    # the predicted field moved to its median, so that a surface crosses the grid whatever the weights; test() meshes
    # exactly this volume
    vol = vol - float(vol.median())
    ex.predict_grid = lambda *a, **k: (vol, occ, vox_feat)
    pred, score = ex.test({"rgb_image": img})
    m = pred[0]
    assert isinstance(m, mesh.Mesh) and score == {}
    assert len(m.faces) > 0
    cv, cf = mesh.marching_cubes_cpu(vol.cpu().numpy(), 0.0, -0.5, 0.5)
    assert np.abs(m.vertices - cv).max() <= 1e-6 and np.array_equal(m.faces, cf)
    ex.save({"rgb_image": img}, pred, str(tmp_path / "item"))
    lines = open(tmp_path / "item_pred.obj").read().splitlines()
    nv = sum(l.startswith("v ") for l in lines)
    nf = sum(l.startswith("f ") for l in lines)
    assert (nv, nf) == (len(m.vertices), len(m.faces))
    assert max(int(x) for l in lines if l.startswith("f ") for x in l.split()[1:]) <= nv
