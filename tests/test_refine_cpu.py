"""CPU: the coarse-to-fine grid's numpy restatement (refine.classify_cpu, refined_points_cpu, fill_cpu) on hand-built
lattices, its meshing guarantee on an analytic sphere, and the C ABI of include/list_refine.h up to the first HIP call."""
import os

import numpy as np
import pytest

from list_amd import mesh, refine as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- geometry -------------------------------------------------------------------------------------------------------
def test_lattice_geometry():
    c = RF.lattice_indices(256, 4)
    assert len(c) == 65 and c[0] == 0 and c[1] == 4 and c[-2] == 252 and c[-1] == 255
    assert RF.dims(256, 4) == (65, 64)
    assert list(RF.lattice_indices(10, 4)) == [0, 4, 8, 9]        # R not divisible: the last brick is thinner
    assert list(RF.lattice_indices(9, 4)) == [0, 4, 8]
    assert list(RF.lattice_indices(2, 8)) == [0, 1]               # R = 2, R < s: one brick
    assert list(RF.lattice_indices(5, 8)) == [0, 4]
    assert RF.default_band(256, 4) == pytest.approx(np.sqrt(3) * 4 / 255)
    for R, s in [(1, 4), (1291, 4), (64, 3), (64, 0), (64, 16)]:
        with pytest.raises(RF.hip.ListError):
            RF.dims(R, s)


def test_lattice_points_are_the_dense_grid_points():
    import torch
    from list_amd import utils
    for R, s in [(256, 4), (37, 8), (2, 2), (101, 2)]:
        c = RF.lattice_indices(R, s)
        dense = utils.grid_points_on_device(-0.5, 0.5, R, "cpu").view(R, R, R, 3)
        want = dense[np.ix_(c, c, c)].reshape(-1, 3)
        assert torch.equal(RF.lattice_points(R, s, "cpu"), want)
        K = len(c)
        assert torch.equal(RF.lattice_points(R, s, "cpu", 3, K ** 3 - 1), want[3:K ** 3 - 1])


# ---- classification -------------------------------------------------------------------------------------------------
def _lattice(K, value=10.0):
    return np.full((K, K, K), value, dtype=np.float32)


def test_active_by_sign_only():
    lat = _lattice(3)
    lat[0, 0, 0] = -10.0
    act, dil = RF.classify_cpu(lat, 0.0, 0.1)
    want = np.zeros((2, 2, 2), bool)
    want[0, 0, 0] = True
    assert np.array_equal(act, want)
    assert dil.all()
    lat[:] = -10.0
    lat[0, 0, 0] = 0.0                       # exactly on the level: outside (v > level is inside), no sign change
    act, _ = RF.classify_cpu(lat, 0.0, 0.0)
    assert not act.any()
    lat[0, 0, 0] = 1e-6
    act, _ = RF.classify_cpu(lat, 0.0, 0.0)
    assert np.array_equal(act, want)


def test_active_by_band_only():
    lat = _lattice(5)
    lat[4, 4, 4] = 0.05                      # same side as every other corner, inside the band
    act, dil = RF.classify_cpu(lat, 0.0, 0.1)
    want = np.zeros((4, 4, 4), bool)
    want[3, 3, 3] = True
    assert np.array_equal(act, want)
    act, dil = RF.classify_cpu(lat, 0.0, 0.05)      # |v - level| < band is strict
    assert not act.any() and not dil.any()


def test_nonfinite_corners_are_active():
    for bad in (np.nan, np.inf, -np.inf):
        lat = _lattice(4)
        lat[2, 1, 3] = bad
        act, _ = RF.classify_cpu(lat, 0.0, 0.1)
        want = np.zeros((3, 3, 3), bool)
        want[1:3, 0:2, 2:3] = True
        assert np.array_equal(act, want), bad


def test_level_other_than_zero():
    lat = _lattice(3, 1.0)
    act, _ = RF.classify_cpu(lat, 1.5, 0.1)          # all outside, 0.5 from the level
    assert not act.any()
    act, _ = RF.classify_cpu(lat, 0.95, 0.1)         # all inside, 0.05 from the level: the band
    assert act.all()
    lat[1, 1, 1] = 2.0
    act, _ = RF.classify_cpu(lat, 1.5, 0.1)          # the centre straddles 1.5: every brick holds it
    assert act.all()
    act, _ = RF.classify_cpu(lat, 2.5, 0.1)
    assert not act.any()


def test_dilation_at_the_faces():
    lat = _lattice(9)                                # NB = 8
    lat[0, 0, 0] = -1.0                              # brick (0,0,0) only: the dilation is clipped at three faces
    lat[8, 4, 8] = -1.0                              # bricks (7,3..4,7): clipped at two faces
    act, dil = RF.classify_cpu(lat, 0.0, 0.01)
    assert act.sum() == 3
    want = np.zeros((8, 8, 8), bool)
    want[0:2, 0:2, 0:2] = True
    want[6:8, 2:6, 6:8] = True
    assert np.array_equal(dil, want)


# ---- refined points -------------------------------------------------------------------------------------------------
def _brute_refined(dilated, R, s):
    """Plain loops: the non-lattice points of the closed extents of the dilated bricks."""
    c = list(RF.lattice_indices(R, s))
    m = np.zeros((R, R, R), bool)
    for bx, by, bz in zip(*np.nonzero(dilated)):
        m[c[bx]:c[bx + 1] + 1, c[by]:c[by + 1] + 1, c[bz]:c[bz + 1] + 1] = True
    m[np.ix_(c, c, c)] = False
    return np.flatnonzero(m.ravel())


@pytest.mark.parametrize("R,s", [(10, 4), (9, 4), (2, 4), (3, 8), (2, 2), (37, 8), (21, 2), (30, 4)])
def test_refined_points_match_brute_force(R, s):
    K, NB = RF.dims(R, s)
    rng = np.random.default_rng(R * 10 + s)
    for dil in (np.ones((NB,) * 3, bool), np.zeros((NB,) * 3, bool), rng.random((NB,) * 3) < 0.2):
        coords, idx = RF.refined_points_cpu(dil, R, s)
        want = _brute_refined(dil, R, s)
        assert idx.dtype == np.int32 and np.array_equal(idx, want)          # raster order
        axis = np.linspace(-0.5, 0.5, R).astype(np.float32)
        ijk = np.unravel_index(want, (R, R, R))
        assert np.array_equal(coords, np.stack([axis[t] for t in ijk], axis=1).reshape(-1, 3))
    assert len(RF.refined_points_cpu(np.ones((NB,) * 3, bool), R, s)[1]) == R ** 3 - K ** 3


def test_refined_points_counts():
    assert len(RF.refined_points_cpu(np.ones((1, 1, 1), bool), 2, 4)[1]) == 0      # every point is a lattice point
    assert len(RF.refined_points_cpu(np.ones((1, 1, 1), bool), 3, 8)[1]) == 27 - 8
    one = np.zeros((3, 3, 3), bool)
    one[0, 0, 0] = True
    assert len(RF.refined_points_cpu(one, 10, 4)[1]) == 125 - 8
    one[:] = False
    one[2, 2, 2] = True                                                       # the thin brick [8, 9]^3
    assert len(RF.refined_points_cpu(one, 10, 4)[1]) == 0


# ---- fill -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,s", [(10, 4), (37, 8), (2, 4), (21, 2)])
def test_fill(R, s):
    c = RF.lattice_indices(R, s)
    ax = np.arange(R, dtype=np.float64)
    dense = (0.25 * ax[:, None, None] - 0.5 * ax[None, :, None] + 0.125 * ax[None, None, :] + 3.0).astype(np.float32)
    lat = dense[np.ix_(c, c, c)]
    on = np.zeros((R, R, R), bool)
    on[np.ix_(c, c, c)] = True
    free = np.flatnonzero(~on.ravel())
    idx = np.unique(free[[0, len(free) // 2, -1]]).astype(np.int32) if len(free) else np.zeros(0, np.int32)
    vals = np.full(idx.shape, 123.0, np.float32)
    vol = RF.fill_cpu(lat, vals, idx, R, s)
    assert vol.shape == (R, R, R) and vol.dtype == np.float32
    assert np.array_equal(vol[np.ix_(c, c, c)], lat)                         # lattice points: their values
    assert np.array_equal(vol.reshape(-1)[idx], vals)                        # refined points: theirs
    rest = ~on.ravel()
    rest[idx] = False
    # the others: trilinear interpolation, which reproduces an affine field (to rounding)
    if rest.any():
        assert np.abs(vol.reshape(-1)[rest] - dense.reshape(-1)[rest]).max() <= 1e-5 * np.abs(dense).max()


def test_fill_stays_on_the_side_of_an_inactive_brick():
    rng = np.random.default_rng(3)
    R, s = 37, 4
    K, NB = RF.dims(R, s)
    band = np.float32(RF.default_band(R, s))
    lat = rng.random((K, K, K)).astype(np.float32) + band
    lat[:, :, K // 2:] *= -1
    act, dil = RF.classify_cpu(lat, 0.0, band)
    assert act.any() and not act.all()
    coords, idx = RF.refined_points_cpu(dil, R, s)
    vol = RF.fill_cpu(lat, np.zeros(len(idx), np.float32), idx, R, s)
    assert np.isfinite(vol).all()
    c = RF.lattice_indices(R, s)
    refined = RF.refined_mask_cpu(dil, R, s)
    for b in zip(*np.nonzero(~act)):
        corners = lat[b[0]:b[0] + 2, b[1]:b[1] + 2, b[2]:b[2] + 2]
        ext = tuple(slice(c[b[a]], c[b[a] + 1] + 1) for a in range(3))
        box = vol[ext][~refined[ext]]                  # the filled points of the brick (refined ones were queried)
        assert box.size and ((box > 0) == (corners[0, 0, 0] > 0)).all() and (box != 0).all()


# ---- the guarantee ----------------------------------------------------------------------------------------------------
def _sphere(R, r=0.35):
    a = np.linspace(-0.5, 0.5, R)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return (r - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def _reader(dense):
    R = dense.shape[0]

    def query(pts):                                   # the exact dense value at each grid point
        p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        ijk = np.rint((p + 0.5) * (R - 1)).astype(np.int64)
        return dense[ijk[:, 0], ijk[:, 1], ijk[:, 2]]
    return query


@pytest.mark.parametrize("s", [2, 4, 8])
def test_refined_sphere_mesh_equals_the_dense_mesh(s):
    R = 96
    dense = _sphere(R)
    vol, st = RF.predict_grid_refined(_reader(dense), R, s, device="cpu", step=50000)
    assert st["lattice"] == RF.dims(R, s)[0] ** 3 and st["queried"] == st["lattice"] + st["refined"]
    assert st["fraction"] < 1.0                       # (a coarse stride on a 96^3 grid refines most of it)
    v0, f0 = mesh.marching_cubes_cpu(dense)
    v1, f1 = mesh.marching_cubes_cpu(vol)
    assert len(f0) > 1000
    assert np.array_equal(v0, v1) and np.array_equal(f0, f1)
    # at a level other than 0 too: the classification follows it
    vol, _ = RF.predict_grid_refined(_reader(dense), R, s, level=0.1, device="cpu")
    v0, f0 = mesh.marching_cubes_cpu(dense, 0.1)
    v1, f1 = mesh.marching_cubes_cpu(vol, 0.1)
    assert np.array_equal(v0, v1) and np.array_equal(f0, f1)


def test_refine_cli_flags():
    from list_amd import arguments
    cfg = arguments.default_config()
    assert cfg.refine_stride == 0 and cfg.refine_band is None
    cfg = arguments.get_args(["--refine_stride", "4", "--refine_band", "0.02"])
    assert cfg.refine_stride == 4 and cfg.refine_band == 0.02
    with pytest.raises(SystemExit):
        arguments.get_args(["--refine_stride", "3"])


# ---- C ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return RF.load()


def test_library_exports_the_refine_symbols(lib):
    from list_amd import build, hip
    assert "list_refine.h" in build.PUBLIC_HEADERS and "refine_kernels.hip" in build.SOURCES
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9
    assert "#define LIST_REFINE_MAX_R 1290" in open(os.path.join(ROOT, "include", "list_refine.h")).read()
    assert 1290 ** 3 <= 2 ** 31 - 1 < 1291 ** 3


def test_refusals_come_before_any_hip_call(lib):
    fake = 256                                    # never dereferenced: every refusal below is a host check
    err = lambda: lib.list_refine_last_error()
    assert lib.list_refine_workspace_bytes(1291, 4) == 0 and b"INT32_MAX" in err()
    assert lib.list_refine_workspace_bytes(1, 4) == 0 and b"R = 1" in err()
    assert lib.list_refine_workspace_bytes(64, 3) == 0 and b"s = 3" in err()
    assert lib.list_refine_mask_offset(64, 3) == 0
    assert lib.list_refine_mask_offset(256, 4) == 64 ** 3                    # host arithmetic: NB^3 rounded to 256
    assert lib.list_refine_mask_offset(10, 4) == 256

    def count(R=64, s=4, lat=fake, level=0.0, band=0.1, ws=fake, tot=fake):
        return lib.list_refine_count(lat, R, s, level, band, ws, 1 << 40, tot, None)
    assert count(R=1291) == -2 and b"INT32_MAX" in err()
    assert count(s=5) == -2 and b"s = 5" in err()
    assert count(lat=None) == -1 and b"NULL" in err()
    assert count(tot=None) == -1
    assert count(ws=None) == -1 and b"workspace" in err()
    assert count(level=float("nan")) == -1 and b"level" in err()
    assert count(band=-1.0) == -1 and b"band" in err()
    assert count(band=float("nan")) == -1 and b"band" in err()

    def emit(R=64, s=4, lo=-0.5, hi=0.5, ws=fake, c=fake, i=fake, n=10):
        return lib.list_refine_emit(R, s, lo, hi, ws, 1 << 40, c, i, n, None)
    assert emit(R=2000) == -2 and b"INT32_MAX" in err()
    assert emit(n=-1) == -1 and b"n = -1" in err()
    assert emit(n=64 ** 3 + 1) == -1 and b"exceeds" in err()
    assert emit(c=None) == -1 and b"NULL" in err()
    assert emit(hi=float("inf")) == -1 and b"finite" in err()
    assert emit(ws=None) == -1 and b"workspace" in err()

    def fill(R=64, s=4, lat=fake, val=fake, n=10, ws=fake, vol=fake):
        return lib.list_refine_fill(lat, val, n, R, s, ws, 1 << 40, vol, None)
    assert fill(s=1) == -2
    assert fill(lat=None) == -1 and b"NULL" in err()
    assert fill(vol=None) == -1
    assert fill(val=None) == -1 and b"values" in err()
    assert fill(n=-3) == -1
    assert fill(ws=None) == -1 and b"workspace" in err()


def test_device_wrappers_refuse_host_tensors():
    import torch
    with pytest.raises(RuntimeError):
        RF.count(torch.zeros(17, 17, 17), 64, 4)
    with pytest.raises(ValueError):
        RF.predict_grid_refined(lambda p: np.zeros(p.shape[1], np.float32), 16, 4, band=-1.0, device="cpu")
