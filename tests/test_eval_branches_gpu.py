"""GPU: the evaluation kernels (eval_kernels.hip) on every dispatch branch and border.

  * contains_kernel and its hash against the answers of the reference's own code (tests/golden/eval_ref.npz, cases in
    tests/_eval_cases.py): narrow windows of exactly kMaxNarrow = 8 cells, with and without a wide list, kx != ky,
    windows cut off at row / column 0, hash_res 33, 17 (all wide), 2 and 1, query points on cell borders, on the faces
    of the scaled box, NaN and infinite.  The device must equal the fixture and the numpy restatement, point by point.
  * nn_kernel<R> at the borders of list_eval_nn's rule (the most points per lane that still gives 1024 workgroups),
    where R changes and the last workgroup keeps lanes whose slots lie past N.
"""
import functools
import os

import numpy as np
import pytest
import torch

import _eval_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_ref.npz"))


def _E():
    from list_amd import evaluate
    return evaluate


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the inside test --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.CASE_NAMES)
def test_inside_test_matches_reference(golden, name):
    E = _E()
    c = EC.build(name)                                            # asserts the case's own property (widths, wide list)
    assert c.sha256 == str(golden[name + ".sha256"]), "the inputs are not the ones the reference was run on"
    ref, _ = EC.unpack(golden, name)
    v, f, q = _t(c.verts), _t(c.faces), _t(c.points)
    contains, hole = (x.cpu().numpy() for x in E.mesh_contains(v, f, q, hash_res=c.res))
    occ, rest = (x.cpu().numpy() for x in E.implicit_waterproofing(v, f, q, hash_res=c.res))
    with np.errstate(invalid="ignore"):
        r_contains, r_hole = E.mesh_contains_cpu(c.verts, c.faces, c.points, hash_res=c.res)
        r_occ, r_rest = E.implicit_waterproofing_cpu(c.verts, c.faces, c.points, hash_res=c.res)
    for got, restated, key in ((contains, r_contains, "contains"), (hole, r_hole, "hole"), (occ, r_occ, "occ"),
                               (rest, r_rest, "rest")):
        np.testing.assert_array_equal(got, ref[key], err_msg=f"{name}: device {key} against the reference")
        np.testing.assert_array_equal(got, restated, err_msg=f"{name}: device {key} against the restatement")


def test_nan_vertex_is_refused():
    E = _E()
    from list_amd import hip
    c = EC.build("soup33_narrow")
    v = c.verts.copy()
    v[7, 1] = np.nan
    with pytest.raises(hip.ListError) as host:
        E.mesh_contains_cpu(v, c.faces, c.points[:100], hash_res=c.res)
    with pytest.raises(hip.ListError) as dev:
        E.mesh_contains(_t(v), _t(c.faces), _t(c.points[:100]), hash_res=c.res)
    assert dev.value.code == host.value.code == hip.ERR_SHAPE
    torch.cuda.synchronize()


# ---- nearest neighbours at the dispatch borders -------------------------------------------------------------------------
# list_eval_nn: R = 4 when ceil(N / 1024) >= 1024, else R = 2 when ceil(N / 512) >= 1024, else R = 1
NN_BORDERS = {523_776: 1, 523_777: 2, 1_047_552: 2, 1_047_553: 4}
NN_MAX = max(NN_BORDERS)
NN_TAIL = 2000


def _expected_R(n):
    return 4 if -(-n // 1024) >= 1024 else 2 if -(-n // 512) >= 1024 else 1


@functools.lru_cache(maxsize=None)
def _nn_clouds(M):
    """dst [M,3] with every point of its first half repeated in the second, and src [NN_MAX,3]: every third point an
    exact copy of a dst point (distance 0, reached by two indices), the others uniform; the NN_TAIL points before each
    border are all uniform.  A prefix src[:N] is the cloud of border N."""
    E = _E()
    dst = E.box_samples_cpu(M, -0.5, 0.5, 40 + M).astype(np.float32)
    dst[M - M // 2:] = dst[:M // 2]
    src = E.box_samples_cpu(NN_MAX, -0.5, 0.5, 41 + M).astype(np.float32)
    i = np.arange(NN_MAX)
    copy = i % 3 == 0
    for n in NN_BORDERS:
        copy[n - NN_TAIL:n] = False
    src[copy] = dst[(i[copy] // 3) % M]
    tail = src[NN_MAX - NN_TAIL:]
    assert len(np.unique(tail, axis=0)) == NN_TAIL and not (tail[:, None, :] == dst[None, :, :]).all(-1).any()
    return src, dst


@functools.lru_cache(maxsize=None)
def _nn_reference(M):
    """(float64 distances by cKDTree, indices by the float32 first-minimum rule of test_eval_gpu._nn_brute in chunks)."""
    src, dst = _nn_clouds(M)
    dist, _ = _E().nn_distance_cpu(src, dst)
    idx = np.empty(NN_MAX, dtype=np.int64)
    d = [np.ascontiguousarray(dst[None, :, k]) for k in range(3)]
    for s in range(0, NN_MAX, 1 << 14):
        p = src[s:s + (1 << 14)]
        dx, dy, dz = (p[:, None, k] - d[k] for k in range(3))
        idx[s:s + (1 << 14)] = np.argmin((dx * dx + dy * dy) + dz * dz, axis=1)   # the first minimum: the smallest j
    return dist, idx


@functools.lru_cache(maxsize=None)
def _nn_device(M):
    src, dst = _nn_clouds(M)
    return _t(src), _t(dst)


@pytest.mark.parametrize("M", [1, 257, 513])
@pytest.mark.parametrize("N", sorted(NN_BORDERS))
def test_nn_distance_dispatch_borders(N, M):
    """One evaluate.nn_distance call is one list_eval_nn launch.  R per N: 523 776 -> 1 (2046 full workgroups),
    523 777 -> 2 and 1 047 553 -> 4 (1024 workgroups, the last with one point: every other slot is past N),
    1 047 552 -> 2 (2046 full workgroups).  M = 1, one point past an LDS tile, one past two.  Every element."""
    assert _expected_R(N) == NN_BORDERS[N] and _expected_R(N - 1) <= NN_BORDERS[N]
    src, dst = _nn_device(M)
    ref_d, ref_i = _nn_reference(M)
    d, i = _E().nn_distance(src[:N], dst)
    assert d.shape == i.shape == (N,)
    np.testing.assert_allclose(d.cpu().numpy(), ref_d[:N], rtol=1e-6, atol=1e-12)
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i[:N])
    if M > 1:                                                     # the ties were there to be decided
        zero = np.flatnonzero(ref_d[:N] == 0)
        assert zero.size > N // 4 and np.all(ref_i[zero] < M - M // 2)


def test_eval_pointcloud_four_points_per_lane():
    """A 1 047 553-point prediction against 300 ground-truth points: accuracy runs nn_kernel<4>, completeness
    nn_kernel<1> over 4093 dst tiles.  Bounds of test_eval_mesh_gpu_vs_cpu."""
    E = _E()
    n = NN_MAX
    pred = E.box_samples_cpu(n, -0.5, 0.5, 50).astype(np.float32)
    gt = E.box_samples_cpu(300, -0.5, 0.5, 51).astype(np.float32)
    g = E.eval_pointcloud(_t(pred), _t(gt))
    c = E.eval_pointcloud_cpu(pred, gt)
    assert set(g) == set(c)
    for k in c:
        if k.startswith(("precision", "recall")):
            assert abs(g[k] - c[k]) * n <= 3, (k, g[k], c[k])
    for k in ("completeness", "accuracy", "completeness2", "accuracy2", "chamfer_l2"):
        assert g[k] == pytest.approx(c[k], rel=1e-3), k
    assert c["recall_0.5"] > 0 and c["precision_5.0"] > 0
