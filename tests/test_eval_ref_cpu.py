"""CPU: the numpy restatement of the inside test and of the point-cloud metrics (evaluate.*_cpu) against the answers of
the reference's own code (evaluation/libmesh, implicit_waterproofing.py, eval_util.py), recorded in
tests/golden/eval_ref.npz by `python -m oracle.gen_eval_golden` on the cases of tests/_eval_cases.py.  Every point of
every case is compared; the device is held to the same file in tests/test_eval_branches_gpu.py."""
import os

import numpy as np
import pytest

import _eval_cases as EC
from list_amd import evaluate as E
from list_amd import hip


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_ref.npz"))


def test_fixture_is_not_empty(golden):
    """The counts the generator asserted when it wrote the file: every soup (bar hash_res 1, which collapses every
    triangle to a point) has inside points and holes, and the retry cases keep holes after the third rotation."""
    assert set(EC.RETRY_NAMES) <= set(EC.NONEMPTY_NAMES)
    for name in EC.CASE_NAMES:
        _, counts = EC.unpack(golden, name)
        if name in EC.NONEMPTY_NAMES:
            assert counts["contains"] > 0 and counts["hole"] > 0, (name, counts)
        if name in EC.RETRY_NAMES:
            assert counts["rest"] > 0, (name, counts)
    assert EC.unpack(golden, "soup1")[1] == dict.fromkeys(EC.FLAG_KEYS, 0)
    assert EC.unpack(golden, "sphere24_open")[1]["hole"] > 1000 and EC.unpack(golden, "sphere24_open")[1]["rest"] == 0


@pytest.mark.parametrize("name", EC.CASE_NAMES)
def test_inside_test_cpu_matches_reference(golden, name):
    c = EC.build(name)                                            # asserts the case's own property (widths, wide list)
    assert c.sha256 == str(golden[name + ".sha256"]), "the inputs are not the ones the reference was run on"
    ref, _ = EC.unpack(golden, name)
    assert len(ref["contains"]) == len(c.points)
    with np.errstate(invalid="ignore"):
        contains, hole = E.mesh_contains_cpu(c.verts, c.faces, c.points, hash_res=c.res)
        occ, rest = E.implicit_waterproofing_cpu(c.verts, c.faces, c.points, hash_res=c.res)
    np.testing.assert_array_equal(contains, ref["contains"])
    np.testing.assert_array_equal(hole, ref["hole"])
    np.testing.assert_array_equal(occ, ref["occ"])
    np.testing.assert_array_equal(rest, ref["rest"])


@pytest.mark.parametrize("name", EC.CLOUD_NAMES)
def test_eval_pointcloud_cpu_matches_reference(golden, name):
    """Exact, key by key: both sides hand the same float32 clouds to cKDTree and reduce its float64 distances with the
    same numpy calls."""
    assert EC.clouds_sha256(name) == str(golden[f"pc.{name}.sha256"])
    pred, gt = EC.clouds(name)
    got = E.eval_pointcloud_cpu(pred, gt)
    ref = dict(zip((str(k) for k in golden[f"pc.{name}.keys"]), golden[f"pc.{name}.values"].tolist()))
    assert set(got) == set(ref)
    for k in sorted(ref):
        assert got[k] == ref[k], (k, got[k], ref[k], got[k] - ref[k])
    assert ref["precision_0.5"] > 0 and ref["recall_0.5"] > 0


def test_nan_vertex_is_refused_cpu():
    c = EC.build("soup33_narrow")
    v = c.verts.copy()
    v[7, 1] = np.nan
    with pytest.raises(hip.ListError) as e:
        E.mesh_contains_cpu(v, c.faces, c.points[:100], hash_res=c.res)
    assert e.value.code == hip.ERR_SHAPE
