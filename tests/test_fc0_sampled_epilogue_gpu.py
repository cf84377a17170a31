"""GPU: fc_0 of an fp16 inference forward on list_prep_img_proj's map as the 256 x 256 ping-pong GEMM whose epilogue
samples the projected channels from the map (k_gemm_nt_pp, EPI_RELU_SAMPLE; the kept channels come from X, written by
the kept-channels-only form of k_gather_img in Morton order) against the row-vector pair (ListQueryArgs.no_fused_fc0 =
1: k_gather_img samples all 640 channels in pixel order and writes fp32 row vectors, the GEMM's epilogue reads them):
the same products in the same order and the sample added to the same sum, so the SDF is the same BIT FOR BIT -- on the
golden cases (non-finite map values and their exact redo, NaN coordinates, points on and beyond the clamp), on BASELINE
configs 2 and 5 at full size (config 5: map 274^2, two row chunks), sorted and unsorted queries, and a batch split in
two calls against one call.  Each side runs in a process of its own.
Reference call sites replaced: network/modules.py:46-53 (bilinear sample), :275-276 (concat + fc_0 + ReLU)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run(tmp_path, side):
    out = os.path.join(tmp_path, f"fc0_{side}.npz")
    env = dict(os.environ)
    env.pop("LIST_FUSED_FC0", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_fc0_sampled.py"), out, side],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def _bits(a):
    # torch.equal on the raw bits: NaN positions (and NaN payloads) count too
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32)


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fc0_sampled"))
    return _run(d, "sampled"), _run(d, "rowvec")


def test_what_the_library_dispatched(sides):
    new, old = sides
    assert int(new["config2_plan_fused_fc0"]) == 1 and int(new["config2_plan_img_proj"]) == 1
    assert int(new["config2_plan_fc0_k"]) == 2752
    assert int(old["config2_plan_fused_fc0"]) == 0 and int(old["config2_plan_img_proj"]) == 1
    assert int(old["config2_plan_fc0_k"]) == 2752
    assert int(new["config5_plan_chunks"]) == 2 and int(new["config5_plan_fused_fc0"]) == 1
    for tag in ("tiny", "small", "real", "edge", "edge_nan", "small_nan_coord", "small_on_clamp"):
        assert int(new[f"{tag}_plan_fused_fc0"]) == 1 and int(old[f"{tag}_plan_fused_fc0"]) == 0, tag


def test_sampling_epilogue_equals_the_row_vector_pair_bit_for_bit(sides):
    new, old = sides
    keys = sorted(k for k in new.files if "_plan_" not in k)
    assert keys == sorted(k for k in old.files if "_plan_" not in k)
    # 7 cases x (sorted, unsorted) + config 2 / 5 x (sorted, unsorted, split) + small split
    assert len(keys) == 7 * 2 + 2 * 3 + 1, keys
    for k in keys:
        assert new[k].shape == old[k].shape
        assert torch.equal(_bits(new[k]), _bits(old[k])), (k, float(np.nanmax(np.abs(new[k] - old[k]))))
    # the cases hold what they are meant to hold
    assert np.isfinite(new["config2_sorted"]).all() and np.abs(new["config2_sorted"]).max() > 1e-3
    assert np.isfinite(new["config5_sorted"]).all() and np.abs(new["config5_sorted"]).max() > 1e-3
    assert np.isnan(new["small_nan_coord_sorted"][0, 3]) and np.isnan(new["small_nan_coord_sorted"]).sum() == 1
    assert np.isnan(new["edge_nan_sorted"]).any() and np.isfinite(new["edge_nan_sorted"]).any()
    assert not np.array_equal(new["small_on_clamp_sorted"], new["small_sorted"])


def test_sorted_unsorted_and_split_queries_agree_within_the_path(sides):
    """The order of the rows and the composition of the row tiles do not change a point's value."""
    new, _ = sides
    for tag in ("small", "config2", "config5"):
        assert torch.equal(_bits(new[f"{tag}_sorted"]), _bits(new[f"{tag}_unsorted"])), tag
    for tag in ("small", "config2", "config5"):
        assert torch.equal(_bits(new[f"{tag}_split"]), _bits(new[f"{tag}_sorted"])), tag
