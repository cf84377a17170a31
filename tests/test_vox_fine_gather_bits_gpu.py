"""k_gather_vox (csrc/gather_kernels.hip) bit for bit against recorded results: the fine voxel levels' kernel holds the
results of a pair of stencil points and stores them behind the next pair's loads -- the order of its memory instructions
is a matter of speed, the arithmetic is not: every feature column and the SDF keep the bits they had before.

tests/golden/vox_fine_gather_digests.json holds the SHA-256 of those bits (NaN positions and payloads included) as the
kernel computed them when it stored every sample at once, written by tests/_child_vox_fine_gather.py run as a program.
Cases (there): two pyramids whose six levels all take k_gather_vox -- cubes of 56 (with the scalar level riding), 40, 32,
29 and 57 voxels at 16 / 32 / 64 channels, and bricks (24 x 40 x 32 ...) at 8 ... 256 channels, the 64-channel one
carrying the scalar level; fp16 maps and operands, and fp32 maps (bf16x3); 2 x 300 points: uniform ones, lattice positions and their float32
neighbours on every axis, faces and corners and beyond, a NaN coordinate; sorted, unsorted and training forwards; and
the same with +-inf / NaN voxels under the taps (the exact redo of the flagged tiles)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vox_fine_gather_digests.json")


@pytest.fixture(scope="module")
def got():
    sys.path.insert(0, HERE)
    import _child_vox_fine_gather as child
    return child.run()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_cases_are_the_recorded_ones(got, want):
    assert sorted(got) == sorted(want)
    assert len(want) == 2 * 2 * (7 + 3 + 2)           # pyramids x precisions x (feature blocks + clean SDFs + spoiled SDFs)


@pytest.mark.parametrize("pyramid", ["cubes", "bricks"])
@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
def test_features_and_sdf_keep_their_bits(got, want, pyramid, precision):
    keys = [k for k in want if k.startswith(f"{pyramid}/{precision}/")]
    assert keys
    differing = [k for k in keys if got[k] != want[k]]
    print(f"{pyramid}/{precision}: {len(keys) - len(differing)} of {len(keys)} digests equal")
    assert not differing, differing
