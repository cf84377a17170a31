"""CPU: which kernel forms the gradient of each voxel level, on which stream, flushing how -- plan_vox_adjoint
(csrc/vox_adjoint_plan.h), the rule launch_scatter_vox executes.  Every form gives the right gradient, only slower or at
another precision grade, so nothing else would notice a level taking another one.  The header is built by a host compiler
with -I include -I csrc alone (tests/csrc/vox_adjoint_plan_host.cpp) and asked for the calls below; the expected rows are
literals, one entry form/lane/flush per level l0 .. l5:
  win9, win18   LDS window of 9216 / 18432 floats;      w0, w1   slot 0 / 1 of the window levels' fp16 scratch
  h16           the direct level's fp16 scratch;         f32      fp32 atomics behind a memset;     st   plain store"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vox_plan as VP  # noqa: E402

SCA, DIR, G8 = "scalar/direct/f32", "direct/direct/f32", "gather8/gather/st"
H2 = "direct_h2/direct/h16"
WORK = dict(B=8, N=20000)                       # the benchmark's training step
ONE = dict(B=1, N=6000, forked=False)           # test_box_adjoint_gpu.py's one_image
CASES = {
    # name: (call, expected l0 .. l5)
    "workload": (VP.case(**WORK), [SCA, DIR, H2, G8, "box/window/w0", "win9/window2/w1"]),
    "workload_inline": (VP.case(**WORK, forked=False), [SCA, DIR, H2, G8, "box/window/w0", "box/window2/w1"]),
    "workload_f32dx": (VP.case(**WORK, fp16=False), [SCA, DIR, DIR, G8, "box/window/f32", "win9/window2/f32"]),
    "D_f32dx_inline": (VP.case(**WORK, fp16=False, forked=False), [SCA, DIR, DIR, G8, "box/window/f32", "box/window2/f32"]),
    "scatter_mode": (VP.case(**WORK, mode=1), [SCA, DIR, DIR, DIR, "win18/window/f32", "win9/window2/f32"]),
    "gather_mode": (VP.case(**WORK, mode=2), [SCA, DIR, G8, G8, G8, G8]),
    "B_gather_mode_no_buffers": (VP.case(**WORK, mode=2, gather_buffers=False),
                                 [SCA, DIR, DIR, DIR, "win18/direct/f32", "win9/direct/f32"]),
    "A_small_scratch": (VP.case(B=8, N=2000), [SCA, DIR, DIR, DIR, "win18/window/f32", "win9/window2/w0"]),
    "C_offsets_plus_4": (VP.case(**WORK, shift=4), [SCA, DIR, H2, "gather1/gather/st", "win18/window/w0", "win9/window2/w1"]),
    "box_mode_1": (VP.case(**WORK, box_mode=1), [SCA, DIR, H2, G8, "win18/window/w0", "box/window2/w1"]),
    "box_mode_3": (VP.case(**WORK, box_mode=3), [SCA, DIR, H2, G8, "box/window/w0", "win9/window2/w1"]),
    "box_mode_0_inline": (VP.case(**WORK, forked=False, box_mode=0), [SCA, DIR, H2, G8, "win18/window/w0", "win9/window2/w1"]),
    "one_image": (VP.case(**ONE), [SCA, DIR, DIR, H2, "box/window/w0", "box/window2/w1"]),
    "one_image_box2_f32": (VP.case(**ONE, box_mode=2, f32=True), [SCA, DIR, DIR, H2, "box/window/f32", "box/window2/f32"]),
    "one_image_box0_f32": (VP.case(**ONE, box_mode=0, f32=True), [SCA, DIR, DIR, H2, "win18/window/f32", "win9/window2/f32"]),
    "two_images": (VP.case(B=2, N=9000, forked=False), [SCA, DIR, DIR, H2, "box/window/w0", "box/window2/w1"]),
    "F_three_window_levels": (VP.case(B=2, N=500, R=32), [SCA, DIR, H2, "win9/window/w0", "win9/window2/w1", "win9/window2/f32"]),
    "G_small_gather_mode": (VP.case(B=2, N=300, R=32, fp16=False, forked=False, mode=2), [SCA, G8, G8, G8, G8, G8]),
    # edges, on the workload's call
    "null_level": (VP.case(**WORK, edits=["l3.null"]), [SCA, DIR, H2, "skip", "box/window/w0", "win9/window2/w1"]),
    # images not back to back: no packed-half form (the 16^3 level then keeps the window kernel's fp32 flush, and the 8^3
    # level is the first to take a slot)
    "padded_images": (VP.case(**WORK, edits=["l2.stride+64", "l4.stride+64"]),
                      [SCA, DIR, DIR, G8, "win18/window/f32", "win9/window2/w0"]),
    "four_channels": (VP.case(**WORK, edits=["l1.C=4"]), [SCA, DIR, H2, G8, "box/window/w0", "win9/window2/w1"]),
    "eight_channels": (VP.case(**WORK, edits=["l1.C=8"]), [SCA, DIR, H2, G8, "box/window/w0", "win9/window2/w1"]),
    # channel counts the dispatch does not know: launch_scatter_vox answers hipErrorInvalidValue (a window level still
    # counts as the first one seen)
    "unknown_channels": (VP.case(**WORK, edits=["l2.C=48"]), [SCA, DIR, "invalid/direct/f32", G8, "box/window/w0", "win9/window2/w1"]),
    "unknown_window_channels": (VP.case(**WORK, edits=["l4.C=96"]), [SCA, DIR, H2, G8, "invalid/window/f32", "win9/window2/w0"]),
}


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    exe = VP.build_host(tmp_path_factory.mktemp("vox_plan"))
    return VP.plans(exe, {name: call for name, (call, _) in CASES.items()})


@pytest.mark.parametrize("name", list(CASES))
def test_every_level_takes_the_expected_form_lane_and_flush(got, name):
    print(name, got[name])
    assert got[name] == CASES[name][1]


def test_the_header_includes_only_the_c_abi_and_standard_headers():
    text = open(os.path.join(VP.CSRC, "vox_adjoint_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", '"list_hip.h"']
    assert "getenv" not in text
