"""GPU: the matrix-core adjoint of the coarse voxel levels (k_scatter_vox_box, csrc/bwd_box_kernels.hip; the reference's autograd of
network/modules.py:256-265 for the 16^3 and 8^3 x 128-channel levels, fp16 operands) against the LDS-window kernel it replaces.

Both consume the SAME dX (everything before the voxel adjoint is deterministic) and flush packed halfs into the same fp16 image, so they
differ by the order of the fp32 sums inside a run and by how the sums are cut into flushes; every flush-add rounds the voxel's running
sum to 11 bits, and a voxel of these levels receives tens of flushes: two runs of the SAME kernel differ by 1 - 2e-3 of a level's largest
entry (measured; the order of the atomics), so the bound is 6e-3 (3e-3 in L2) -- against O(0.1 .. 1) for any error in a tap, a weight or
a run's box.  (The packed-half flush, hence the matrix-core kernel, needs the level's fp16 image to fit the call's scratch: at least
4 096 rows per image, so there is no few-points form of this test.)  The library reads LIST_SCATTER_BOX once per process, so each side
comes from a process of its own (this file run as a script): 0 = window kernels, 2 = matrix-core kernel on both levels.  The sharp
comparison is the fp32-flush form below."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

WANT = dict(want_mlp=False, want_img=False, want_trans=False)
CASES = {"one_image": dict(seed=8181, batch=1, n=6000), "two_images": dict(seed=8282, batch=2, n=9000)}


def coarse_level_gradients(case, overlap, precision="fp16"):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    ge.build()
    from list_amd import hip
    from oracle import cases, synth
    from test_hip_backward import hip_gradients
    hip.load()
    k = CASES[case]
    c = cases._case(seed=k["seed"], batch=k["batch"], n=k["n"], img_res=64, vox_res=128)   # levels 4, 5: 16^3 and 8^3 x 128 channels
    gs = synth.normalish(k["seed"] + 1, (k["batch"], k["n"]))
    _, g = hip_gradients(hip, c, gs, precision, want=dict(WANT, overlap=overlap))
    return {k2: g[k2] for k2 in ("d_vox3", "d_vox4", "d_vox5")}


def rel_max(a, ref):
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


def other_process(tmp, mode, case, overlap, f32=False, precision="fp16"):
    out = os.path.join(tmp, f"{case}_{mode}_{int(overlap)}_{int(f32)}_{precision}.npz")
    env = dict(os.environ, LIST_SCATTER_BOX=str(mode), LIST_SCATTER_F32="1" if f32 else "0",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, case, str(int(overlap)), precision], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(out))


def test_the_fp16_images_of_both_levels_fit_the_scratch_in_these_cases(tmp_path):
    """(What makes a window level take the packed-half flush, hence the matrix-core kernel: two window levels share rows x H2
    halfs of scratch.  The rule itself is asked -- csrc/vox_adjoint_plan.h, which launch_scatter_vox executes, through the
    host program of tests/test_vox_adjoint_plan_cpu.py: levels 4 and 5 take a slot each, in line and forked.)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _vox_plan as VP
    got = VP.plans(VP.build_host(tmp_path), {f"{name}_{int(forked)}": VP.case(B=k["batch"], N=k["n"], forked=forked)
                                             for name, k in CASES.items() for forked in (False, True)})
    assert len(got) == 2 * len(CASES)
    for name, levels in got.items():
        assert levels[4].endswith("/window/w0") and levels[5].endswith("/window2/w1"), (name, levels)


@pytest.mark.parametrize("case,bound", [("one_image", 6e-3), ("two_images", 6e-3)])
@pytest.mark.parametrize("overlap", [False, True])
def test_matrix_core_adjoint_equals_the_window_kernel_up_to_flush_rounding(tmp_path, case, bound, overlap):
    win = other_process(str(tmp_path), 0, case, overlap)
    box = other_process(str(tmp_path), 2, case, overlap)
    for k in ("d_vox4", "d_vox5"):
        assert np.isfinite(box[k]).all(), k
        assert np.abs(win[k]).max() > 0
        assert rel_max(box[k], win[k]) < bound, (k, rel_max(box[k], win[k]))
        l2 = float(np.linalg.norm((box[k] - win[k]).ravel()) / np.linalg.norm(win[k].ravel()))
        assert l2 < bound / 2, (k, l2)
    assert rel_max(box["d_vox3"], win["d_vox3"]) < bound               # (64 channels: the window kernel either way)
    # ... and the library's default choice in THIS process (16^3 level on the matrix cores; 8^3 too when not forked)
    got = coarse_level_gradients(case, overlap)
    for k in ("d_vox4", "d_vox5"):
        assert rel_max(got[k], win[k]) < bound, (k, rel_max(got[k], win[k]))


@pytest.mark.parametrize("case", ["one_image", "two_images"])
def test_matrix_core_adjoint_equals_the_window_kernel_when_both_flush_fp32(tmp_path, case):
    """The sharp form: LIST_SCATTER_F32=1 (diagnostic) makes both kernels add their UNROUNDED fp32 sums into the fp32 gradient, so
    what is left between them is the order of fp32 additions -- 5e-7 of a level's largest entry, where a wrong tap, weight, slot or
    box row would show at 1e-2 .. 1.  (The shipped packed-half flush rounds the same accumulators.)"""
    win = other_process(str(tmp_path), 0, case, False, f32=True)
    box = other_process(str(tmp_path), 2, case, False, f32=True)
    for k in ("d_vox4", "d_vox5"):
        assert np.abs(win[k]).max() > 0
        assert rel_max(box[k], win[k]) < 5e-6, (k, rel_max(box[k], win[k]))     # measured 3 - 5e-7 (the window kernel twice: 2 - 3e-7)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_split_operand_adjoint_equals_the_window_kernel_to_its_products_grade(tmp_path, precision):
    """The formats whose dX is fp32 (k_scatter_vox_box<ADJ_SPLIT>, bwd_box_kernels.hip): both kernels add fp32 sums into the fp32
    gradient; the window kernel multiplies in fp32, the matrix-core kernel takes bf16 hi + lo of both operands (three products,
    16 mantissa bits each way -- the grade of the forward's bf16x3 GEMMs): 3 - 6e-6 of a level's largest entry measured, against
    2e-7 for the window kernel twice and 2e-4 for the bf16x3 path's stated bound."""
    for case in CASES:
        win = other_process(str(tmp_path), 0, case, False, precision=precision)
        box = other_process(str(tmp_path), 2, case, False, precision=precision)
        for k in ("d_vox4", "d_vox5"):
            assert np.abs(win[k]).max() > 0
            assert rel_max(box[k], win[k]) < 3e-5, (k, rel_max(box[k], win[k]))
            assert not np.array_equal(box[k], win[k])                      # the other kernel did run
        assert rel_max(box["d_vox3"], win["d_vox3"]) < 3e-6                 # (fp32 atomics either way)


def test_matrix_core_adjoint_against_the_fp32_grade_backward():
    """... and against the bf16x3 backward (fp32 atomics, fp32-grade dX): the fp16 mode's stated L2 bound (tests/test_hip_backward.py)."""
    got = coarse_level_gradients("one_image", False)
    ref = coarse_level_gradients("one_image", False, precision="bf16x3")
    for k in ("d_vox4", "d_vox5"):
        err = float(np.linalg.norm((got[k] - ref[k]).ravel()) / np.linalg.norm(ref[k].ravel()))
        assert err < 0.08, (k, err)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **coarse_level_gradients(sys.argv[2], bool(int(sys.argv[3])), precision=sys.argv[4]))
