"""GPU: every form of the voxel adjoint (csrc/bwd_scatter_kernels.hip, csrc/bwd_box_kernels.hip) bit for bit against float64
on grid-aligned samples (tests/_exact_sample_case.py; DESIGN.md "Exact-integer tests", "Grid-aligned samples").

dX is a small integer, every trilinear weight of the aligned sample a multiple of 1/8 and the dX of the six other samples
exactly 0 (fc_0 has zero weights there), so d_vox = sum w dX is a small multiple of 1/8 whatever adds it up: the scalar
kernel, fp32 atomics, packed-half atomics, the LDS windows with either flush, the matrix-core adjoint with packed flush (fp16)
or split operands (bf16x3), the voxel-side gather with 8 lanes or 1.  The builder bounds the per-voxel sum |w dX| below the
2^11 units a packed-half flush holds exactly.  The form of every level is asked of the rule itself (csrc/vox_adjoint_plan.h)
on the host.  np.array_equal only.  Reference call site: the autograd of network/modules.py:256-265."""
import os
import subprocess
import sys

import pytest

import _child_exact_sample as X
import _vox_plan as VP

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

MODES = (("auto", True), ("auto", False), ("scatter", False), ("gather", True))
# (pyramid, points per image, j*, pile): 600 points in every precision and mode; 4 096 of one image, where the packed-half forms
# have their scratch, in fp16 with the automatic choice
SMALL = [(p, 300, j, 0) for p in ("p8", "p16", "p32") for j in range(7)] + \
        [("c4", 300, j, 0) for j in (0, 3, 6)] + [("nc8", 300, 1, 0), ("nc", 300, 0, 0), ("nc", 300, 2, 0), ("nc", 300, 3, 0), ("nc", 300, 6, 0)]
LARGE = [(p, 4096, j, 0) for p in ("p8", "p16", "p32") for j in range(7)] + [("p8", 4096, 2, 701)]
NEEDED = {"scalar/direct/f32", "direct/direct/f32", "direct_h2/direct/h16", "gather8/gather/st", "gather1/gather/st",
          "win9/window/w0", "win9/window2/w1", "win9/window2/f32", "win18/window/w0", "win18/window2/f32",
          "box/window2/w1", "box/window2/f32"}
# what a few calls must choose for l0 .. l5 (the rest is printed, and the union is held to NEEDED)
PINNED = {
    ("p8", 4096, "fp16", "auto", False): "scalar/direct/f32 gather8/gather/st gather8/gather/st win9/window/w0 box/window2/w1 win9/window2/f32",
    ("p8", 4096, "fp16", "auto", True): "scalar/direct/f32 gather8/gather/st gather8/gather/st win9/window/w0 win9/window2/w1 win9/window2/f32",
    ("p16", 4096, "fp16", "auto", True): "scalar/direct/f32 gather8/gather/st gather8/gather/st win18/window/w0 box/window2/w1 win18/window2/f32",
    ("p32", 4096, "fp16", "auto", True): "scalar/direct/f32 direct/direct/f32 direct_h2/direct/h16 direct_h2/direct/h16 direct/direct/f32 direct/direct/f32",
    ("p16", 300, "bf16x3", "auto", True): "scalar/direct/f32 direct/direct/f32 direct/direct/f32 win18/window/f32 box/window2/f32 box/window2/f32",
    ("p8", 300, "bf16x3", "auto", False): "scalar/direct/f32 gather8/gather/st gather8/gather/st win9/window/f32 box/window2/f32 box/window2/f32",
    ("c4", 300, "fp16", "auto", True): "scalar/direct/f32 direct/direct/f32 gather1/gather/st win9/window/w0 win9/window2/f32 win9/window2/f32",
    ("p16", 300, "fp16", "gather", True): "scalar/direct/f32 gather8/gather/st gather8/gather/st gather8/gather/st gather8/gather/st gather8/gather/st",
}


@pytest.fixture(scope="module")
def hip():
    return X.load_hip()


@pytest.fixture(scope="module")
def plan_host(tmp_path_factory):
    return VP.build_host(tmp_path_factory.mktemp("vox_adjoint_plan"))


def calls_of(run):
    pyramid, n, j_star, pile = run
    for precision in (("fp16", "bf16x3") if n == 300 else ("fp16",)):
        for mode, overlap in (MODES if n == 300 else MODES[:2]):
            yield precision, mode, overlap


def test_the_cases_reach_every_form_of_the_voxel_adjoint(plan_host):
    asked, aligned = {}, {}
    for pyramid, n in sorted({(r[0], r[1]) for r in SMALL + LARGE}):      # (the rule does not read j*: one call per pyramid and size)
        c = X.case(pyramid, n, 0)
        aligned[(pyramid, n)] = c["aligned"]
        for precision, mode, overlap in calls_of((pyramid, n, 0, 0)):
            asked[f"{pyramid}|{n}|{precision}|{mode}|{int(overlap)}"] = X.adjoint_plan_case(VP, c, precision, mode, overlap)
    got = VP.plans(plan_host, asked)
    reached, pinned = set(), 0
    for name, levels in got.items():
        print(name, " ".join(levels))
        pyramid, n, precision, mode, overlap = name.split("|")
        reached |= {levels[l] for l in aligned[(pyramid, int(n))]}        # only a level that is compared counts
        assert "invalid" not in " ".join(levels) and "skip" not in levels
        want = PINNED.get((pyramid, int(n), precision, mode, bool(int(overlap))))
        if want:
            pinned += 1
            assert " ".join(levels) == want, name
    assert pinned == len(PINNED)
    assert NEEDED <= reached, NEEDED - reached


@pytest.mark.parametrize("pyramid,n,j_star,pile", SMALL + LARGE)
def test_voxel_adjoint_is_exact_on_aligned_samples(hip, pyramid, n, j_star, pile):
    c = X.case(pyramid, n, j_star, pile)
    print(f"{pyramid} n={n} j*={j_star}: aligned levels {c['aligned']}, grad_sdf density {c['density']:.2f}, "
          f"heaviest voxel {c['flush_units']:.0f} units of 1/8 (limit 2048)")
    bad = []
    for precision, mode, overlap in calls_of((pyramid, n, j_star, pile)):
        assert precision in c["precisions"]
        bad += X.check_adjoint(hip, c, precision, mode, overlap)
    assert not bad, "\n".join(bad)


def _child(env, specs):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_exact_sample.py"), "adjoint", *specs], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": done") == len(specs)


def _plans_of(plan_host, specs, **switch):
    asked = {}
    for spec in specs:
        f = spec.split(":")
        asked[spec] = X.adjoint_plan_case(VP, X.case(f[0], int(f[1]), int(f[2])), f[3], f[4], bool(int(f[5])), **switch)
    return VP.plans(plan_host, asked)


def test_lds_windows_in_place_of_the_matrix_core_adjoint_are_exact(plan_host):
    """LIST_SCATTER_BOX=0 (read once per process): the 128-channel window levels through k_scatter_vox_win, packed flush and fp32."""
    specs = ["p8:4096:1:fp16:auto:0", "p16:4096:3:fp16:auto:0", "p16:300:5:bf16x3:auto:0", "p8:300:2:bf16x3:auto:0"]
    got = _plans_of(plan_host, specs, box_mode=0)
    assert got[specs[0]][3:] == ["win9/window/w0", "win9/window2/w1", "win9/window2/f32"], got[specs[0]]
    assert got[specs[1]][3:] == ["win18/window/w0", "win18/window2/w1", "win18/window2/f32"], got[specs[1]]
    assert got[specs[2]][3:] == ["win18/window/f32"] + ["win18/window2/f32"] * 2 and got[specs[3]][3:] == ["win9/window/f32"] + ["win9/window2/f32"] * 2
    _child({"LIST_SCATTER_BOX": "0"}, specs)


def test_window_levels_flushing_fp32_atomics_are_exact(plan_host):
    """LIST_SCATTER_F32=1: both window kernels and the matrix-core adjoint add their fp32 sums straight into the gradient."""
    specs = ["p8:4096:6:fp16:auto:0", "p16:4096:0:fp16:auto:1", "p16:4096:4:fp16:auto:0"]
    got = _plans_of(plan_host, specs, f32=True)
    assert got[specs[0]][3:] == ["win9/window/f32", "box/window2/f32", "box/window2/f32"], got[specs[0]]
    assert got[specs[1]][3:] == ["win18/window/f32", "box/window2/f32", "box/window2/f32"], got[specs[1]]
    _child({"LIST_SCATTER_F32": "1"}, specs)
