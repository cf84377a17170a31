"""GPU: the voxel gathers -- k_gather_vox, the TailRide pair, k_gather_vox_near, k_gather_vox_box, k_gather_tail -- bit for bit
against float64 on grid-aligned samples (tests/_exact_sample_case.py; DESIGN.md "Exact-integer tests", "Grid-aligned samples").

One stencil sample j* per run lies on half integers of every level of one size, so each of its trilinear weights is a
multiple of 1/8 and, on integer maps, every sum any kernel forms is exact: gather_features is compared on the aligned and the
perceptual columns, sdf_query -- whose fc_0 has zero weights on the six unaligned samples -- on every point, sorted and
unsorted, on fp16 and fp32 voxel maps.  np.array_equal only.  Reference call sites: network/modules.py:205-214 (stencil),
:256-265 (grid_sample over the pyramid)."""
import os
import subprocess
import sys

import pytest

import _child_exact_sample as X
import _query_plan as QP

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# pyramid -> the form of l0 .. l5 (tests/csrc/query_fwd_plan_host.cpp's words) with fp16 operands on fp16 maps | on fp32 maps
FORMS = {
    "p8": ("tail,near,near,near,box,box", "tail,near,near,near,near,near"),
    "p16": ("tail,near,near,near,box,box", "tail,near,near,near,near,near"),
    "p32": ("ride,plain+ride,plain,plain,plain,plain", "ride,plain+ride,plain,plain,plain,plain"),
    "c4": ("tail,plain,near,near,near,near", "tail,plain,near,near,near,near"),      # (column offsets 4 mod 8: no 16-byte pieces of X)
    "nc8": ("tail,near,near,near,box,box", "tail,near,near,near,near,near"),
    "nc": ("tail,near,near,near,box,box", "tail,near,near,near,near,near"),
}
RUNS = ([(p, j) for p in ("p8", "p16", "p32") for j in range(7)] +
        [("c4", 0), ("c4", 3), ("c4", 6), ("nc8", 0), ("nc8", 2), ("nc", 0), ("nc", 1), ("nc", 4), ("nc", 5)])


@pytest.fixture(scope="module")
def hip():
    return X.load_hip()


@pytest.fixture(scope="module")
def plan_host(tmp_path_factory):
    return QP.build_host(tmp_path_factory.mktemp("query_fwd_plan"))


def level_forms(line):
    return line.split()[1]


def test_the_cases_reach_every_form_of_the_voxel_gather(plan_host):
    asked, want = {}, {}
    for p, (f16, f32) in FORMS.items():
        c = X.case(p, 300, 0)
        for gather_only in (0, 1):
            asked[f"{p}_16_{gather_only}"], want[f"{p}_16_{gather_only}"] = X.fwd_plan_words(c, "fp16", True, gather_only=gather_only), f16
            asked[f"{p}_32_{gather_only}"], want[f"{p}_32_{gather_only}"] = X.fwd_plan_words(c, "fp16", False, gather_only=gather_only), f32
            asked[f"{p}_x3_{gather_only}"], want[f"{p}_x3_{gather_only}"] = X.fwd_plan_words(c, "bf16x3", False, gather_only=gather_only), f32
    got = QP.plans(plan_host, asked)
    for name in asked:
        assert level_forms(got[name]) == want[name], (name, got[name])
    reached = set(",".join(level_forms(v) for v in got.values()).split(","))
    # VG_SCALAR through k_gather_tail and riding, VG_PLAIN, VG_PLAIN_RIDE, VG_NEAR, VG_BOX
    assert reached == {"tail", "ride", "plain", "plain+ride", "near", "box"}, reached


@pytest.mark.parametrize("pyramid,j_star", RUNS)
def test_voxel_gathers_are_exact_on_aligned_samples(hip, pyramid, j_star):
    c = X.case(pyramid, 300, j_star)
    print(f"{pyramid} j*={j_star}: aligned levels {c['aligned']}, yields {c['yields']}, partial sums {c['units']:.0f} units")
    bad = []
    for precision, vox16 in X.GATHER_CONFIGS:
        forms = FORMS[pyramid][0 if vox16 else 1].split(",")
        box_levels = sum(1 << l for l, f in enumerate(forms) if f == "box")
        bad += X.check_gather(hip, c, precision, vox16, want_box_levels=box_levels)
    assert not bad, "\n".join(bad)


def _child(env_switch, specs):
    env = dict(os.environ, **{env_switch: "0"})
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_exact_sample.py"), "gather", *specs], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": done") == len(specs)


def test_near_kernel_in_place_of_the_matrix_core_gather_is_exact(plan_host):
    """LIST_GATHER_BOX=0 (read once per process): the 128-channel levels of the 8^3 and 16^3 pyramids through k_gather_vox_near."""
    got = QP.plans(plan_host, {p: X.fwd_plan_words(X.case(p, 300, 0), "fp16", True, box=0) for p in ("p8", "p16")})
    for p, line in got.items():
        assert level_forms(line) == "tail,near,near,near,near,near" and " box=0 " in line, (p, line)
    _child("LIST_GATHER_BOX", ["p8:300:1", "p8:300:4", "p16:300:0", "p16:300:6"])


def test_tail_kernel_in_place_of_the_riding_scalar_level_is_exact(plan_host):
    """LIST_TAIL_RIDE=0: the 32^3 pyramid's occupancy level through k_gather_tail, its 16-channel level through plain k_gather_vox."""
    got = QP.plans(plan_host, {"p32": X.fwd_plan_words(X.case("p32", 300, 0), "fp16", True, ride=0)})
    assert level_forms(got["p32"]) == "tail,plain,plain,plain,plain,plain", got
    _child("LIST_TAIL_RIDE", ["p32:300:0", "p32:300:2", "p32:300:5"])
