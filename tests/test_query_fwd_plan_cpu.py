"""CPU: which launches a forward query makes and in which form -- plan_query_fwd (csrc/query_fwd_plan.h), the rule that
list_sdf_query_fwd, list_query_plan and list_gather_features_fwd execute.  Every form gives the right SDF, only slower, so
nothing else would notice a level or a call sliding onto another one.  The header is built by a host compiler with -I include
-I csrc alone (tests/csrc/query_fwd_plan_host.cpp, which documents the words of a call) and asked for the calls below; the
expected rows are literals:
  sort | l0 .. l5 | box_levels | 2-D gather | fc_0/K[/produced K-tiles][/gap at+tiles]/row vector's home | tail | pixel order
  ride          the scalar level is written by the plain+ride level's kernel;   tail   by k_gather_tail
  kept          the kept channels of the projected map alone;   kept+rowvec   ... and the projected ones into the row vector"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _query_plan as QP  # noqa: E402

F16 = "ride,plain+ride,plain,plain,box,box box=48"
F32 = "ride,plain+ride,plain,plain,near,near box=0"
BF = "prec=bf16x3 map16=0 vox16=0"              # fp32 maps throughout
HEAD = f"morton {F16} kept sampled/2688/gap1+15/lo fused pix=1"
TRAIN = "f16 gemm/3648/- two+h3"
CASES = {
    # name: (call, expected)
    "headline": ("img=proj", HEAD),
    "headline_no_fused_fc0": ("img=proj no_fused=1", f"morton+pixel {F16} kept+rowvec gemm/2688/gap1+15/lo fused pix=1"),
    "fp16_inf": ("", f"morton {F16} none fused/3648/produced16/- fused pix=1"),
    "fp16_inf_FUSED_FC0_x": ("fused=2", f"morton+pixel {F16} f16 fused/3648/produced0/- fused pix=1"),
    "fp16_inf_FUSED_FC0_0": ("fused=0", f"morton+pixel {F16} f16 gemm/3648/- fused pix=1"),
    "fp16_train": ("inf=0", f"morton+pixel {F16} {TRAIN} pix=1"),
    "bf16x3_inf_img_proj": (f"{BF} img=proj", f"morton+pixel {F32} kept+rowvec gemm/2688/gap2+30/behind_kept two pix=1"),
    "bf16_inf": ("prec=bf16 map16=0 vox16=0", f"morton {F32} none fused/3648/produced32/- two pix=1"),
    "bf16x3_inf": (BF, f"morton+pixel {F32} f32 gemm/3648/- two pix=1"),
    "bf16x3_inf_FUSED_FC0_3": (f"{BF} fused=3", f"morton {F32} none fused/3648/produced32/- two pix=1"),
    "percep_feat_train": ("inf=0 img=pfeat", f"morton {F16} copy gemm/3648/- two+h3 pix=0"),
    "percep_feat_train_bf16x3": (f"{BF} inf=0 img=pfeat", f"morton {F32} copy gemm/3648/- two+h3 pix=0"),
    "percep_proj_fp16_inf": ("img=pproj", f"morton+pixel {F16} projected gemm/2624/head fused pix=1"),
    "no_sort": ("img=proj no_sort=1", HEAD.replace("morton", "none").replace("pix=1", "pix=0")),
    "no_sort_train": ("inf=0 no_sort=1", f"none {F16} {TRAIN} pix=0"),
    "map_size_180_train": ("inf=0 ms=180", f"morton+pixel {F16} {TRAIN} pix=1"),
    "map_size_181_train": ("inf=0 ms=181", f"morton {F16} {TRAIN} pix=0"),
    "map_size_181_percep_feat": ("inf=0 ms=181 img=pfeat", f"morton {F16} copy gemm/3648/- two+h3 pix=0"),
    "GATHER_BOX_0": ("img=proj box=0", HEAD.replace(F16, F32)),
    "TAIL_RIDE_0": ("img=proj ride=0", HEAD.replace(F16, "tail,plain,plain,plain,box,box box=48")),
    "R32": ("img=proj R=32", HEAD.replace(F16, "ride,plain+ride,near,near,box,box box=48")),
    "R32_fp32_maps": (f"{BF} R=32", f"morton+pixel ride,plain+ride,near,near,near,near box=0 f32 gemm/3648/- two pix=1"),
    "two_scalar_levels": ("img=proj l1.C=1", f"morton tail,tail,plain,plain,box,box box=48 kept sampled/2560/gap1+15/lo fused pix=1"),
    "H1_768_img_proj": ("img=proj H1=768", f"morton+pixel {F16} kept+rowvec gemm/2688/gap1+15/lo fused pix=1"),
    "H1_768": ("H1=768", f"morton+pixel {F16} f16 gemm/3648/- fused pix=1"),
    "H2_512": ("img=proj H2=512", HEAD.replace("lo fused", "lo two")),
    "no_kept_level": ("img=proj kept=0", f"morton {F16} none sampled/2624/gap0+16/lo fused pix=1"),
    "gather_only": ("gather_only=1", f"none {F16} f16 - - pix=1"),
    "gather_only_fp32_maps": (f"{BF} gather_only=1 inf=0", f"none {F32} f32 - - pix=1"),
    "gather_only_percep_feat": ("gather_only=1 img=pfeat", f"none {F16} copy - - pix=0"),
}


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    exe = QP.build_host(tmp_path_factory.mktemp("query_plan"))
    return QP.plans(exe, {name: call for name, (call, _) in CASES.items()})


@pytest.mark.parametrize("name", list(CASES))
def test_every_launch_takes_the_expected_form(got, name):
    print(name, got[name])
    assert got[name] == CASES[name][1]


def test_the_header_includes_only_the_c_abi_the_adjoint_plan_and_standard_headers():
    text = open(os.path.join(QP.CSRC, "query_fwd_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", '"list_hip.h"', '"vox_adjoint_plan.h"']
    assert "getenv" not in text
