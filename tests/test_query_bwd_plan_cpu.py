"""CPU: which form and which stream every stage of the query's backward takes behind the MLP chain -- plan_query_bwd
(csrc/query_bwd_plan.h), the rule that list_sdf_query_bwd and list_percep_pool_bwd execute.  Every form and every order gives
the same gradients, only slower (or, for the trans_mat gradient beside dW0, less reproducibly), so nothing else would notice
a stage sliding onto another stream.  The header is built by a host compiler with -I include -I csrc alone
(tests/csrc/query_bwd_plan_host.cpp, which documents the words of a call and of an answer), once more as a stand-alone
program under AddressSanitizer + UBSan, and asked for the calls below; the expected rows are literals.  Where nothing else is
said: B = 2, N = 300, map_size = 137, img_C = 1024, fp16, sort on, three auxiliary streams, every gradient asked with the
encoder levels, an fp32 map.
  streams=      the stream the main, direct, window and window2 lanes run on (window2 = main with two auxiliary streams)
  forks=        the hand-overs main -> window lane ahead of dW2 / dW1; /early: join window, dW0 on main, join direct, no fan-out
  main=         the 2-D stage on main behind the voxel levels; +pix: the 2-D adjoints walk the forward's pixel order
  event=1       dW0's event exists: recorded on the window lane behind dW0, waited for on the trans_mat gradient's lane"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _host_cxx import host_cxx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")

S3 = "streams=main,direct,window,window2 colsum=direct wgrad=window"
S2 = "streams=main,direct,window,main colsum=direct wgrad=window"
S0 = "streams=main,main,main,main colsum=main wgrad=main"
FORK3, FORK2, INLINE = f"{S3} forks=w2+w1 dw0=window", f"{S2} forks=w2+w1 dw0=window", f"{S0} forks=- dw0=main"
GATHER = "main=gather+heavy/f32+pix"
THREE = f"{FORK3} {GATHER} trans=behind_dw0@window2 event=1 resize=f32"
TWO = f"{FORK2} {GATHER} trans=behind_dw0@main event=1 resize=f32"       # on main: behind the resize and behind dW0's event
NONE = f"{INLINE} {GATHER} trans=inline@main event=0 resize=f32"         # directly behind the map gradient, ahead of the resize
ATOMIC = f"{FORK3} main=atomic/f32 trans=behind_dw0@window2 event=1 resize=f32"
# a half-precision map without the gather form or without fp16 operands: list_sdf_query_bwd refuses these calls before it
# plans (tests/test_hip_backward.py has the rejected calls); the plan names them so that a launcher never guesses
INVALID = f"{FORK3} main=invalid trans=behind_dw0@window2 event=1 resize=f16"
NO_WEIGHTS = "ask=b0,b1,b2,b3,map,levels,trans,vox"
CASES = {
    # name: (call, expected)
    "three_aux": ("", THREE),
    "two_aux": ("aux=2", TWO),
    "no_aux": ("aux=0", NONE),
    "three_aux_TRANS_UNORDERED": ("unordered=1", f"{FORK3} {GATHER} trans=inline@main event=0 resize=f32"),
    "two_aux_TRANS_UNORDERED": ("aux=2 unordered=1", f"{FORK2} {GATHER} trans=inline@main event=0 resize=f32"),
    "three_aux_no_trans": ("ask=mlp,map,levels,vox", f"{FORK3} {GATHER} trans=none event=0 resize=f32"),
    "only_trans_of_the_maps": ("ask=mlp,trans,vox", f"{FORK3} main=none+pix trans=behind_dw0@window2 event=1 resize=none"),
    "no_levels": ("ask=mlp,map,trans,vox", THREE.replace("resize=f32", "resize=none")),
    "no_sort": ("no_sort=1", ATOMIC),
    "map_size_180": ("ms=180", THREE),                  # 180 * 45 = 8100 <= 8192 < 181 * 46
    "map_size_181": ("ms=181", ATOMIC),
    "B64": ("B=64 N=5", THREE),
    "B65": ("B=65 N=5", ATOMIC),
    "B64_map_size_180": ("B=64 N=5 ms=180", THREE),     # 64 * 8100 <= 64 * 8192: the heavy groups are still planned
    "no_heavy_scratch": ("heavy=0", THREE.replace("+heavy", "")),
    "f16_map": ("map16=1", THREE.replace("/f32+pix", "/f16+pix").replace("resize=f32", "resize=f16")),
    "f16_map_bf16x3": ("map16=1 prec=bf16x3", INVALID.replace("invalid", "invalid+pix")),
    "f16_map_no_sort": ("map16=1 no_sort=1", INVALID),
    "f16_map_B65": ("map16=1 B=65 N=5", INVALID),
    "f16_map_map_size_181": ("map16=1 ms=181", INVALID),
    "percep_feat": ("pfeat=1 ask=mlp,pfeat,vox", f"{FORK3} main=rows_to_grad trans=none event=0 resize=none"),
    "percep_feat_no_grad": ("pfeat=1 ask=mlp,vox", f"{FORK3} main=none trans=none event=0 resize=none"),
    "percep_feat_only": ("pfeat=1 ask=mlp,pfeat", f"{FORK3} main=rows_to_grad trans=none event=0 resize=none"),
    "mlp_only": ("ask=mlp", f"{S3} forks=w2+w1 dw0=main/early main=none+pix trans=none event=0 resize=none"),
    "mlp_only_no_aux": ("ask=mlp aux=0", f"{S0} forks=- dw0=main/early main=none+pix trans=none event=0 resize=none"),
    "vox_only": ("ask=vox", f"{S3} forks=- dw0=window main=none+pix trans=none event=0 resize=none"),
    "no_w2": ("ask=w0,b0,w1,b1,b2,w3,b3,map,levels,trans,vox", THREE.replace("forks=w2+w1", "forks=w1")),
    "no_w1": ("ask=w0,b0,b1,w2,b2,w3,b3,map,levels,trans,vox", THREE.replace("forks=w2+w1", "forks=w2")),
    "no_weights": (NO_WEIGHTS, THREE.replace("forks=w2+w1", "forks=-")),
    "no_weights_no_aux": (f"{NO_WEIGHTS} aux=0", NONE),
    # nothing in the plan depends on the precision except the F16 map
    "bf16x3_three_aux": ("prec=bf16x3", THREE),
    "bf16x3_two_aux": ("prec=bf16x3 aux=2", TWO),
    "bf16x3_no_aux": ("prec=bf16x3 aux=0", NONE),
    "bf16_three_aux": ("prec=bf16", THREE),
    "bf16_two_aux": ("prec=bf16 aux=2", TWO),
    "bf16_no_aux": ("prec=bf16 aux=0", NONE),
    # list_percep_pool_bwd: a point set without orders on the main stream only, whatever else the call's words say
    "pool": ("pool=1 ask=map,trans aux=0 heavy=0", f"{INLINE} main=atomic/f32 trans=inline@main event=0 resize=none"),
    "pool_map_only": ("pool=1 ask=map aux=0 heavy=0", f"{INLINE} main=atomic/f32 trans=none event=0 resize=none"),
    "pool_trans_only": ("pool=1 ask=trans aux=3", f"{INLINE} main=none trans=inline@main event=0 resize=none"),
}


def build_host(directory, sanitize):
    exe = os.path.join(str(directory), "query_bwd_plan_host" + ("_san" if sanitize else ""))
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([host_cxx(), "-O1", "-std=c++17", "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "csrc", "query_bwd_plan_host.cpp"), "-o", exe], check=True)
    return exe


def plans(exe):
    text = "".join(f"{name} {call}\n" for name, (call, _) in CASES.items())
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
    return {line.split(" ", 1)[0]: line.split(" ", 1)[1] for line in out.splitlines()}


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    return plans(build_host(tmp_path_factory.mktemp("query_bwd_plan"), sanitize=False))


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_takes_the_expected_form_and_lane(got, name):
    print(name, got[name])
    assert got[name] == CASES[name][1]


def test_the_table_under_address_and_undefined_behaviour_sanitizers(tmp_path, got):
    """the same program, instrumented, run on its own (no preloading): it ends clean and answers the same"""
    assert plans(build_host(tmp_path, sanitize=True)) == got


def test_the_header_includes_only_the_c_abi_the_other_plans_and_standard_headers():
    text = open(os.path.join(CSRC, "query_bwd_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", '"list_hip.h"', '"query_fwd_plan.h"', '"vox_adjoint_plan.h"']
    assert "getenv" not in text and "hip/" not in text and "hipStream_t" not in text
