"""The backward's voxel-adjoint rule (csrc/vox_adjoint_plan.h) asked on the host, through tests/csrc/vox_adjoint_plan_host.cpp:
shared by test_vox_adjoint_plan_cpu.py and test_box_adjoint_gpu.py."""
import os
import subprocess

from _host_cxx import host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")


def build_host(directory):
    """Compiles the host program with -I include -I csrc alone -> its path."""
    exe = os.path.join(str(directory), "vox_adjoint_plan_host")
    subprocess.run([host_cxx(), "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "csrc", "vox_adjoint_plan_host.cpp"), "-o", exe], check=True)
    return exe


def case(B, N, R=128, fp16=True, forked=True, mode=0, gather_buffers=True, box_mode=-1, f32=False, shift=0, edits=()):
    """One call of the rule.  mode: ListQueryGradArgs.vox_adjoint; box_mode, f32: LIST_SCATTER_BOX (-1: unset) and
    LIST_SCATTER_F32; shift: added to every level's column offset; edits: "lK.null", "lK.C=V", "lK.stride+V", "lK.dims=D,H,W", "lK.off=V"."""
    return [B, N, R, int(fp16), int(forked), mode, int(gather_buffers), box_mode, int(f32), shift, *edits]


def plans(exe, cases):
    """{name: case(...)} -> {name: ["form/lane/flush" or "skip" for l0 .. l5]}"""
    text = "".join(" ".join(str(x) for x in [name, *c]) + "\n" for name, c in cases.items())
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
    got = {name: [None] * 6 for name in cases}
    for line in out.splitlines():
        name, l, choice = line.split()
        got[name][int(l)] = choice
    return got
