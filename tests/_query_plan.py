"""The forward's launch rule (csrc/query_fwd_plan.h) asked on the host, through tests/csrc/query_fwd_plan_host.cpp."""
import os
import subprocess

from _host_cxx import host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")


def build_host(directory):
    """Compiles the host program with -I include -I csrc alone -> its path."""
    exe = os.path.join(str(directory), "query_fwd_plan_host")
    subprocess.run([host_cxx(), "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "csrc", "query_fwd_plan_host.cpp"), "-o", exe], check=True)
    return exe


def plans(exe, cases):
    """{name: "key=value ..."} -> {name: the host program's line for it, without the name}"""
    text = "".join(f"{name} {words}\n" for name, words in cases.items())
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
    return {line.split(" ", 1)[0]: line.split(" ", 1)[1] for line in out.splitlines()}
