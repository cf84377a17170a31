"""The host C++ compiler of the tests that build a header-only rule of csrc/ into a small host program (tests/csrc/)."""
import os
import shutil


def host_cxx():
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler found (c++, g++, clang++ or ROCm's clang++)"
    return cxx
