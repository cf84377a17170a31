"""Shared by test_augment_cpu.py and test_augment_gpu.py: the stand-alone host program over csrc/augment_math.h
(tests/csrc/augment_host.cpp) and the image of every colour."""
import os
import subprocess

import numpy as np

from _host_cxx import host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")


def build_host(directory):
    """Compiles tests/csrc/augment_host.cpp for the host as the library is built (no contraction) -> the program's path."""
    exe = os.path.join(str(directory), "augment_host")
    subprocess.run([host_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(ROOT, "tests", "csrc", "augment_host.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_host(exe, step, value, directory, pixels=None):
    """One step of the header on `pixels` (uint8 [..., 3]; None: every colour, [4096, 4096, 3]) -> uint8 of that shape.
    `value` is the shift, or the factor as a float32."""
    out, args = os.path.join(str(directory), "augment_host.out"), []
    shape = (4096, 4096, 3)
    if pixels is not None:
        pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
        shape = pixels.shape
        args = [os.path.join(str(directory), "augment_host.in")]
        pixels.tofile(args[0])
    text = str(int(value)) if step == "hue" else repr(float(np.float32(value)))
    subprocess.run([exe, step, text, out] + args, check=True, timeout=120)
    return np.fromfile(out, np.uint8).reshape(shape)


def all_colours():
    """uint8 [4096, 4096, 3]: pixel i of the flattened image is (i >> 16, (i >> 8) & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([i >> 16, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
