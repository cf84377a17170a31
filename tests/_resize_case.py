"""Shared by test_resize_cpu.py and test_resize_gpu.py: pixel patterns, the ragged batch of every branch of the resize, and
the stand-alone host program over csrc/resize_math.h (tests/csrc/resize_host.cpp)."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")
PATTERNS = ("random", "zeros", "ones", "checker")


def pixels(pattern, H, W, seed=0):
    """uint8 [H,W,3]: random levels, all 0, all 255, or a 0 / 255 checkerboard."""
    if pattern == "random":
        return np.random.default_rng([seed, H, W]).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if pattern == "checker":
        y, x = np.mgrid[0:H, 0:W]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    return np.full((H, W, 3), {"zeros": 0, "ones": 255}[pattern], np.uint8)


def branch_sizes(out_h, out_w):
    """(H, W) of nine images that between them take every branch of H x W -> out_h x out_w (out_h < 300): 1 x 1, one side
    equal to the target (either), both equal (the copy), up-scaling with ksize 3, a plain reduction, a long filter
    (700 rows), and the tall-image rule on both sides of its border (303 > 100 * 3, 300 is not)."""
    return [(1, 1), (out_h, 29), (31, out_w), (out_h, out_w), (13, 13), (37, 53), (700, 3), (303, 3), (300, 3)]


def branch_batch(A, out_h, out_w, seed=0):
    """The nine images with mixed content (the 13 x 13 all 255, the 37 x 53 and the 300 x 3 checkerboards) and their records:
    some flipped, some jittered in several orders, some both, some plain."""
    sizes = branch_sizes(out_h, out_w)
    patterns = ["random", "random", "random", "random", "ones", "checker", "random", "random", "checker"]
    images = [pixels(p, h, w, seed) for p, (h, w) in zip(patterns, sizes)]
    records = [A.make_params(15, (3, 0, 2, 1), 0.7, 1.5, 127), A.make_params(A.FLIP), A.make_params(14, (2, 1, 0, 3), 1.3, 0.5, 255),
               A.make_params(15, (0, 3, 1, 2), 1.1, 0.9, 1), A.make_params(0), A.make_params(15, (1, 2, 3, 0), 0.8, 1.2, 200),
               A.make_params(A.FLIP | A.HUE, (0, 1, 2, 3), 1.0, 1.0, 64), A.make_params(A.FLIP), A.make_params(A.BRIGHTNESS, brightness=1.3)]
    return images, np.concatenate(records)


def build_host(directory):
    """Compiles csrc/resize_kernels.hip (as the library is built: no contraction) and tests/csrc/resize_host.cpp with the
    address and undefined-behaviour sanitizers on the host side alone (the device code is plain), and links them -> the program's
    path.  Nothing of it is loaded into python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    d = str(directory)
    host_sanitizers = ["-fsanitize=address,undefined", "-fno-gpu-sanitize"]      # the host side only: plain gfx950 device code
    flags = ["--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + host_sanitizers + [
        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    objs = []
    for src in (os.path.join(CSRC, "resize_kernels.hip"), os.path.join(ROOT, "tests", "csrc", "resize_host.cpp")):
        objs.append(os.path.join(d, os.path.basename(src) + ".o"))
        subprocess.run([hipcc] + flags + ["-c", src, "-o", objs[-1]], check=True)
    exe = os.path.join(d, "resize_host")
    subprocess.run([hipcc] + host_sanitizers + objs + ["-o", exe], check=True)
    return exe


def run_host(exe, image, out_h, out_w, directory):
    """The program on one uint8 [H,W,3] image -> (uint8 [out_h,out_w,3], the plan buffer of the one-image batch as
    list_resize_plan filled it, uint8)."""
    d = str(directory)
    src, dst, tab = (os.path.join(d, n) for n in ("resize_host.in", "resize_host.out", "resize_host.tab"))
    np.ascontiguousarray(image, dtype=np.uint8).tofile(src)
    H, W, _ = image.shape
    subprocess.run([exe, str(H), str(W), str(out_h), str(out_w), src, dst, tab], check=True, timeout=120)
    return np.fromfile(dst, np.uint8).reshape(out_h, out_w, 3), np.fromfile(tab, np.uint8)
