"""Inputs shared by test_objtext_cpu.py and test_objtext_gpu.py: the structured float32 bit patterns, the border face
indices, the oracle (the f-string of utils.write_obj, value by value) and the host program of tests/csrc/objtext_host.cpp."""
import os
import subprocess
from fractions import Fraction

import numpy as np

from _host_cxx import host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")
FLT_MAX = 0x7F7FFFFF
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def pow2_bits(k):
    """The bits of 2^k, -149 <= k <= 127."""
    return (k + 127) << 23 if k >= -126 else 1 << (k + 149)


def interval_end_class():
    """Positive float32 bit patterns whose widened float64 has a rounding interval that ENDS on a short decimal: with
    the 24-bit significand m and the float64 unit u = 2^(e - 52), the ends are (m * 2^30 -+ 1) * u / 2; for u / 2 =
    2^j, j >= k, an end is a multiple of 10^k iff 5^k divides m * 2^30 -+ 1, and with 10^k above the interval's width
    2^(j+1) no other multiple of 10^k lies inside.  The shortest digits are then the end itself, which only an interval
    with included ends offers (float32's 33995312 -> 33995310.0 is this class one size down)."""
    out = []
    for k in range(5, 11):
        p = 5 ** k
        for sign in (1, -1):                                   # m * 2^30 == sign (mod 5^k)
            m0 = (sign * pow(2 ** 30, -1, p)) % p
            for m in range(m0, 2 ** 24, p):
                if m < 2 ** 23:
                    continue
                for j in range(k, 40):                         # the ends are multiples of 2^j
                    if 2 ** (j + 1) >= 10 ** k:
                        break
                    # x = m * 2^29 float64 units of 2^(j+1), i.e. m * 2^(j+30): the float32 exponent field
                    expo = j + 30 + 23 + 127
                    if expo <= 254:
                        out.append((expo << 23) | (m & 0x7FFFFF))
    return np.array(sorted(set(out))[::13], dtype=np.uint32)      # every 13th of some 63 000: all exponents and both ends stay


def on_interval_end(bits):
    """Whether the text of the positive finite float32 `bits` is exactly an end of its float64 rounding interval (the
    midpoints to the float64 neighbours, as Fractions)."""
    x = float(np.uint32(bits).view(np.float32))
    v = Fraction(x)
    hi, lo = (v + Fraction(float(np.nextafter(x, np.inf)))) / 2, (v + Fraction(float(np.nextafter(x, -np.inf)))) / 2
    return Fraction(repr(x)) in (hi, lo)


def structured_bits():
    """The positive structured list: every power of two with its +-2 ulp neighbours, the float nearest every power of
    ten with +-1 ulp, the neighbours of 1e-4, 1e16 and 2^24 and of the layout's own borders (the float32 whose float64
    digits first reach e-05 and e+16), zero, infinity, NaNs, the subnormal extremes, FLT_MAX, and the interval-end class."""
    b = []
    for k in range(-149, 128):
        b += [pow2_bits(k) + d for d in (-2, -1, 0, 1, 2)]
    for k in range(-45, 39):
        b += [f32_bits(float(f"1e{k}")) + d for d in (-1, 0, 1)]
    for x in (1e-4, 1e16, 2.0 ** 24, 9.999999e15, 1.0001e-4):
        b += [f32_bits(x) + d for d in (-2, -1, 0, 1, 2)]
    b += [0, 1, 2, 0x7FFFFF, 0x800000, 0x800001, FLT_MAX, FLT_MAX - 1, 0x7F800000]
    b += [0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000, 0x7FC12345]
    b += [f32_bits(x) for x in (0.1, 0.5, 1.0, 1.5, 123456.79, 33995312.0, 0.00012345679, 1e-5, 3.4028235e38, 16777216.0)]
    pos = np.array([x for x in b if 0 <= x <= 0x7FFFFFFF], dtype=np.uint32)
    return np.unique(np.concatenate([pos, interval_end_class()]))


def signed(bits):
    """bits and the same with the sign bit set."""
    bits = np.asarray(bits, dtype=np.uint32)
    return np.concatenate([bits, bits | np.uint32(0x80000000)])


def random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def oracle_tokens(bits):
    """What utils.write_obj's f-string prints for each float32, value by value -> list of str."""
    return [f"{x}" for x in np.asarray(bits, dtype=np.uint32).view(np.float32)]


def as_vertices(bits):
    """uint32 [T] -> float32 [ceil(T/3), 3], padded with 1.0."""
    bits = np.asarray(bits, dtype=np.uint32)
    pad = (-len(bits)) % 3
    return np.concatenate([bits, np.full(pad, 0x3F800000, dtype=np.uint32)]).view(np.float32).reshape(-1, 3).copy()


def border_indices():
    """Face indices a with a + 1 at every decimal length border, the negative ones and the ends of int32 the Python loop
    can print (INT32_MAX alone overflows its int32 sum)."""
    idx = [0, -1, -2, -3, -10, -11, -12, INT32_MIN, INT32_MIN + 1, INT32_MAX - 1, INT32_MAX - 2]
    for k in range(1, 10):
        idx += [10 ** k - 2, 10 ** k - 1, 10 ** k]
    idx = [a for a in idx if INT32_MIN <= a < INT32_MAX]
    idx += [7] * ((-len(idx)) % 3)
    return np.array(idx, dtype=np.int32).reshape(-1, 3)


def sphere_mesh(n=32, r=0.3):
    """marching_cubes_cpu of a sphere of radius r in the [-0.5, 0.5]^3 box -> (verts float32 [V,3], faces int32 [F,3])."""
    from list_amd import mesh
    ax = np.linspace(-0.5, 0.5, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return mesh.marching_cubes_cpu((r - np.sqrt(x * x + y * y + z * z)).astype(np.float32), 0.0, -0.5, 0.5)


def loop_file(directory, verts, faces, name="loop.obj"):
    """The bytes of the file utils.write_obj writes."""
    from list_amd import utils
    path = os.path.join(str(directory), name)
    utils.write_obj(path, verts, faces)
    with open(path, "rb") as fh:
        return fh.read()


# ---- the header on the host -------------------------------------------------------------------------------------------
def build_host(directory):
    """Compiles tests/csrc/objtext_host.cpp with AddressSanitizer and UndefinedBehaviorSanitizer -> the program's path."""
    exe = os.path.join(str(directory), "objtext_host")
    subprocess.run([host_cxx(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "csrc", "objtext_host.cpp"),
                    "-o", exe], check=True)
    return exe


def run_host(exe, directory, verts, faces, cap):
    """objtext_host_file on the host with an output buffer of exactly `cap` bytes -> (the file's full length, the
    min(length, cap) bytes written)."""
    src, out = os.path.join(str(directory), "objtext_host.in"), os.path.join(str(directory), "objtext_host.out")
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    with open(src, "wb") as fh:
        fh.write(np.array([len(v), len(f), cap], dtype=np.int64).tobytes() + v.tobytes() + f.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    subprocess.run([exe, src, out], check=True, env=env)
    raw = open(out, "rb").read()
    total = int(np.frombuffer(raw[:8], dtype=np.int64)[0])
    assert len(raw) == 8 + min(total, cap)
    return total, raw[8:]
