"""hip.gemm_nt / hip.gemm_tn against the float64 product of exact-integer operands, bit for bit, on every branch of
launch_one (gemm_kernels.hip) that the EPI_F32 entry point reaches, at the K values on each side of its borders.

The operands come from tests/_exact_case.py, whose builder asserts -- on the host, before anything is launched -- that
every operand is stored without loss in the format under test and that no partial sum can reach 2^24 units.  fp32
accumulation is then exact in any order, so there is no tolerance: a missed or doubled K-tile, a wrong fragment mapping,
a dropped hi . lo term, a lost lo plane or a race each move an integer.

Kernel reached per row (launch_one's dispatch: K >= 512 -> ping-pong for single-plane operands, K >= 1024 -> the
16 x 16 x 32 shape for split operands, plain_loop, interleaved):

  bf16x3  -            K =   64,  128,  960        k_gemm_nt<3>
  bf16x3  -            K = 1024, 1088, 3648        k_gemm_nt16<3>
  bf16x3  interleaved  K = 64, 512, 576, 1088, 3648   k_gemm_nt_pp<EPI_F32, 0, true, 3>
  bf16    -            K =   64,  448              k_gemm_nt<1>
  bf16    -            K =  512,  576,  640, 3648  k_gemm_nt_pp<EPI_F32, 0, true>
  bf16    plain_loop   K =  512,  576, 3648        k_gemm_nt16<1>
  bf16    interleaved  K =   64,  576, 3648        k_gemm_nt_pp<EPI_F32, 0, true, 1>
  fp16    -            K =   64,  448              k_gemm_nt<1, EPI_F32, 1>
  fp16    -            K =  512,  576,  640, 3648  k_gemm_nt_pp<EPI_F32, 1, true>
  fp16    plain_loop   K =  512, 3648              k_gemm_nt16<1, EPI_F32, 1>
"""
import numpy as np
import pytest
import torch

import _exact_case as E

pytestmark = pytest.mark.gpu

# (precision, flags, K values): every K at (M, N) = (256, 256), the last one at (768, 512) as well
NT_BRANCHES = [
    ("bf16x3", "", (64, 128, 960)),
    ("bf16x3", "", (1024, 1088, 3648)),
    ("bf16x3", "interleaved", (64, 512, 576, 1088, 3648)),
    ("bf16", "", (64, 448)),
    ("bf16", "", (512, 576, 640, 3648)),
    ("bf16", "plain_loop", (512, 576, 3648)),
    ("bf16", "interleaved", (64, 576, 3648)),
    ("fp16", "", (64, 448)),
    ("fp16", "", (512, 576, 640, 3648)),
    ("fp16", "plain_loop", (512, 3648)),
]
NT_CASES = [(p, f, K, 256, 256) for p, f, Ks in NT_BRANCHES for K in Ks] + \
           [(p, f, Ks[-1], 768, 512) for p, f, Ks in NT_BRANCHES]

# (P, M, N).  wgrad_splits(M, N, P, terms) = min(128, 512 / tiles, K-steps) with tiles = M / 256 * ceil(N / 256) and
# P / 64 K-steps (single-plane formats) or P / 32 (split):
#   (256, 256, 8)       4 / 8 splits of one step, N below the 16-column fragment
#   (512, 256, 264)     8 / 16 splits, a ragged second column tile
#   (4096, 256, 512)    64 / 128 splits of one step
#   (1024, 512, 3648)   17 nominal: 16 splits of one step / 17 of two steps, the last one empty
#   (1792, 768, 3648)   11 splits (512 / 45): 28 steps -> 3 per split, nine full and a last one of ONE step, one empty;
#                       split formats 56 steps -> 6 per split, nine full and a last one of TWO steps, one empty
TN_SHAPES = [(256, 256, 8), (512, 256, 264), (4096, 256, 512), (1024, 512, 3648), (1792, 768, 3648)]


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date
    from list_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def classes_for(precision):
    return [cls for cls, precs in E.GEMM_CLASSES.items() if precision in precs]


def check(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32
    if not np.array_equal(got.astype(np.float64), want):
        pytest.fail(f"{what}: {E.first_mismatch(got, want)}")


@pytest.mark.parametrize("precision,flags,K,M,N", NT_CASES)
def test_gemm_nt_is_exact_on_every_branch(hip, precision, flags, K, M, N):
    kw = dict(precision=precision, plain_loop=flags == "plain_loop", interleaved=flags == "interleaved")
    for cls in classes_for(precision):
        g = E.gemm_case(cls, precision, M, N, K)          # asserts representability and the 2^24 bound
        a, w, b = dev(g["a"]), dev(g["w"]), dev(g["bias"])
        what = f"gemm_nt {precision} {flags or 'default'} class {cls} M={M} N={N} K={K}"
        check(hip.gemm_nt(a, w, None, relu=False, **kw), g["ref"], what + " plain")
        check(hip.gemm_nt(a, w, None, relu=True, **kw), np.maximum(g["ref"], 0), what + " relu")
        check(hip.gemm_nt(a, w, b, relu=False, **kw), g["ref_bias"], what + " bias")
        check(hip.gemm_nt(a, w, b, relu=True, **kw), np.maximum(g["ref_bias"], 0), what + " bias+relu")


@pytest.mark.parametrize("precision", E.PRECISIONS)
@pytest.mark.parametrize("P,M,N", TN_SHAPES)
def test_gemm_tn_is_exact(hip, P, M, N, precision):
    """out[M, N] = a[P, M]^T b[P, N]: k_gemm_tn<1, 1> (fp16), k_gemm_tn<1, 0> (bf16), k_gemm_tn16<3, 0> (bf16x3) and the
    split-K slab reduction k_wgrad_reduce."""
    for cls in classes_for(precision):
        g = E.gemm_case(cls, precision, M, N, P)          # A [M, P], W [N, P]: the contraction index is the row of a and b
        got = hip.gemm_tn(dev(g["a"].T), dev(g["w"].T), precision)
        check(got, g["ref"], f"gemm_tn {precision} class {cls} P={P} M={M} N={N}")
