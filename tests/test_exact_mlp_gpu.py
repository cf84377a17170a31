"""The SDF query's MLP chain -- forward and backward, every precision -- against the integer reference of
tests/_exact_case.py, bit for bit.

Every operand of every launch (X, H1..H3, dZ3..dZ1, dX, the weights) is an integer multiple of one power of two that the
format under test stores without loss, and no partial sum can reach 2^24 units: the builder asserts both on the host.  So
the ReLU masks are unambiguous, fp32 accumulation is exact in any order, and fp16, bf16x3 and bf16 must all return the
same numbers as the float64 reference -- hi / lo split stores, the fused fc_2 + fc_out reduction, k_mlp_tail_f16, the
masked data gradients, the split-K weight gradients with their padded rows, the column map of d fc_0.weight and the
fp16 gradient scale included.  No tolerance anywhere.
"""
import numpy as np
import pytest
import torch

import _exact_case as E

pytestmark = pytest.mark.gpu

PERM, SCALE = (0, 1, 2), 1.0
FORWARD_CASES = [("narrow", 512, "fp16"), ("narrow", 512, "bf16x3"), ("narrow", 512, "bf16"),
                 ("wide", 512, "fp16"), ("wide", 512, "bf16x3"),
                 ("narrow", 768, "fp16"), ("narrow", 768, "bf16x3"), ("narrow", 768, "bf16")]
BACKWARD_CASES = [c for c in FORWARD_CASES if c[1] == 512]


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


def prepare(hip, c, precision):
    md = hip.map_dtype_for(precision)
    vox = hip.prep_vox_maps([dev(m) for m in c["vox_maps"]], dtype=md)
    params = {k: dev(v) for k, v in c["weights"].items()}
    packed = hip.prep_mlp_weights(params, vox.channels, E.IMG_C, precision)
    return vox, packed, params


def same(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want, np.float64).reshape(got.shape)
    if not np.array_equal(got.astype(np.float64), want):
        pytest.fail(f"{what}: {E.first_mismatch(got.reshape(got.shape[0], -1), want.reshape(got.shape[0], -1))}")


# ------------------------------------------------------------------------------------------ the gathers come first
@pytest.mark.parametrize("variant,precision", [("narrow", "fp16"), ("narrow", "bf16x3"), ("wide", "fp16"), ("wide", "bf16x3")])
def test_gathered_features_are_the_integer_X(hip, variant, precision):
    """Zero levels give zeros, the 1 x 1 x 1 level gives its channel with weight 1 to all seven stencil samples, the
    pre-pooled perceptual features and the coordinates are copied: X is exact before any GEMM runs."""
    c = E.mlp_case(variant)
    vox, packed, _ = prepare(hip, c, precision)
    X = hip.gather_features(dev(c["query"]), None, None, vox, packed, perm=PERM, scale=SCALE, percep_feat=dev(c["percep_feat"]))
    assert tuple(X.shape) == (E.B, E.F, E.N)
    same(X.reshape(E.B * E.F, E.N), c["X"].reshape(E.B * E.F, E.N), f"gather_features {variant} {precision} (row = b * F + column)")


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("variant,H1,precision", FORWARD_CASES)
def test_forward_is_exact(hip, monkeypatch, variant, H1, precision):
    c = E.mlp_case(variant, H1)
    assert precision in c["precisions"]
    vox, packed, _ = prepare(hip, c, precision)
    q, pf = dev(c["query"]), dev(c["percep_feat"])
    what = f"sdf {variant} H1={H1} {precision}"

    def run(query=q, **kw):
        return hip.sdf_query(query, None, None, vox, packed, perm=PERM, scale=SCALE, precision=precision, percep_feat=pf, **kw)

    for sort in (True, False):
        plan = {}
        same(run(sort_points=sort, plan=plan), c["sdf"], f"{what} sort_points={sort}")
        # fp16 inference forwards take k_mlp_tail_f16 (fc_1 + fc_2 + fc_out in one launch), the rest k_gemm_nt* twice
        assert plan["fused_tail"] == (1 if precision == "fp16" else 0) and plan["chunks"] == 1
    if precision == "fp16":
        monkeypatch.setenv("LIST_FUSED_TAIL", "0")
        plan = {}
        same(run(plan=plan), c["sdf"], f"{what} LIST_FUSED_TAIL=0")
        assert plan["fused_tail"] == 0
        monkeypatch.setenv("LIST_FUSED_TAIL", "1")
        same(run(), c["sdf"], f"{what} LIST_FUSED_TAIL=1")
        monkeypatch.delenv("LIST_FUSED_TAIL")
    sdf, ctx = run(save_for_backward=True)
    same(sdf, c["sdf"], f"{what} save_for_backward")
    assert ctx is not None
    # a strided view: every second point, three of four columns
    base = torch.full((E.B, 2 * E.N, 4), 0.25, dtype=torch.float32, device="cuda:0")
    view = base[:, ::2, :3]
    view.copy_(q)
    assert not view.is_contiguous()
    same(run(query=view), c["sdf"], f"{what} strided query")


# ------------------------------------------------------------------------------------------ backward
def backward(hip, c, precision, **want):
    vox, packed, params = prepare(hip, c, precision)
    packed_b = hip.prep_mlp_weights_bwd(params, vox.channels, E.IMG_C, precision)
    sdf, ctx = hip.sdf_query(dev(c["query"]), None, None, vox, packed, perm=PERM, scale=SCALE, precision=precision,
                             percep_feat=dev(c["percep_feat"]), save_for_backward=True)
    out = hip.sdf_query_backward(ctx, dev(c["grad_sdf"]), packed_b, **want)
    torch.cuda.synchronize()
    return sdf, out


@pytest.mark.parametrize("variant,H1,precision", BACKWARD_CASES)
def test_backward_is_exact(hip, variant, H1, precision):
    c = E.mlp_case(variant, H1)
    r = c["ref"]
    what = f"{variant} {precision}"
    for label, want in (("default", dict(want_vox=False)), ("overlap=False", dict(want_vox=False, overlap=False)),
                        ("want_vox=True", dict(want_vox=True)),
                        ("mlp only (early-return dW0)", dict(want_img=False, want_vox=False))):
        sdf, out = backward(hip, c, precision, **want)
        same(sdf, c["sdf"], f"sdf {what} {label}")
        assert set(out["mlp"]) == {k[2:] for k in E.MLP_GRAD_KEYS}
        for k in E.MLP_GRAD_KEYS:                         # d fc_0.weight over all 3610 columns: zero-X columns exactly 0
            same(out["mlp"][k[2:]], r[k], f"{k} {what} {label}")
        dw0 = out["mlp"]["fc_0.weight"].cpu().numpy()
        assert dw0.shape == (H1, E.F, 1) and not dw0[:, :E.LAST_LEVEL_COL].any()
        if want.get("want_img", True):
            same(out["percep_feat"].reshape(E.B * E.IMG_C, E.N), c["d_percep_feat"].reshape(E.B * E.IMG_C, E.N),
                 f"d percep_feat {what} {label} (row = b * 1024 + channel)")
        else:
            assert "percep_feat" not in out
        assert ("vox" in out) == bool(want.get("want_vox"))


# ------------------------------------------------------------------------------------------ the image paths on zero maps
@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
def test_zero_map_image_paths_are_exact(hip, precision):
    """All image and voxel maps zero: only xyz and the biases drive the chain, through every way fc_0 can take its
    perceptual block -- sampled into X (unfused), produced inside k_fc0_fused, sampled from the projected map
    (percep_proj), and the projected low-resolution levels of prep_img_proj."""
    c = E.mlp_case("zero_maps")
    vox, packed, _ = prepare(hip, c, precision)
    md = hip.map_dtype_for(precision)
    maps = [dev(m) for m in c["img_maps"]]
    img = hip.prep_img_maps(maps, dtype=md)
    q, T = dev(c["query"]), dev(c["trans_mat"])
    what = f"sdf zero maps {precision}"

    def run(image, **kw):
        return hip.sdf_query(q, T, image, vox, packed, perm=PERM, scale=SCALE, precision=precision, **kw)

    for fused in (True, False):
        for sort in (True, False):
            same(run(img, fused_fc0=fused, sort_points=sort), c["sdf"], f"{what} fused_fc0={fused} sort_points={sort}")
    sdf, _ = run(img, save_for_backward=True)
    same(sdf, c["sdf"], f"{what} save_for_backward")
    proj = hip.prep_percep_proj(img, packed, precision)
    same(run(img, percep_proj=proj), c["sdf"], f"{what} percep_proj")
    imgp = hip.prep_img_proj(maps, packed, 137, precision)
    for fused in (True, False):
        plan = {}
        same(run(imgp, fused_fc0=fused, plan=plan), c["sdf"], f"{what} prep_img_proj fused_fc0={fused}")
        assert plan["img_proj"] == 1
