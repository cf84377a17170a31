"""GPU: the 2-D sample and its map gradient bit for bit against float64 on pixel-aligned projections
(tests/_exact_sample_case.py img_case; DESIGN.md "Exact-integer tests", "Grid-aligned samples").

The camera [[a,0,0],[0,a,0],[0,0,0],[h,h,1]] with a = 64 and h = (ms - 1) / 2 projects px = k / 128 onto the pixel coordinate
h + k / 2; the builder keeps the targets whose restated fp32 chain gives it exactly, so every bilinear weight is a multiple of
1/4, and the integer map [B, ms, ms, 1024] is handed over as a PreparedImage (no resize).  Forward: k_gather_img on fp16 and
fp32 maps, k_fc0_fused, the projected map of prep_percep_proj, percep_pool.  Backward: d_img_map through the pixel-order gather
(with more than 1024 points on one pixel: the heavy partials), through the atomic form and through percep_pool_backward.
d_trans_mat passes through divisions and is left to its tolerance tests; so is the half-precision map of want_img_map=False,
an intermediate no caller can read (only the resized levels behind it come out, through non-dyadic resize weights).
np.array_equal only.  Reference call sites: network/modules.py:37-53 (projection and grid_sample), :275-276 (concat, fc_0)."""
import numpy as np
import pytest
import torch

import _child_exact_sample as X
import _exact_case as E
import _exact_sample_case as S

pytestmark = pytest.mark.gpu

# name -> img_case(ms, B, N, clamp_hi, variant, pile)
CASES = {
    "ms50": (50, 2, 300, None, "plain", 0),                    # both clamps, ix = ms - 1
    "ms50_outside": (50, 2, 300, 136.0, "model", 0),           # the clamp beyond the map: taps and whole samples outside (zeros padding)
    "ms50_heavy": (50, 1, 2400, None, "model", 1500),          # 1500 points on pixel (0, 0): more than one chunk of heavy partials
    "ms137": (137, 1, 600, None, "plain", 0),                  # the model's map size
}
CONFIGS = (("fp16", "f16"), ("bf16x3", "f32"))


@pytest.fixture(scope="module")
def hip():
    return X.load_hip()


def prepared(hip, c, precision, map_dtype):
    data = X.dev(c["img_map"])
    if map_dtype == "f16":
        data = data.half()
    img = hip.PreparedImage(data.contiguous(), c["ms"], S.IMG_C, hip.MAP_DTYPES[map_dtype])
    vox = hip.prep_vox_maps([X.dev(m) for m in c["vox_maps"]], dtype=map_dtype)
    params = {k: X.dev(v) for k, v in c["weights"].items()}
    packed = hip.prep_mlp_weights(params, vox.channels, S.IMG_C, precision)
    return img, vox, packed, params


@pytest.mark.parametrize("name", list(CASES))
def test_sampled_features_and_sdf_are_exact(hip, name):
    c = S.img_case(*CASES[name])
    print(f"{name}: {c['yields'][0]} of {c['yields'][1]} half-pixel targets, heaviest pixel {c['flush_units']:.0f} units (limit 2^24)")
    q, T = X.dev(c["query"]), X.dev(c["trans_mat"])
    call = dict(perm=c["perm"], scale=c["scale"])
    bad = []
    for precision, md in CONFIGS:
        img, vox, packed, _ = prepared(hip, c, precision, md)
        what = f"{name} {precision}"
        Xf = hip.gather_features(q, T, img, vox, packed, **call) if c["clamp_hi"] == 136.0 else None     # (its clamp is the model's)
        if Xf is not None:
            got = Xf[:, E.VOX_COLS:E.VOX_COLS + S.IMG_C, :]
            bad.append(X.mismatch(got.reshape(-1, c["N"]), c["X_percep"].reshape(-1, c["N"]), f"gather_features {what} (row = b * 1024 + channel)"))
            assert not Xf[:, :E.VOX_COLS, :].any()                                         # zero voxel maps
        for fused in (True, False):
            for sort in (True, False):
                plan = {}
                sdf = hip.sdf_query(q, T, img, vox, packed, precision=precision, clamp_hi=c["clamp_hi"], fused_fc0=fused,
                                    sort_points=sort, plan=plan, **call)
                assert plan["fused_fc0"] == int(fused and precision == "fp16"), plan          # k_fc0_fused | k_gather_img + k_gemm_nt_pp
                bad.append(X.mismatch(sdf, c["sdf"], f"sdf {what} fused_fc0={fused} sort_points={sort}"))
        sdf, _ = hip.sdf_query(q, T, img, vox, packed, precision=precision, clamp_hi=c["clamp_hi"], save_for_backward=True, **call)
        bad.append(X.mismatch(sdf, c["sdf"], f"sdf {what} save_for_backward"))
        proj = hip.prep_percep_proj(img, packed, precision)
        sdf = hip.sdf_query(q, T, img, vox, packed, precision=precision, clamp_hi=c["clamp_hi"], percep_proj=proj, **call)
        bad.append(X.mismatch(sdf, c["sdf"], f"sdf {what} percep_proj"))
        # standalone pooling: the permuted and scaled points themselves
        pc = X.dev(S.restate_load_point(c["query"], c["perm"], c["scale"]))
        pooled = hip.percep_pool(pc, T, img, clamp_hi=c["clamp_hi"])
        assert tuple(pooled.shape) == (c["B"], S.IMG_C, 1, c["N"])
        bad.append(X.mismatch(pooled.reshape(-1, c["N"]), c["X_percep"].reshape(-1, c["N"]), f"percep_pool {what}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(CASES))
def test_map_gradient_is_exact(hip, name):
    c = S.img_case(*CASES[name])
    q, T, g = X.dev(c["query"]), X.dev(c["trans_mat"]), X.dev(c["grad_sdf"])
    call = dict(perm=c["perm"], scale=c["scale"])
    want = c["d_img_map"].reshape(-1, S.IMG_C)
    assert np.abs(want).max() > 0
    if c["pile"]:
        assert c["pile"] > 1024 and (c["m"][0, :c["pile"]] == 0).all()             # kHeavyChunk candidates and more in one group
    bad = []
    for precision, md in CONFIGS:
        img, vox, packed, params = prepared(hip, c, precision, md)
        packed_b = hip.prep_mlp_weights_bwd(params, vox.channels, S.IMG_C, precision)
        for sort, overlap in ((True, True), (True, False), (False, True)):      # pixel-order gather (k_img_grad_gather) | atomics (k_img_grad_atomic)
            sdf, ctx = hip.sdf_query(q, T, img, vox, packed, precision=precision, clamp_hi=c["clamp_hi"], save_for_backward=True,
                                     sort_points=sort, **call)
            out = hip.sdf_query_backward(ctx, g, packed_b, want_mlp=False, want_vox=False, want_trans=False, overlap=overlap)
            torch.cuda.synchronize()
            what = f"{name} {precision} sort_points={sort} overlap={overlap}"
            bad.append(X.mismatch(sdf, c["sdf"], f"sdf {what}"))
            bad.append(X.mismatch(out["img_map"].reshape(-1, S.IMG_C), want, f"d_img_map {what} (row = pixel, column = channel)"))
        pc = X.dev(S.restate_load_point(c["query"], c["perm"], c["scale"]))
        out = hip.percep_pool_backward(pc, T, img, X.dev(c["d_percep"].astype(np.float32)), want_trans=False, clamp_hi=c["clamp_hi"])
        bad.append(X.mismatch(out["img_map"].reshape(-1, S.IMG_C), want, f"percep_pool_backward {name} {precision}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)
