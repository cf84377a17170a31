"""No GPU: list_amd.stage, what the wrappers of the opt-in HIP stages (voxenc, imgenc, coarse) share -- the weight cache,
the refusals of forward(), the one statement of the eval-mode BN fold -- and the one validation of their model options."""
import os
import sys

import numpy as np
import pytest
import torch

from list_amd import arguments, coarse, imgenc, stage, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxenc_check as vc  # noqa: E402


# ---- pack_cached -----------------------------------------------------------------------------------------------------
class CountingPrep:
    def __init__(self):
        self.calls, self.fail = 0, False

    def __call__(self):
        self.calls += 1
        if self.fail:
            raise RuntimeError("prep failed")
        return object()


def _pack(m, prep):
    return stage.pack_cached(m, "_test_pack", list(m.parameters()) + list(m.buffers()), prep)


def test_pack_cached_returns_the_same_object_until_a_tensor_changes():
    m, prep = torch.nn.Linear(4, 3), CountingPrep()
    first = _pack(m, prep)
    assert _pack(m, prep) is first and prep.calls == 1
    with torch.no_grad():
        m.weight.add_(1.0)                                   # in place: the version counter moves
    second = _pack(m, prep)
    assert second is not first and prep.calls == 2
    assert _pack(m, prep) is second and prep.calls == 2
    m.bias = torch.nn.Parameter(m.bias.detach().clone())     # another tensor in the parameter's place
    third = _pack(m, prep)
    assert third is not second and prep.calls == 3
    assert _pack(m, prep) is third and prep.calls == 3
    m.double()
    fourth = _pack(m, prep)
    assert fourth is not third and prep.calls == 4
    assert _pack(m, prep) is fourth and prep.calls == 4
    assert m.__dict__["_test_pack"][2] is fourth


def test_pack_cached_leaves_no_entry_when_prep_raises():
    m, prep = torch.nn.Linear(4, 3), CountingPrep()
    _pack(m, prep)
    with torch.no_grad():
        m.weight.add_(1.0)
    prep.fail = True
    with pytest.raises(RuntimeError, match="prep failed"):
        _pack(m, prep)
    assert m.__dict__["_test_pack"] is None and prep.calls == 2
    with pytest.raises(RuntimeError, match="prep failed"):
        _pack(m, prep)
    assert prep.calls == 3                                    # ran again: nothing stale was served
    prep.fail = False
    got = _pack(m, prep)
    assert prep.calls == 4 and _pack(m, prep) is got and prep.calls == 4


# ---- the refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["vox_encoder", "img_encoder", "coarse_stage"])
def test_refuse_training_and_grad(flag):
    m, x = torch.nn.Linear(4, 3), torch.zeros(2, 4)
    m.train()
    with pytest.raises(RuntimeError, match="training mode") as e:
        stage.refuse_training_and_grad(flag, "encoder", [m], [x])
    assert f"{flag}='hip'" in str(e.value) and f"--{flag} torch" in str(e.value)
    with torch.no_grad(), pytest.raises(RuntimeError, match="training mode"):
        stage.refuse_training_and_grad(flag, "encoder", [torch.nn.Linear(2, 2).eval(), m], [x])
    m.eval()
    with pytest.raises(RuntimeError, match="no backward") as e:
        stage.refuse_training_and_grad(flag, "encoder", [m], [x, None])
    assert f"{flag}='hip'" in str(e.value) and f"--{flag} torch" in str(e.value)
    with torch.no_grad():
        stage.refuse_training_and_grad(flag, "encoder", [m], [x, None])
    m.requires_grad_(False)
    stage.refuse_training_and_grad(flag, "encoder", [m], [x])            # grad mode on, nothing requires a gradient
    with pytest.raises(RuntimeError, match="no backward"):
        stage.refuse_training_and_grad(flag, "encoder", [m], [None, x.clone().requires_grad_()])


def test_require_hip_module_names_the_caller():
    with pytest.raises(RuntimeError, match="HIP device") as e:
        stage.require_hip_module("voxenc.pack", torch.device("cpu"))
    assert "voxenc.pack" in str(e.value)
    stage.require_hip_module("voxenc.pack", torch.device("cuda", 0))


# ---- the BN fold -----------------------------------------------------------------------------------------------------
def _bn_arrays():
    rng = np.random.default_rng(5)
    n = 16
    g = rng.normal(1.0, 0.5, n).astype(np.float32)
    b = rng.normal(0.0, 0.5, n).astype(np.float32)
    m = rng.normal(0.0, 2.0, n).astype(np.float32)
    v = rng.uniform(0.01, 3.0, n).astype(np.float32)
    g[0], g[1] = 0.0, -1.25                                  # a zero and a negative weight
    v[2] = v[3] = 0.0                                        # with the tiny eps below: v + eps is denormal
    g[3] = -g[3]
    return g, b, m, v


@pytest.mark.parametrize("eps", [1e-5, 1e-3, 1e-40])
def test_bn_affine_is_the_fp32_formula_bit_for_bit(eps):
    g, b, m, v = _bn_arrays()
    f32 = np.float32
    if eps == 1e-40:
        assert 0 < f32(v[2] + f32(eps)) < np.finfo(f32).tiny          # a denormal
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = (g / np.sqrt((v + f32(eps)).astype(f32)).astype(f32)).astype(f32)
        t = (b - (m * s).astype(f32)).astype(f32)
        gs, gt = stage.bn_affine(g, b, m, v, eps)
    assert gs.dtype == f32 and gt.dtype == f32
    assert np.array_equal(gs.view(np.uint32), s.view(np.uint32)) and np.array_equal(gt.view(np.uint32), t.view(np.uint32))
    assert gs[0] == 0 and gt[0] == b[0] and gs[1] < 0
    # the float64 inputs of a state_dict read as float64 are rounded to fp32 first
    gs2, gt2 = stage.bn_affine(g.astype(np.float64), b.astype(np.float64), m.astype(np.float64), v.astype(np.float64), eps)
    assert np.array_equal(gs2.view(np.uint32), s.view(np.uint32)) and np.array_equal(gt2.view(np.uint32), t.view(np.uint32))


@pytest.mark.parametrize("eps", [1e-5, 1e-40])
def test_bn_affine_exact_is_float64(eps):
    g, b, m, v = _bn_arrays()
    f64 = np.float64
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = g.astype(f64) / np.sqrt(v.astype(f64) + eps)
        t = b.astype(f64) - m.astype(f64) * s
        gs, gt = stage.bn_affine(g, b, m, v, eps, exact=True)
    assert gs.dtype == f64 and gt.dtype == f64
    assert np.array_equal(gs.view(np.uint64), s.view(np.uint64)) and np.array_equal(gt.view(np.uint64), t.view(np.uint64))


@pytest.mark.parametrize("eps", [1e-5, 1e-40])
def test_the_stages_bn_affine_are_this_one(eps):
    g, b, m, v = _bn_arrays()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for exact in (False, True):
            s, t = stage.bn_affine(g, b, m, v, eps, exact)
            state = {"x.bn.weight": g, "x.bn.bias": b, "x.bn.running_mean": m, "x.bn.running_var": v}
            got = [imgenc.bn_affine(state, eps, "x.bn", exact),
                   coarse.bn_affine({"g": g, "b": b, "m": m, "v": v, "eps": eps}, exact)]
            if not exact:
                state = {"bn.4.weight": g, "bn.4.bias": b, "bn.4.running_mean": m, "bn.4.running_var": v}
                got.append(vc.bn_affine(state, eps, 4))
            for gs, gt in got:
                assert gs.dtype == s.dtype and gt.dtype == t.dtype
                assert gs.tobytes() == s.tobytes() and gt.tobytes() == t.tobytes()


# ---- sizes and options -----------------------------------------------------------------------------------------------
def test_align256():
    assert [stage.align256(n) for n in (0, 1, 255, 256, 257)] == [0, 256, 256, 256, 512]


@pytest.mark.parametrize("option", ["vox_encoder", "coarse_stage", "img_encoder"])
def test_models_refuse_a_bad_value_of_each_option_by_name(option):
    LIST = utils.get_class("network.models.LIST")
    with pytest.raises(ValueError, match=option) as e:
        LIST(arguments.default_config(vox_res=32, train_batch_size=2, **{option: "triton"}))
    assert "'triton'" in str(e.value) and "'torch' or 'hip'" in str(e.value)
    if option != "vox_encoder":
        with pytest.raises(ValueError, match=option):
            utils.get_class("network.models.CoarseNet")(
                arguments.default_config(vox_res=32, train_batch_size=2, **{option: "triton"}))
