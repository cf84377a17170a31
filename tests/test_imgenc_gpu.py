"""GPU: the HIP image encoder (list_amd.imgenc) launch by launch against a float64 evaluation of that one launch on the
device's own inputs (tests/_imgenc_check.py: every element within a derived bound), its levels and vector against the
numpy restatement, against the torch module (calibrated by the torch module under autocast fp16), and in the whole model."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fill, synth
from list_amd import arguments, imgenc, utils
from list_amd.network.modules import ResEncoder

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _imgenc_check as ic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 32, 48), (3, 64, 80), (2, 96, 96)]      # levels down to 2 x 3; partial tiles in W and a batch stride; full tiles


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def plain_encoder():
    return fill.fill_state(ResEncoder(), seed=3).eval()


def signed_encoder():
    """BN scales of both signs and zero: every third channel negated, every seventh zero, in every BN."""
    m = plain_encoder()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight[::3] *= -1.0
                mod.weight[5::7] = 0.0
    return m


def image(seed, B, H, W):
    return synth.uniform(seed, (B, 3, H, W)).astype(np.float32)


def _cl(t):
    """[B,C,h,w] view with channels-last strides -> numpy [B,h,w,C]."""
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def per_launch(module, img, what, poke=None):
    """Every launch alone (encode_steps) on what the launches before it left on the device, judged by ic.check on ITS OWN
    inputs read back from the device.  poke: {step name: fn(view)} applied to that launch's fp16 activation after it ran
    (and after it was judged), before the next launch reads it.  Returns the worst error / bound per launch."""
    params = imgenc.params_of(module)
    B, _, H, W = img.shape
    module.to(DEV)
    try:
        packed = imgenc.pack(module)
        Ls = ic.launches(params, head=tuple(t.cpu().numpy() for t in packed.head()))
        d_img = torch.from_numpy(img).to(DEV)
        buffers, worst = None, {}
        names = imgenc.step_names()
        assert len(Ls) == imgenc.n_steps()
        for k, L in enumerate(Ls):
            vec, levels, ws, buffers = imgenc.encode_steps(packed, d_img, k, k + 1, buffers)
            torch.cuda.synchronize()
            view = lambda i: _cl(imgenc.mid_view(ws, B, H, W, names[i]))
            s = L.step
            if L.kind == "stem":
                x = np.moveaxis(img, 1, 3)
            elif L.kind == "head":
                x = _cl(levels[4])
            else:
                x = view(s.src)
            idt = view(s.idt) if s.idt is not None else None
            act = vec.cpu().numpy() if L.kind == "head" else view(k)
            level = _cl(levels[s.level]) if s.level is not None else None
            q = ic.check(L, x, idt, act=act, level=level)
            worst[L.name] = q
            print(f"{what} {L.name:15s} max error / bound = {q:.3f}")
            if poke and L.name in poke:
                poke[L.name](imgenc.mid_view(ws, B, H, W, L.name))
        bad = {n: q for n, q in worst.items() if not q <= 1.0}
        assert not bad, (what, bad)
        return worst, (vec, levels, ws)
    finally:
        module.cpu()


@pytest.mark.parametrize("bn", ["plain", "signed"])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_launch_within_its_bound(shape, bn):
    m = plain_encoder() if bn == "plain" else signed_encoder()
    per_launch(m, image(11, *shape), f"{shape} {bn}")


def test_non_finite_values_propagate_and_are_compared_by_class():
    """A NaN pixel in image 0 and an infinity written into an fp16 activation of image 1 (through mid_view, between two
    launches); image 2 stays finite.  Every launch still meets its bound, with NaN and the infinities compared by class."""
    B, H, W = 3, 64, 80
    img = image(11, B, H, W)
    img[0, 1, 5, 7] = np.nan

    def inf_in(view):
        view[1, 3, 2, 2] = float("inf")
    _, (vec, levels, ws) = per_launch(signed_encoder(), img, "non-finite", poke={"layer1_0_conv1": inf_in})
    f0, f4 = levels[0].cpu().numpy(), levels[4].cpu().numpy()
    assert np.isnan(f0[0, :, 2:9, 4:11]).all() and np.isfinite(f0[0, :, 20:, 20:]).all()       # the 7 x 7 field of the pixel
    assert np.isnan(vec[0].cpu().numpy()).all()
    assert not np.isfinite(f4[1]).all()
    assert np.isfinite(f4[2]).all() and np.isfinite(vec[2].cpu().numpy()).all() and np.isfinite(f0[1:]).all()


def test_fp16_overflow_gives_infinity_not_saturation():
    """A BN scale that lifts layer3's output beyond 65504: the fp32 level keeps the value, its fp16 copy is an infinity (not
    65504), and layer4 sees it."""
    m = plain_encoder()
    with torch.no_grad():
        m.layer3[1].bn2.weight[:] = 2.0e6
    B, H, W = 1, 32, 48
    _, (vec, levels, ws) = per_launch(m, image(11, B, H, W), "overflow")
    f3 = levels[3].cpu().numpy()
    h3 = imgenc.mid_view(ws, B, H, W, "layer3_1_conv2").float().cpu().numpy()
    assert np.isfinite(f3).all() and f3.max() > 65520
    assert np.isinf(h3[f3 > 65520]).all() and np.isfinite(h3[f3 < 65000]).all()
    assert not np.isfinite(levels[4].cpu().numpy()).all()


def _vec_bound(module, ref):
    """What a level-4 difference of 2^-9 max|f4| does to vec through the mean and the composed matrix, per output."""
    wc, _ = imgenc.compose_head(imgenc.params_of(module)["state"])
    return 2.0 ** -9 * float(np.abs(ref["levels"][4]).max()) * np.abs(wc.astype(np.float64)).sum(axis=1)


# ---- the whole forward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 32, 48), (1, 224, 224)])
def test_levels_and_vec_match_the_restatement(shape):
    """The forward as one call against encode_cpu("device").  The restatement rounds each sum once and the device in
    its own order, so an fp16 activation may land on the neighbouring half and the difference travels on: the bound is
    2^-9 of the tensor's maximum (two fp16 ulps of the largest value, as for the 3-D encoder), and for vec what a
    level-4 difference of that size does through the mean and the composed matrix, 2^-9 max|f4| sum_k |W[n,k]|.  A
    second call gives identical bits (no atomics, fixed orders)."""
    B, H, W = shape
    m = plain_encoder()
    img = image(12, B, H, W)
    ref = imgenc.encode_cpu(imgenc.params_of(m), img, arithmetic="device", storage="fp16")
    m.to(DEV)
    packed = imgenc.pack(m)
    d_img = torch.from_numpy(img).to(DEV)
    vec, levels = imgenc.encode(packed, d_img)
    vec2, levels2 = imgenc.encode(packed, d_img)
    torch.cuda.synchronize()
    assert vec.shape == (B, 128) and vec.dtype == torch.float32
    for k, (a, b, c) in enumerate(zip(levels, ref["levels"], imgenc.LEVEL_CHANNELS)):
        assert a.dtype == torch.float32 and a.shape == (B, c, H >> k, W >> k) == b.shape
        assert a.stride(1) == 1 and a.is_contiguous(memory_format=torch.channels_last)
        err, top = float(np.abs(a.cpu().numpy() - b).max()), float(np.abs(b).max())
        print(f"{shape} f{k}: max|hip - restatement| = {err:.3e} (bound {2.0 ** -9 * top:.3e})")
        assert err <= 2.0 ** -9 * top, (k, err, top)
    bound = _vec_bound(m, ref)
    err = np.abs(vec.cpu().numpy().astype(np.float64) - ref["vec"])
    print(f"{shape} vec: max|hip - restatement| = {err.max():.3e} (bound from {bound.min():.3e})")
    assert (err <= bound).all()
    assert torch.equal(vec, vec2) and all(torch.equal(a, b) for a, b in zip(levels, levels2))
    # the composed head as the device holds it is the float64 composition rounded once (the last bit may differ where
    # the two float64 sums straddle a rounding boundary)
    dw, db = (t.cpu().numpy() for t in packed.head())
    wc64, bc64 = imgenc.compose_head(imgenc.params_of(m)["state"], np.float64)
    assert (np.abs(dw - wc64) <= 2.0 ** -24 * np.abs(wc64) * 1.0001 + 1e-45).all()
    assert (np.abs(db - bc64) <= 2.0 ** -24 * np.abs(bc64) * 1.0001 + 1e-45).all()


def test_channels_last_and_nchw_images_give_identical_bits():
    m = plain_encoder().to(DEV)
    packed = imgenc.pack(m)
    a = torch.from_numpy(image(13, 2, 64, 80)).to(DEV)
    b = a.contiguous(memory_format=torch.channels_last)
    assert a.stride() != b.stride() and torch.equal(a, b)
    va, la = imgenc.encode(packed, a)
    vb, lb = imgenc.encode(packed, b)
    torch.cuda.synchronize()
    assert torch.equal(va, vb) and all(torch.equal(x, y) for x, y in zip(la, lb))
    # ... and so does a batch taken apart: the order of every sum is fixed by the shapes alone
    v1, l1 = imgenc.encode(packed, a[1:2])
    assert torch.equal(v1, va[1:2]) and all(torch.equal(x, y[1:2]) for x, y in zip(l1, la))


def _rel(got, ref):
    return [float(np.abs(g.float().cpu().numpy() - r).max()) / float(np.abs(r).max()) for g, r in zip(got, ref)]


def test_error_against_fp32_is_within_twice_the_autocast_modules():
    """224^2, B = 2, fill_state weights.  e_hip: distance from the HIP encoder to the fp32 module on the CPU, per tensor,
    relative to max|tensor|; e_amp: the same for the torch module under autocast fp16 on the device.  The yardstick is the
    torch module, never the code under test; the condition e_hip <= 2 e_amp is the one the 3-D encoder uses."""
    m = plain_encoder()
    img = torch.from_numpy(image(14, 2, 224, 224))
    with torch.no_grad():
        vec, levels = m(img)
    ref = [vec.numpy()] + [v.numpy() for v in levels]
    m.to(DEV)
    d_img = img.to(DEV)
    with torch.no_grad():
        hv, hl = imgenc.forward(m, d_img)
        with torch.autocast("cuda", dtype=torch.float16):
            av, al = m(d_img)
    e_hip, e_amp = _rel([hv] + hl, ref), _rel([av] + al, ref)
    for name, a, b in zip(["vec", "f0", "f1", "f2", "f3", "f4"], e_hip, e_amp):
        print(f"224^2 B=2 {name}: e_hip = {a:.3e}, e_amp = {b:.3e}, ratio {a / b:.2f}")
    for name, a, b in zip(["vec", "f0", "f1", "f2", "f3", "f4"], e_hip, e_amp):
        assert a <= 2 * b, (name, a, b)


def test_pack_is_rebuilt_after_load_state_dict():
    a, other = plain_encoder().to(DEV), fill.fill_state(ResEncoder(), seed=5).eval()
    img = torch.from_numpy(image(15, 1, 32, 32)).to(DEV)
    p0 = imgenc.pack(a)
    assert imgenc.pack(a) is p0
    v0, _ = imgenc.encode(p0, img)
    a.load_state_dict(other.state_dict())
    p1 = imgenc.pack(a)
    assert p1 is not p0
    v1, _ = imgenc.encode(p1, img)
    ref = imgenc.encode_cpu(imgenc.params_of(other), img.cpu().numpy())
    assert not torch.equal(v0, v1) and (np.abs(v1.cpu().numpy() - ref["vec"]) <= _vec_bound(other, ref)).all()


def test_training_mode_raises_instead_of_falling_back():
    m = ResEncoder().to(DEV)
    img = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="training mode"):
        imgenc.forward(m, img)
    m.eval()
    with pytest.raises(RuntimeError, match="no backward"):
        imgenc.forward(m, img)
    with torch.no_grad():
        vec, levels = imgenc.forward(m, img)
    assert vec.shape == (1, 128) and len(levels) == 5


# ---- the whole model -------------------------------------------------------------------------------------------------
def _amp_encoders(net):
    """The two ResEncoders of `net` run under autocast fp16 (their outputs handed on as fp32, as the query path takes them)."""
    for enc in (net.im_encoder, net.im_encoder2):
        inner = enc.forward

        def fwd(x, inner=inner):
            with torch.autocast("cuda", dtype=torch.float16):
                v, f = inner(x)
            return v.float(), [t.float() for t in f]
        enc.forward = fwd


def test_whole_model_against_the_reference_golden(golden_dir):
    """LIST(img_encoder="hip") on the golden inputs, the other stages at their defaults: the SDF's distance to the reference's
    list_sdf, against that of the same model with its torch encoders under autocast fp16 -- the same condition as for the
    encoder alone, e_hip <= 2 e_amp; no absolute tolerance."""
    g = np.load(os.path.join(golden_dir, "models.npz"))
    LIST = utils.get_class("network.models.LIST")
    img = torch.from_numpy(synth.uniform(78, (2, 3, 64, 64))).to(DEV)
    q = torch.from_numpy(synth.make_query(79, 2, 100)).to(DEV)
    top = float(np.abs(g["list_sdf"]).max())
    errs = {}
    for kind in ("hip", "amp", "torch"):
        cfg = arguments.default_config(vox_res=32, train_batch_size=2, img_encoder="hip" if kind == "hip" else "torch")
        net = fill.fill_state(LIST(cfg), seed=2).eval().to(DEV)
        if kind == "amp":
            _amp_encoders(net)
        with torch.no_grad():
            _, sdf = net(img, q)
        errs[kind] = float(np.abs(sdf.cpu().numpy() - g["list_sdf"]).max()) / top
    print(f"whole model, max|sdf - list_sdf| / max|list_sdf|: hip encoders {errs['hip']:.3e}, torch encoders under "
          f"autocast fp16 {errs['amp']:.3e}, torch encoders fp32 {errs['torch']:.3e}")
    assert errs["hip"] <= 2 * errs["amp"], errs


def test_test_py_with_every_hip_stage_writes_meshes(tmp_path):
    out = str(tmp_path / "out") + "/"
    cmd = [sys.executable, os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "test.py"),
           "--model", "network.models.LIST", "--dataset", "datasets.Datasets.SyntheticIM2SDF", "-e", "ie",
           "--output_dir", out, "--mcube_znum", "40", "--vox_res", "32", "--img_encoder", "hip", "--coarse_stage", "hip",
           "--vox_encoder", "hip", "--precision", "fp16", "--testlist_file", ""]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    objs = [f for f in os.listdir(os.path.join(out, "ie", "test_objs", "synthetic")) if f.endswith("_pred.obj")]
    assert len(objs) == 2
