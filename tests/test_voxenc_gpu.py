"""GPU: the HIP occupancy encoder (list_amd.voxenc, include/list_voxenc.h) against its numpy restatement, against the
reference's arithmetic (calibrated by the existing autocast-fp16 encoder), end to end against the reference's golden
SDF, and its plumbing through LIST.encode, predict_grid and test.py.

Bound of the kernel checks (levels 1 .. 5): max|hip - restatement| <= 2^-9 max|level|.  Device and restatement round
the same fp32 values to fp16 and differ only by the MFMA's accumulation order; that can flip a final rounding by one
fp16 ulp (<= 2^-10 of the magnitude), earlier flips arrive attenuated (one input among 27 C_in): two ulps of the
largest binade.  Level 0 is fp32 throughout: 1e-5, the project's bound for this level."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fill, synth
from list_amd import arguments, utils, voxenc
from list_amd.network.modules import VoxelEncoder2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [1, 1, 1, 1, 16, 32, 64, 128, 128]
HALF_BOUND = 2.0 ** -9


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


@pytest.fixture(scope="module")
def enc():
    return fill.fill_state(VoxelEncoder2(LAYERS), seed=2).eval()


def make_occ(kind, B, R):
    if kind == "zero":
        return np.zeros((B, R, R, R), dtype=np.float32)
    if kind == "random":
        return (np.random.default_rng(11).random((B, R, R, R)) < 0.03).astype(np.float32)
    occ = np.zeros((B, R, R, R), dtype=np.float32)          # "faces": ones on all six faces
    occ[:, 0, 3:9, 5:7] = 1
    occ[:, R - 1, 10:12, 1:20] = 1
    occ[:, 4:6, 0, 2:9] = 1
    occ[:, 20:23, R - 1, 7] = 1
    occ[:, 7, 7:19, 0] = 1
    occ[:, 9:30, 9, R - 1] = 1
    occ[:, 0, 0, 0] = occ[:, R - 1, R - 1, R - 1] = 1
    return occ


def point_occ(seed, B, R, n=2048):
    """Occupancy of n random points per image, as LIST.create_occ voxelises a coarse cloud."""
    occ = np.zeros((B, R ** 3), dtype=np.float32)
    rng = np.random.default_rng(seed)
    for b in range(B):
        c = np.clip(rng.normal(0.5, 0.15, size=(n, 3)), 0, 1)
        ijk = np.floor(c * (R - 1) + 0.5).astype(np.int64)
        occ[b, (ijk[:, 0] * R + ijk[:, 1]) * R + ijk[:, 2]] = 1
    return occ.reshape(B, R, R, R)


def check_levels(got, ref, what, first=0):
    for k in range(first, 6):
        if ref[k] is None:
            continue
        a, b = got[k].float().cpu().numpy(), ref[k].astype(np.float32)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        err, top = float(np.abs(a - b).max()), float(np.abs(b).max())
        bound = 1e-5 if k == 0 else HALF_BOUND * top
        print(f"{what}: level {k}: max|hip - restatement| = {err:.3e} (bound {bound:.3e}, max|level| {top:.3e})")
        assert np.isfinite(a).all() and err <= bound, (what, k, err, bound)


@pytest.mark.parametrize("B,R", [(2, 32), (1, 64)])
@pytest.mark.parametrize("kind", ["random", "faces", "zero"])
def test_kernels_match_the_restatement(enc, B, R, kind):
    occ = make_occ(kind, B, R)
    ref = voxenc.encode_cpu(occ, voxenc.params_of(enc), storage="fp16")
    enc.to(DEV)
    try:
        packed = voxenc.pack(enc)
        d_occ = torch.from_numpy(occ).to(DEV)
        levels, ws = voxenc.encode(d_occ, packed, return_workspace=True)
        again = voxenc.encode(d_occ, packed)
        torch.cuda.synchronize()
        assert levels[0].dtype == torch.float32 and levels[0].shape == (B, 1, R, R, R)
        for k in range(1, 6):
            D = R >> (k - 1)
            assert levels[k].dtype == torch.float16 and levels[k].shape == (B, LAYERS[k + 3], D, D, D)
            assert levels[k].stride(1) == 1 and levels[k].is_contiguous(memory_format=torch.channels_last_3d)
        check_levels(levels, ref, f"B={B} R={R} {kind}")
        for a, b in zip(levels, again):                     # no atomics: the same bits
            assert torch.equal(a, b)
        for stage in range(3, 7):                           # the fused pool is max_pool3d of the level, exactly
            pooled = voxenc.pooled_view(ws, B, R, LAYERS, stage)
            want = torch.nn.functional.max_pool3d(levels[stage - 2].float(), 2)
            assert torch.equal(pooled.float(), want), stage
        assert ws.numel() == voxenc.workspace_bytes(B, R, LAYERS)
    finally:
        enc.cpu()


def _relative_errors(net_cpu, occ):
    """(e_hip, e_amp): worst level error, relative to the level's maximum, of the HIP encoder and of the existing
    autocast-fp16 encoder against the fp32 torch module on the CPU."""
    with torch.no_grad():
        ref = [v.numpy() for v in net_cpu.vox_encoder(occ)]
    net_cpu.to(DEV)
    try:
        d_occ = occ.to(DEV)
        with torch.no_grad():
            hip_levels = voxenc.forward(net_cpu.vox_encoder, d_occ)
            net_cpu.vox_encoder.to(memory_format=torch.channels_last_3d)
            with torch.autocast("cuda", dtype=torch.float16):
                amp_levels = net_cpu.vox_encoder(d_occ)
        worst = lambda ls: max(float(np.abs(v.float().cpu().numpy() - r).max()) / float(np.abs(r).max())
                               for v, r in zip(ls, ref))
        return worst(hip_levels), worst(amp_levels)
    finally:
        net_cpu.cpu()


def test_error_against_fp32_is_within_twice_the_autocast_encoders():
    """The yardstick is the project's existing half-precision encoder (vox_encoder_precision="fp16") against the fp32
    torch module, never the code under test; factor 2: autocast keeps BN and the sigmoid in fp32 and rounds fewer
    intermediates than a pipeline that stores every activation in fp16."""
    cfg = arguments.default_config(vox_res=32, train_batch_size=2, vox_encoder_precision="fp16")
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval()
    with torch.no_grad():
        occ = net.encode(torch.from_numpy(synth.uniform(78, (2, 3, 64, 64))))[4]
    e_hip, e_amp = _relative_errors(net, occ)
    print(f"R=32 B=2: e_hip = {e_hip:.3e}, e_amp = {e_amp:.3e}, ratio {e_hip / e_amp:.2f}")
    assert e_hip <= 2 * e_amp, (e_hip, e_amp)
    cfg = arguments.default_config(vox_res=128, train_batch_size=1, vox_encoder_precision="fp16")
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval()
    e_hip, e_amp = _relative_errors(net, torch.from_numpy(point_occ(3, 1, 128)))
    print(f"R=128 B=1: e_hip = {e_hip:.3e}, e_amp = {e_amp:.3e}, ratio {e_hip / e_amp:.2f}")
    assert e_hip <= 2 * e_amp, (e_hip, e_amp)


def test_end_to_end_against_the_reference_golden(golden_dir):
    from list_amd import hip
    g = np.load(os.path.join(golden_dir, "models.npz"))
    cfg = arguments.default_config(vox_res=32, train_batch_size=2, vox_encoder="hip", precision="fp16")
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(DEV)
    img = torch.from_numpy(synth.uniform(78, (2, 3, 64, 64))).to(DEV)
    q = torch.from_numpy(synth.make_query(79, 2, 100)).to(DEV)
    with torch.no_grad():
        vox0, sdf = net(img, q)
        feat_l2, vox_feat, tm, _, _ = net.encode(img)
        vox = hip.prep_vox_maps(vox_feat, "f16")
    top = max(1.0, float(np.abs(g["list_sdf"]).max()))
    err = float(np.abs(sdf.cpu().numpy() - g["list_sdf"]).max())
    err0 = float(np.abs(vox0.cpu().numpy()[:, :, ::4, ::4, ::4] - g["list_vox0"]).max())
    print(f"HIP encoder + fp16 query vs reference: max|sdf - list_sdf| = {err:.3e} (bound {5e-3 * top:.3e}); "
          f"max|vox0 - list_vox0| = {err0:.3e}")
    assert vox0.dtype == torch.float32 and err0 <= 1e-5
    assert err <= 5e-3 * top
    for l in range(1, 6):
        assert vox_feat[l].dtype == torch.float16
        assert vox.levels[l].data == vox_feat[l].data_ptr() and vox.levels[l].dtype == hip.MAP_F16


def test_predict_grid_uses_the_hip_encoder():
    from list_amd import refine as RF
    from list_amd.train import _Module
    cfg = arguments.default_config(vox_res=32, train_batch_size=2, vox_encoder="hip", precision="fp16", mcube_znum=40)
    cfg.device = torch.device(DEV)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(DEV)
    ex = utils.get_class("network.executors.LIST")(cfg, _Module(net))
    img = torch.from_numpy(synth.uniform(78, (1, 3, 64, 64))).to(DEV)
    with torch.no_grad():
        frozen = net.encode(img)       # the 2-D encoders are not run-to-run deterministic: freeze the per-image stage
    calls = []

    def encode(*a, **k):
        calls.append(1)
        return frozen
    net.encode = encode
    try:
        with torch.no_grad():
            hand = voxenc.encode(frozen[4], voxenc.pack(net.vox_encoder))
        for a, b in zip(frozen[1], hand):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert all(v.dtype == torch.float16 for v in hand[1:])
        ms = net.percep_pooling.map_size
        project = 40 ** 3 >= 4 * ms * ms
        pts = utils.grid_points_on_device(-0.5, 0.5, 40, torch.device(DEV), 0, 40 ** 3).unsqueeze(0)

        def query(p):
            with torch.no_grad():
                return net.query_sdf(p, frozen[0], hand, frozen[2], ordered_points=True,
                                     project_percep=project)[0] / cfg.sdf_scale
        vol, occ, vox_feat = ex.predict_grid(img, shard=False)
        assert vol.shape == (40, 40, 40) and torch.isfinite(vol).all()
        assert torch.equal(vol, query(pts).view(40, 40, 40))
        vol_r, _, _ = ex.predict_grid(img, shard=False, refine=4)
        want, _ = RF.predict_grid_refined(query, 40, 4, device=torch.device(DEV),
                                          step=max(int(cfg.test_pointnum), 1 << 20), shard=False)
        assert torch.equal(vol_r, want)
        assert len(calls) == 2
    finally:
        del net.encode


def test_test_py_with_the_hip_encoder_writes_meshes(tmp_path):
    out = str(tmp_path / "out") + "/"
    cmd = [sys.executable, os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "test.py"),
           "--model", "network.models.LIST", "--dataset", "datasets.Datasets.SyntheticIM2SDF", "-e", "ve",
           "--output_dir", out, "--mcube_znum", "40", "--vox_res", "32", "--vox_encoder", "hip", "--precision", "fp16",
           "--testlist_file", ""]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    objs = [f for f in os.listdir(os.path.join(out, "ve", "test_objs", "synthetic")) if f.endswith("_pred.obj")]
    assert len(objs) == 2


def test_pack_is_rebuilt_after_load_state_dict():
    a = fill.fill_state(VoxelEncoder2(LAYERS), seed=2).eval()
    other = fill.fill_state(VoxelEncoder2(LAYERS), seed=5).eval()
    occ = make_occ("random", 1, 32)
    ref_a = voxenc.encode_cpu(occ, voxenc.params_of(a), storage="fp16")
    ref_b = voxenc.encode_cpu(occ, voxenc.params_of(other), storage="fp16")
    assert float(np.abs(ref_a[1].astype(np.float32) - ref_b[1].astype(np.float32)).max()) > 1e-2
    a.to(DEV)
    d_occ = torch.from_numpy(occ).to(DEV)
    with torch.no_grad():
        p1 = voxenc.pack(a)
        assert voxenc.pack(a) is p1                         # unchanged parameters: served from the cache
        check_levels(voxenc.forward(a, d_occ), ref_a, "before load_state_dict")
        a.load_state_dict(other.state_dict())
        p2 = voxenc.pack(a)
        assert p2 is not p1
        check_levels(voxenc.forward(a, d_occ), ref_b, "after load_state_dict")
        a.bn[4].running_mean.add_(0.25)                     # a buffer written in place
        assert voxenc.pack(a) is not p2


def test_training_mode_raises_instead_of_falling_back():
    cfg = arguments.default_config(vox_res=32, train_batch_size=2, vox_encoder="hip", precision="fp16")
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).to(DEV)
    img = torch.from_numpy(synth.uniform(78, (2, 3, 64, 64))).to(DEV)
    q = torch.from_numpy(synth.make_query(79, 2, 50)).to(DEV)
    net.train()
    with pytest.raises(RuntimeError, match="training mode"):
        net(img, q)
    net.eval()
    with pytest.raises(RuntimeError, match="no backward"):
        net(img, q)                                         # eval mode, but autograd would record the call
    with torch.no_grad():
        _, sdf = net(img, q)
    assert torch.isfinite(sdf).all()


def test_full_size_batch():
    """B = 8, R = 128, 2048-point occupancies.  Levels 2 .. 5 of image 0 against the restatement's stages 4 .. 7 run
    on the device's own pooled level 1; level 1 on two 16^3 blocks, each against the restatement on the crop of occ
    that holds the block and its receptive field (5 voxels per side; at the corner the crop ends at the true
    boundary, so the zero padding there is the real one)."""
    B, R = 8, 128
    enc = fill.fill_state(VoxelEncoder2(LAYERS), seed=2).eval()
    params = voxenc.params_of(enc)
    occ = point_occ(7, B, R)
    occ[B - 1, 0, 0, 0] = occ[B - 1, 2, 5, 9] = occ[B - 1, 12, 3, 0] = occ[B - 1, 7, 0, 15] = 1     # the corner block's
    enc.to(DEV)
    with torch.no_grad():
        levels, ws = voxenc.encode(torch.from_numpy(occ).to(DEV), voxenc.pack(enc), return_workspace=True)
    torch.cuda.synchronize()
    assert ws.numel() == voxenc.workspace_bytes(B, R, LAYERS) == voxenc.workspace_bytes_closed_form(B, R, LAYERS)
    for k, v in enumerate(levels):
        assert v.shape[0] == B and torch.isfinite(v).all(), k
    pooled1 = voxenc.pooled_view(ws, B, R, LAYERS, 3)[0:1].cpu().numpy()
    ref = voxenc.encode_cpu(None, params, storage="fp16", start=(4, pooled1))
    check_levels([None, None] + [v[0:1] for v in levels[2:]], ref, "B=8 R=128 image 0", first=2)
    for name, lo in (("corner", 0), ("interior", 56)):
        c0, c1 = max(lo - 5, 0), lo + 16 + 5
        crop = occ[B - 1:B, c0:c1, c0:c1, c0:c1]
        assert crop.sum() > 0
        r1 = voxenc.encode_cpu(crop, params, storage="fp16", stop_after=3)[1]
        o = lo - c0
        want = r1[:, :, o:o + 16, o:o + 16, o:o + 16].astype(np.float32)
        got = levels[1][B - 1:B, :, lo:lo + 16, lo:lo + 16, lo:lo + 16].float().cpu().numpy()
        top = float(levels[1][B - 1].float().abs().max())
        err = float(np.abs(got - want).max())
        print(f"B=8 R=128 level 1, {name} block: max|hip - restatement| = {err:.3e} (bound {HALF_BOUND * top:.3e})")
        assert err <= HALF_BOUND * top
