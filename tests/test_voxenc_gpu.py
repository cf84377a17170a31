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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxenc_check as vc  # noqa: E402

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


# ---- every launch on its own, every element against its own bound (tests/_voxenc_check.py) ---------------------------
def _occ(kind, B, R, seed=11):
    if kind == "ones":
        return np.ones((B, R, R, R), dtype=np.float32)
    p = {"sparse": 0.03, "dense": 0.5}[kind]
    return (np.random.default_rng(seed).random((B, R, R, R)) < p).astype(np.float32)


def _blocks(D, R, thick, rng):
    """The blocks [(z0, z1, y0, y1, x0, x1)] of a volume of side D that are checked.  R <= 48 and every level of side
    <= 24: the whole volume.  Wider levels of R = 80, 96: the first and the last slab of bricks along z over the whole
    xy extent (two faces, eight edges, all eight corners, and every last brick along x and y) and three seeded
    8 x 8 x 16 blocks (2 x 2 x 2 bricks) inside.  R = 256: the two 16^3 corner blocks on the diagonal and one inside."""
    if R <= 48 or D <= 24:
        return [(0, D, 0, D, 0, D)]
    if R == 256:
        o = 16 * int(rng.integers(1, max(D // 16 - 1, 2)))
        return [(0, 16) * 3, (D - 16, D) * 3, (o, o + 16) * 3]
    out = [(0, thick, 0, D, 0, D), (D - thick, D, 0, D, 0, D)]
    for _ in range(3):
        z, y = (thick + 4 * int(rng.integers(0, (D - 2 * thick - 8) // 4 + 1)) for _ in range(2))
        x = 8 * int(rng.integers(1, (D - 16) // 8))
        out.append((z, z + 8, y, y + 8, x, x + 16))
    return out


def _io(step, L, occ, levels, ws, B, R, layers):
    """(input, output) of launch `step` as device tensors [B,D,D,D,C] (views of the buffers the launch uses)."""
    n = B * R ** 3
    cl = lambda v: v.permute(0, 2, 3, 4, 1)
    t0 = ws[0:4 * n].view(torch.float32).view(B, R, R, R, 1)
    o1 = voxenc._align(4 * n)
    t1 = ws[o1:o1 + 4 * n].view(torch.float32).view(B, R, R, R, 1)
    if step < 3:
        return (occ.unsqueeze(-1), t0, t1)[step], (t0, t1, cl(levels[0]))[step]
    mid = cl(voxenc.mid_view(ws, B, R, layers, L.stage))
    if L.second:
        return mid, cl(levels[L.stage - 2])
    return (cl(levels[0]) if L.stage == 3 else cl(voxenc.pooled_view(ws, B, R, layers, L.stage - 1))), mid


def _assert_pool(levels, ws, B, R, layers, stage, what):
    """The fused pool is max_pool3d of the level just written, bit for bit; a window that holds a NaN gives a NaN."""
    pooled = voxenc.pooled_view(ws, B, R, layers, stage).float()
    want = torch.nn.functional.max_pool3d(levels[stage - 2].float(), 2)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(pooled), nan), (what, stage)
    assert torch.equal(pooled[~nan], want[~nan]), (what, stage)
    return int(nan.sum())


def per_launch(module, occ, what, poke=None, table=None):
    """Runs the 13 launches one at a time on the device and checks each against the float64 reference of that layer on
    the device's own input (vc.check), and the fused pool of stages 3 .. 6.  poke(step, ws) may write into the
    workspace before a launch.  Returns (levels, ws, worst error / bound per launch)."""
    params = voxenc.params_of(module)
    layers, Ls = params["layers"], vc.launches(params)
    B, R = occ.shape[0], occ.shape[1]
    rng = np.random.default_rng(17)
    module.to(DEV)
    try:
        packed = voxenc.pack(module)
        d_occ = torch.from_numpy(occ).to(DEV)
        buffers, worst = None, []
        for step, L in enumerate(Ls):
            if buffers is None:
                levels, ws, buffers = voxenc.encode_steps(d_occ, packed, 0, 0)
            if poke is not None:
                poke(step, ws)
            levels, ws, buffers = voxenc.encode_steps(d_occ, packed, step, step + 1, buffers)
            torch.cuda.synchronize()
            x_dev, y_dev = _io(step, L, d_occ, levels, ws, B, R, layers)
            D = L.D(R)
            assert x_dev.shape == (B, D, D, D, L.cin) and y_dev.shape == (B, D, D, D, L.cout)
            q = 0.0
            for blk in _blocks(D, R, 4 if L.mfma else 8, rng):
                (za, zb, sz), (ya, yb, sy), (xa, xb, sx) = (vc.crop_range(blk[2 * i], blk[2 * i + 1], D)
                                                            for i in range(3))
                x = x_dev[:, za:zb, ya:yb, xa:xb].cpu().numpy()
                got = y_dev[:, blk[0]:blk[1], blk[2]:blk[3], blk[4]:blk[5]].cpu().numpy()
                q = max(q, vc.check(got, x, L, inner=(sz, sy, sx)))
            worst.append(q)
            print(f"{what}: {L.name:9s} {L.template():12s} D={D:3d}: max error / bound = {q:.3f}")
            if table is not None:
                table.append((what, L.name, L.template(), D, q))
            if L.second and L.stage < voxenc.N_STAGES - 1:
                _assert_pool(levels, ws, B, R, layers, L.stage, what)
        assert ws.numel() == voxenc.workspace_bytes(B, R, layers) == voxenc.workspace_bytes_closed_form(B, R, layers)
        bad = [(L.name, q) for L, q in zip(Ls, worst) if not q <= 1.0]
        assert not bad, (what, bad)
        return levels, ws, worst
    finally:
        module.cpu()


def whole_pipeline(module, occ, what, images=None):
    """The existing check: the whole forward against the whole restatement (check_levels), on `images` (all)."""
    params = voxenc.params_of(module)
    module.to(DEV)
    try:
        levels = voxenc.encode(torch.from_numpy(occ).to(DEV), voxenc.pack(module))
        torch.cuda.synchronize()
        levels = [v.cpu() for v in levels]
    finally:
        module.cpu()
    sel = slice(None) if images is None else images
    ref = voxenc.encode_cpu(occ[sel], params, storage="fp16")
    check_levels([v[sel] for v in levels], ref, what)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [16, 32, 48, 80, 96])
def test_every_launch_at_every_grid(enc, R, B):
    """Default layers ([1,1,1,1,16,32,64,128,128]: expand C=16, then <16,1> <16,2> <32,2> <32,4> <32,4> <32,8> x 4) at
    grids whose levels are single partial bricks (R = 16: 16, 8, 4, 2, 1), powers of two (32), several bricks with a
    partial last one (R = 48: 48, 24, 12 = 8 + 4, 6 = 4 + 2, 3; R = 80: 80, 40, 20, 10, 5) and R = 96.  R = 16 is
    accepted by the HIP path (the torch module raises there; test_voxenc_cpu.py) and is checked like every size.
    The whole-pipeline check runs on every image up to R = 48 and on the last image (the largest image offset) of the
    two wider grids, where the restatement of three images would cost more than the rest of this file."""
    occ = _occ("sparse", B, R)
    per_launch(enc, occ, f"R={R} B={B}")
    whole_pipeline(enc, occ, f"R={R} B={B}", images=None if R <= 48 else slice(B - 1, B))


@pytest.mark.parametrize("layers,R", [(vc.LIST_A, 48), (vc.LIST_B, 32)])
def test_every_launch_of_other_architectures(layers, R):
    """The instantiations and widths the default network never reaches, launch by launch (conv_3 .. conv_7_0):
      [1,1,1,1,64,16,128,16,64], R = 48: expand C=64, <32,4> | <32,1> <16,1> | <16,8> <32,8> | <32,1> <16,1> |
                                          <16,4> <32,4>            -- first runs of <32,1>, <16,8>, <16,4>
      [1,1,1,1,128,128,32,16,16], R = 32: expand C=128 (its LDS limit), <32,8> | <32,8> <32,8> | <32,2> <32,2> |
                                          <32,1> <16,1> | <16,1> <16,1>   -- a 128-channel level 1."""
    m = fill.fill_state(VoxelEncoder2(layers), seed=2).eval()
    occ = _occ("sparse", 1, R)
    per_launch(m, occ, f"layers={layers[4:]} R={R}")
    whole_pipeline(m, occ, f"layers={layers[4:]} R={R}")


@pytest.mark.parametrize("R", [32, 48])
@pytest.mark.parametrize("kind", ["ones", "dense"])
def test_every_launch_on_full_halos(enc, kind, R):
    """All ones and dense random (p = 0.5) occupancy: every halo voxel is non-zero, so a brick halo that reads zero
    where the neighbouring brick has data, or data where the volume ends, is an error of order one."""
    occ = _occ(kind, 1, R)
    per_launch(enc, occ, f"{kind} R={R}")
    whole_pipeline(enc, occ, f"{kind} R={R}")


def _signed_bn(layers, seed):
    """fill_state, then BN scales of both signs with exact zeros among them and shifts of both signs (seeded)."""
    m = fill.fill_state(VoxelEncoder2(layers), seed=2).eval()
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for bn in m.bn:
            n = bn.weight.numel()
            w = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
            if n > 1:
                w[rng.choice(n, max(n // 8, 1), replace=False)] = 0.0
            bn.weight.copy_(torch.from_numpy(w.astype(np.float32)))
            bn.bias.copy_(torch.from_numpy(rng.uniform(-0.3, 0.3, n).astype(np.float32)))
    return m


def test_every_launch_with_negative_and_zero_bn_scales():
    """ReLU, THEN the affine: a negative scale gives negative activations (the pool is over negative values, the next
    convolution reads them), a zero scale a constant channel."""
    m = _signed_bn(LAYERS, 23)
    assert any((bn.weight < 0).any() and (bn.weight == 0).any() for bn in m.bn[3:])
    occ = _occ("sparse", 2, 32, seed=12)
    levels, _, _ = per_launch(m, occ, "signed BN R=32 B=2")
    assert all(float(v.float().min()) < 0 for v in levels[1:])
    whole_pipeline(m, occ, "signed BN R=32 B=2")


def test_non_finite_activations_propagate_as_in_the_reference(enc):
    """A NaN and a +inf written into the pooled output of stage 3 (the fp16 input of conv_4) between two launches:
    only the device sees them.  Per launch the non-finite classes must be those of the float64 reference (vc.ratios);
    at conv_4 that is: NaN at exactly the 3^3 neighbourhood of the NaN voxel, in every channel; around the +inf voxel
    +inf where the tap's weight is positive and relu(-inf) = 0 where it is negative.  The fused pools return NaN for
    every window that holds one, as max_pool3d does (_assert_pool)."""
    R, at_nan, at_inf = 32, (3, 0, 8), (9, 12, 7)              # voxels of the 16^3 pooled volume: a face and inside

    def poke(step, ws):
        if step == 5:
            v = voxenc.pooled_view(ws, 1, R, LAYERS, 3)
            v[0, 5, at_nan[0], at_nan[1], at_nan[2]] = float("nan")
            v[0, 9, at_inf[0], at_inf[1], at_inf[2]] = float("inf")
    levels, ws, _ = per_launch(enc, _occ("sparse", 1, R), "non-finite R=32", poke=poke)
    lvl2 = levels[2].float().cpu().numpy()[0]                  # [C,16,16,16]: two launches after the poke
    assert np.isnan(lvl2).any() and np.isfinite(lvl2).any()
    near = np.zeros((16, 16, 16), dtype=bool)
    for z, y, x in (at_nan, at_inf):
        near[max(z - 2, 0):z + 3, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = True
    assert np.isfinite(lvl2[:, ~near]).all()                   # two 3^3 convolutions: nothing beyond 5^3
    nan5 = np.zeros((16, 16, 16), dtype=bool)
    z, y, x = at_nan
    nan5[max(z - 2, 0):z + 3, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = True
    assert np.isnan(lvl2[:, nan5]).all()
    assert torch.isnan(voxenc.pooled_view(ws, 1, R, LAYERS, 4)).any()


def test_fp16_overflow_gives_infinity_not_saturation():
    """conv_3 (fp32 weights) and conv_3_0 scaled so that level 1 passes 65504: the output holds +inf where the
    reference rounded to fp16 does (include/list_voxenc.h: not saturated), and the later launches, which now read
    infinities, agree with the reference by class."""
    m = fill.fill_state(VoxelEncoder2(LAYERS), seed=2).eval()
    with torch.no_grad():
        m.conv["conv_3"].weight.mul_(2000.0)
        m.conv["conv_3_0"].weight.mul_(80.0)
    assert float(m.conv["conv_3_0"].weight.abs().max()) < 60000    # the fp16 weights themselves stay finite
    levels, _, _ = per_launch(m, _occ("sparse", 1, 32), "overflow R=32")
    lvl1 = levels[1].float()
    n_inf = int(torch.isinf(lvl1).sum())
    print(f"overflow R=32: {n_inf} of {lvl1.numel()} elements of level 1 are infinite")
    assert n_inf > 0 and not torch.isnan(lvl1).any() and float(lvl1[torch.isfinite(lvl1)].max()) > 4096


def test_every_launch_at_the_largest_grid(enc):
    """R = 256 = LIST_VOXENC_MAX_R, B = 1 (the workspace is about 0.8 GiB): finite outputs, buffer sizes equal to
    their closed forms (per_launch asserts it), the fused pools over the whole volumes, and the per-launch check on
    the two corner blocks of the diagonal and one interior block of every launch."""
    occ = _occ("sparse", 1, 256)
    levels, ws, _ = per_launch(enc, occ, "R=256 B=1")
    assert ws.numel() == voxenc.workspace_bytes_closed_form(1, 256, LAYERS) == 725 << 20
    for k, v in enumerate(levels):
        assert v.shape[2] == 256 >> max(k - 1, 0) and torch.isfinite(v).all(), k
