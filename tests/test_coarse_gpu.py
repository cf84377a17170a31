"""GPU: every launch of the HIP coarse stage (list_amd.coarse) alone, through decode_steps, on the device's own inputs,
element by element against a float64 evaluation of that one launch with the bounds of tests/_coarse_check.py; the
occupancy bit for bit against LIST.create_occ; the whole stage against its steps and the reference's goldens."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fill, synth
from list_amd import arguments, coarse, utils
from list_amd.network.modules import PointMLP, TreeGraphDecoder

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coarse_check as cc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


class Holder(torch.nn.Module):
    def __init__(self, dec, mlp=None, cam=None):
        super().__init__()
        self.point_decoder = dec
        if mlp is not None:
            self.point_mlp_coarse = mlp
        if cam is not None:
            self.spatial_transformer = cam


def camera(g2=24, hidden=40):
    nn = torch.nn
    return nn.Sequential(nn.Linear(512 + g2, hidden), nn.LeakyReLU(0.2), nn.BatchNorm1d(hidden),
                         nn.Linear(hidden, hidden), nn.LeakyReLU(0.2), nn.BatchNorm1d(hidden), nn.Linear(hidden, 12))


def small(features=None, degrees=None, negative_scale=False, seed=8):
    """A small stage: decoder (default: features [32,16,48,3], degrees [3,1,5]), point MLP, a 536 -> 40 -> 40 -> 12 camera."""
    dec = TreeGraphDecoder(2, features or cc.SMALL["features"], degrees or cc.SMALL["degrees"], 10)
    m = fill.fill_state(Holder(dec, PointMLP(), camera()), seed=seed).eval()
    if negative_scale:
        with torch.no_grad():
            for blk in (m.point_mlp_coarse.block1, m.point_mlp_coarse.block2, m.point_mlp_coarse.block3):
                blk[1].weight[::3] *= -1.0
    return m


class Stage:
    def __init__(self, model):
        self.params = coarse.params_of(model)                   # read on the CPU, before the model moves
        self.model = model.to(DEV)
        self.packed = coarse.pack(self.model)
        self.L = self.packed.shape.n_degrees


@pytest.fixture(scope="module")
def default_stage():
    cfg = arguments.default_config(vox_res=32, train_batch_size=2)
    return Stage(fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval())


@pytest.fixture(scope="module")
def small_stage():
    return Stage(small())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def check_tree(st, B, seed=5):
    code = synth.uniform(seed, (B, st.params["features"][0]))
    buf, levels = None, [code.reshape(B, 1, -1)]
    for l in range(st.L):
        buf = coarse.decode_steps(st.packed, dev(code), l, l + 1, buf=buf)
        got = (buf.pc if l == st.L - 1 else coarse.level_view(buf, st.packed, l + 1)).cpu().numpy()
        y, bound = cc.tree_reference(st.params, l, levels)        # of the device's own levels 0 .. l
        q = cc.worst(got, y, bound)
        print(f"B={B} tree_{l} {got.shape}: max error / bound = {q:.3f}, max|y| = {np.abs(y).max():.3g}")
        assert q <= 1.0, (l, q)
        levels.append(got)
    return buf


@pytest.mark.parametrize("B", [1, 3])
def test_tree_launches_of_the_default_decoder(default_stage, B):
    check_tree(default_stage, B)


@pytest.mark.parametrize("B", [1, 16, 17])
def test_tree_launches_of_the_small_decoder(small_stage, B):
    """An odd degree, degree 1, a whole image group, a partial last group and more than one group."""
    check_tree(small_stage, B)


def check_mlp(st, pc):
    B = pc.shape[0]
    buf = coarse.buffers(st.packed, B)
    buf.pc.copy_(dev(pc))
    code = dev(np.zeros((B, st.params["features"][0])))
    coarse.decode_steps(st.packed, code, st.L, st.L + 1, buf=buf)
    tm = coarse.tile_max_view(buf, st.packed).cpu().numpy()
    y, bound = cc.mlp_reference(st.params, pc)
    q = cc.worst(tm, y, bound)
    print(f"point_mlp P={pc.shape[1]} B={B}: max error / bound = {q:.3f}")
    assert tm.shape == y.shape and q <= 1.0, q
    coarse.decode_steps(st.packed, code, st.L + 1, st.L + 2, buf=buf)
    got = buf.coarse.cpu().numpy()
    assert np.array_equal(got, cc.nanmax_tiles(tm), equal_nan=True)                  # point_max: exact
    with torch.no_grad():
        ref = torch.max(st.model.point_mlp_coarse(dev(pc)), -1)[0].reshape(B, -1).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    return got


def test_point_mlp_at_4096_points(default_stage):
    check_mlp(default_stage, (synth.uniform(6, (2, 4096, 3)) - 0.5).astype(np.float32) * 0.4)


@pytest.mark.parametrize("degrees,negative_scale", [([3, 5], False), ([5, 13], False), ([5, 13], True)])
def test_point_mlp_with_a_partial_last_tile(degrees, negative_scale):
    """P = 15 (one partial tile) and P = 65 (a full tile and one of a single row); BN scales of both signs.  The points
    are small, so the padding rows (zeros) would win many channels if they took part."""
    st = Stage(small([32, 16, 3], degrees, negative_scale))
    P = degrees[0] * degrees[1]
    check_mlp(st, (synth.uniform(6, (3, P, 3)) * 0.02).astype(np.float32))


def test_point_mlp_nan_point_poisons_its_image_only():
    st = Stage(small([32, 16, 3], [5, 13]))
    pc = (synth.uniform(6, (3, 65, 3)) * 0.3).astype(np.float32)
    pc[1, 64, 1] = np.nan
    got = check_mlp(st, pc)
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()


@pytest.mark.parametrize("B", [1, 17])
def test_camera_launch(small_stage, B):
    st = small_stage
    code, g2 = synth.uniform(5, (B, 32)), synth.uniform(6, (B, 24))
    buf = coarse.decode_steps(st.packed, dev(code), 0, st.L + 2)
    buf.trans_mat.fill_(-77.0)
    coarse.decode_steps(st.packed, dev(code), st.L + 2, st.L + 3, buf=buf)               # without feat_g2: untouched
    assert bool((buf.trans_mat == -77.0).all())
    coarse.decode_steps(st.packed, dev(code), st.L + 2, st.L + 3, feat_g2=dev(g2), buf=buf)
    y, bound = cc.camera_reference(st.params, buf.coarse.cpu().numpy(), g2)
    q = cc.worst(buf.trans_mat.cpu().numpy(), y, bound)
    print(f"camera B={B}: max error / bound = {q:.3f}")
    assert q <= 1.0
    assert coarse.decode(st.packed, dev(code))[2] is None


@pytest.mark.parametrize("R", [32, 128])
def test_occupancy_is_create_occ_bit_for_bit(small_stage, R):
    st = small_stage
    net = utils.get_class("network.models.LIST")(arguments.default_config(vox_res=R, train_batch_size=2))
    pc = cc.cloud_with_edge_cases(9, 2, 15, R)
    code = dev(np.zeros((2, 32)))
    buf = coarse.buffers(st.packed, 2, R)
    buf.pc.copy_(dev(pc))
    buf.occ.fill_(5.0)                                                                # the clear must clear
    coarse.decode_steps(st.packed, code, st.L + 3, st.L + 5, buf=buf, bb_min=net.bb_min, bb_max=net.bb_max)
    ref = net.create_occ(buf.pc)
    assert torch.equal(buf.occ, ref) and np.array_equal(buf.occ.cpu().numpy(), coarse.occupancy_cpu(pc, R))
    bad = pc.copy()
    bad[0, 3] = [np.nan, 0.0, 0.0]
    bad[1, 4] = [0.1, -np.inf, 0.0]
    buf.pc.copy_(dev(bad))
    coarse.decode_steps(st.packed, code, st.L + 3, st.L + 5, buf=buf)
    assert np.array_equal(buf.occ.cpu().numpy(), coarse.occupancy_cpu(bad, R))       # only the finite points mark


def test_decode_is_the_chain_of_its_steps(small_stage):
    st = small_stage
    code, g2 = dev(synth.uniform(5, (17, 32))), dev(synth.uniform(6, (17, 24)))
    whole = coarse.decode(st.packed, code, g2, vox_res=32)
    buf = None
    for s in range(len(coarse.step_names(st.packed.shape))):
        buf = coarse.decode_steps(st.packed, code, s, s + 1, feat_g2=g2, buf=buf, vox_res=32)
    for a, b in zip(whole, (buf.pc, buf.coarse, buf.trans_mat, buf.occ)):
        assert torch.equal(a, b)
    assert coarse.pack(st.model) is st.packed                                         # cached on the module


def test_coarse_cloud_matches_the_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "models.npz"))
    cfg = arguments.default_config(vox_res=32, train_batch_size=2, coarse_stage="hip")
    net = fill.fill_state(utils.get_class("network.models.CoarseNet")(cfg), seed=1).eval()
    with torch.no_grad():
        code, _ = net.image_encoder(torch.from_numpy(synth.uniform(77, (2, 3, 128, 128))))      # on the CPU, as the golden
        net.to(DEV)
        pc = coarse.forward(net, code.to(DEV))[0].cpu().numpy()
        whole = net(torch.from_numpy(synth.uniform(77, (2, 3, 128, 128))).to(DEV)).cpu().numpy()
    err = float(np.abs(pc - g["coarse_pc"]).max())
    print(f"max|pc_hip - coarse_pc| = {err:.3e}; with the image encoder on the device too: "
          f"{np.abs(whole - g['coarse_pc']).max():.3e}")
    assert pc.shape == (2, 4096, 3) and err <= 2e-6
    net.train()
    with pytest.raises(RuntimeError, match="training mode"):
        net(torch.zeros(2, 3, 128, 128, device=DEV))


@pytest.mark.parametrize("vox_encoder", ["torch", "hip"])
def test_list_with_the_hip_coarse_stage_matches_the_reference_model(golden_dir, vox_encoder):
    """The tolerances of tests/test_boundary_gpu.py (whole model on the device, fp32-grade query: 2e-3) and of
    tests/test_voxenc_gpu.py (HIP encoder and fp16 query: 5e-3 of max(1, max|sdf|)) for the same goldens."""
    g = np.load(os.path.join(golden_dir, "models.npz"))
    kw = {"vox_encoder": "hip", "precision": "fp16"} if vox_encoder == "hip" else {}
    cfg = arguments.default_config(vox_res=32, train_batch_size=2, coarse_stage="hip", **kw)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(DEV)
    img = torch.from_numpy(synth.uniform(78, (2, 3, 64, 64))).to(DEV)
    q = torch.from_numpy(synth.make_query(79, 2, 100)).to(DEV)
    tm = torch.from_numpy(synth.make_trans_mat(80, 2)).to(DEV)
    with torch.no_grad():
        _, sdf = net(img, q)
        _, sdf2 = net(img, q, tm)
    for name, got in (("list_sdf", sdf), ("list_sdf_given_transmat", sdf2)):
        bound = 5e-3 * max(1.0, float(np.abs(g[name]).max())) if vox_encoder == "hip" else 2e-3
        err = float(np.abs(got.cpu().numpy() - g[name]).max())
        print(f"coarse_stage=hip, vox_encoder={vox_encoder}: max|sdf - {name}| = {err:.3e} (bound {bound:.1e})")
        assert err < bound
