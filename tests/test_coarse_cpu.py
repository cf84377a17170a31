"""CPU: the numpy restatement of the HIP coarse stage (coarse.decode_cpu) against the torch modules and the reference's
golden, the rules the device follows, the C ABI of include/list_coarse.h without a GPU (exports, sizes, refusals), and
the model option."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fill, synth
from list_amd import arguments, coarse, hip, utils
from list_amd.network.modules import PointMLP, TreeGraphDecoder

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H  # noqa: E402
import _coarse_check as cc  # noqa: E402

DEFAULT_F, DEFAULT_D = [128, 128, 256, 256, 256, 128, 128, 3], [2, 2, 2, 2, 2, 2, 64]


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


@pytest.fixture(scope="module")
def cfg():
    return arguments.default_config(vox_res=32, train_batch_size=2)


@pytest.fixture(scope="module")
def coarsenet(cfg):
    """The CoarseNet of test_coarsenet_cpu_plumbing_matches_reference, its image code and its parameters."""
    net = fill.fill_state(utils.get_class("network.models.CoarseNet")(cfg), seed=1).eval()
    with torch.no_grad():
        code, _ = net.image_encoder(torch.from_numpy(synth.uniform(77, (2, 3, 128, 128))))
    return net, code.numpy(), coarse.params_of(net)


def small_decoder(seed=3):
    return fill.fill_state(TreeGraphDecoder(2, cc.SMALL["features"], cc.SMALL["degrees"], 10), seed=seed).eval()


# ---- restatement -----------------------------------------------------------------------------------------------------
def test_device_restatement_is_the_reference_golden(coarsenet, golden_dir):
    _, code, params = coarsenet
    g = np.load(os.path.join(golden_dir, "models.npz"))
    pc = coarse.decode_cpu(params, code, arithmetic="device")["pc"]
    assert pc.shape == (2, 4096, 3) and pc.dtype == np.float32
    err = float(np.abs(pc - g["coarse_pc"]).max())
    print(f"max|decode_cpu('device') - coarse_pc| = {err:.3e}, max|pc| = {np.abs(pc).max():.3f}")
    assert err <= 2e-6


@pytest.mark.parametrize("which", ["default", "small"])
def test_exact_restatement_is_the_torch_decoder_in_float64(coarsenet, which):
    if which == "default":
        dec, code = copy.deepcopy(coarsenet[0].point_decoder).double(), coarsenet[1][:1]
    else:
        dec, code = small_decoder().double(), synth.uniform(5, (3, 32))
    with torch.no_grad():
        ref = dec([torch.from_numpy(code).double().unsqueeze(1)]).numpy()
    got = coarse.decode_cpu(coarse.params_of(dec), code, arithmetic="exact")["pc"]
    err = float(np.abs(got - ref).max())
    print(f"{which}: max|decode_cpu('exact') - torch float64| = {err:.3e}, max|pc| = {np.abs(ref).max():.3f}")
    assert got.dtype == np.float64 and got.shape == ref.shape and err <= 1e-12


@pytest.mark.parametrize("which", ["default", "small"])
def test_composed_w_loop_is_the_uncomposed_one_in_float64(coarsenet, which):
    """W_loop has no nonlinearity between its two Linears: the decoder with loop1 @ loop0 as ONE float64 matrix (written
    here as loop0' = loop1 @ loop0, loop1' = I) equals the reference formula."""
    if which == "default":
        params, code = coarsenet[2], coarsenet[1][:1]
    else:
        params, code = coarse.params_of(small_decoder()), synth.uniform(5, (3, 32))
    composed = dict(params, layers=[dict(l, loop0=coarse.compose(l["loop0"], l["loop1"], np.float64),
                                         loop1=np.eye(l["loop1"].shape[0])) for l in params["layers"]])
    a = coarse.decode_cpu(params, code, arithmetic="exact")["pc"]
    b = coarse.decode_cpu(composed, code, arithmetic="exact")["pc"]
    err = float(np.abs(a - b).max())
    print(f"{which}: max|composed - uncomposed| in float64 = {err:.3e}")
    assert err <= 1e-12


# ---- device rules against the torch modules --------------------------------------------------------------------------
def _mlp(seed=4, negative_scale=False, big_bias=False):
    m = fill.fill_state(PointMLP(), seed=seed).eval()
    with torch.no_grad():
        if negative_scale:
            for blk in (m.block1, m.block2, m.block3):
                blk[1].weight[::3] *= -1.0
        if big_bias:                       # a padding row (a point at the origin would do the same) gives large values
            m.block1[0].bias += 3.0
    return m


class _Holder(torch.nn.Module):
    def __init__(self, dec, mlp=None, cam=None):
        super().__init__()
        self.point_decoder = dec
        if mlp is not None:
            self.point_mlp_coarse = mlp
        if cam is not None:
            self.spatial_transformer = cam


def _code_of(mlp, pc):
    """coarse (device arithmetic) of a given cloud, and the launch's float64 reference with its bound."""
    params = coarse.params_of(_Holder(small_decoder(), mlp))
    x = np.asarray(pc, np.float32)
    h = x
    for lay in params["mlp"]:
        h = coarse._dense(h, lay, False, "bn_relu")
    y, bound = cc.mlp_reference(params, x)
    return h.max(axis=1), y.max(axis=1), bound.max(axis=1), params


@pytest.mark.parametrize("P", [15, 65])
@pytest.mark.parametrize("negative_scale", [False, True])
def test_padding_rows_take_no_part_in_the_max(P, negative_scale):
    """The torch module has no padding rows; the restatement's tiles hold the real rows only.  Both fp32 evaluations
    lie within the launch's bound of its float64 value.  And the rule matters: with a row of zeros appended -- what a
    padded tile holds -- some channel's maximum changes."""
    m = _mlp(negative_scale=negative_scale, big_bias=True)
    pc = (synth.uniform(6, (3, P, 3)) * 0.02).astype(np.float32)
    with torch.no_grad():
        ref = torch.max(m(torch.from_numpy(pc)), -1)[0].reshape(3, -1).numpy()
    got, y, bound, params = _code_of(m, pc)
    # torch's BN is (x - mean) / sqrt(var + eps) * g + b, the device's x * s + t: 4 more roundings of values <= |y| + |t|
    slack = 8 * cc.U24 * (np.abs(y) + 1.0)
    assert cc.worst(got, y, bound) <= 1.0 and cc.worst(ref, y, 2 * bound + slack) <= 1.0
    padded = np.concatenate([pc, np.zeros((3, 1, 3), np.float32)], axis=1)
    assert (_code_of(m, padded)[0] > got).any()
    tm = coarse.decode_cpu(params, synth.uniform(5, (3, 32)))["tile_max"]
    assert tm.shape == (3, 1, 512)


def test_nan_point_poisons_its_image_only():
    m = _mlp()
    pc = (synth.uniform(6, (3, 65, 3)) * 0.3).astype(np.float32)
    pc[1, 64, 1] = np.nan
    with torch.no_grad():
        ref = torch.max(m(torch.from_numpy(pc)), -1)[0].reshape(3, -1).numpy()
    got, y, bound, _ = _code_of(m, pc)
    assert np.isnan(ref[1]).all() and np.isfinite(ref[[0, 2]]).all()
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and cc.worst(got, y, bound) <= 1.0
    tiles = cc.mlp_reference(coarse.params_of(_Holder(small_decoder(), m)), pc)[0]
    assert np.isfinite(tiles[1, 0]).all() and np.isnan(tiles[1, 1]).all()          # the NaN sits in the second tile
    assert np.isnan(cc.nanmax_tiles(tiles)[1]).all()


@pytest.mark.parametrize("R", [32, 128])
def test_occupancy_rounding_is_create_occ(cfg, R):
    LIST = utils.get_class("network.models.LIST")
    net = LIST(arguments.default_config(vox_res=R, train_batch_size=2))
    pc = cc.cloud_with_edge_cases(9, 2, 200, R)
    ref = net.create_occ(torch.from_numpy(pc)).numpy()
    got = coarse.occupancy_cpu(pc, R, net.bb_min, net.bb_max)
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    assert 0 < got.sum() < 2 * 200                                     # duplicates and ties share voxels
    bad = pc.copy()
    bad[0, 50] = [np.nan, 0.0, 0.0]
    bad[1, 51] = [0.0, np.inf, 0.0]
    keep = np.ones(200, bool)
    keep[[50]] = False
    only = coarse.occupancy_cpu(bad, R)
    assert np.array_equal(only[0], coarse.occupancy_cpu(pc[:1, keep], R)[0])
    assert np.array_equal(only[1], coarse.occupancy_cpu(np.delete(pc[1:], 51, axis=1), R)[0])


# ---- the per-launch check has teeth ----------------------------------------------------------------------------------
def test_per_launch_check_accepts_the_restatement_and_rejects_wrong_layers():
    cam = torch.nn.Sequential(torch.nn.Linear(512 + 24, 40), torch.nn.LeakyReLU(0.2), torch.nn.BatchNorm1d(40),
                              torch.nn.Linear(40, 40), torch.nn.LeakyReLU(0.2), torch.nn.BatchNorm1d(40),
                              torch.nn.Linear(40, 12))
    model = fill.fill_state(_Holder(small_decoder(), _mlp(), cam), seed=8).eval()
    params = coarse.params_of(model)
    code, g2 = synth.uniform(5, (3, 32)), synth.uniform(6, (3, 24))
    r = coarse.decode_cpu(params, code, g2)
    for l in range(3):
        y, bound = cc.tree_reference(params, l, r["levels"][:l + 1])
        q = cc.worst(r["levels"][l + 1], y, bound)
        print(f"tree_{l}: restatement, max error / bound = {q:.3f}")
        assert q <= 1.0
        if l > 0:                                                      # the ancestor of node n is n // reps, not n % m
            wrong = [np.roll(v, 1, axis=1) if 0 < i < l else v for i, v in enumerate(r["levels"][:l + 1])]
            if l > 1:
                assert cc.worst(coarse.tree_layer_cpu(params, l, wrong), y, bound) > 1.0
        nob = dict(params, layers=[dict(x, bias=x["bias"] * 0) for x in params["layers"]])
        if params["layers"][l]["activation"]:
            assert cc.worst(coarse.tree_layer_cpu(nob, l, r["levels"][:l + 1]), y, bound) > 1.0
    y, bound = cc.mlp_reference(params, r["pc"])
    assert cc.worst(r["tile_max"], y, bound) <= 1.0
    assert cc.worst(np.roll(r["tile_max"], 1, axis=2), y, bound) > 1.0
    y, bound = cc.camera_reference(params, r["coarse"], g2)
    assert cc.worst(r["trans_mat"], y, bound) <= 1.0
    assert cc.worst(r["trans_mat"].reshape(3, 3, 4).transpose(0, 2, 1), y, bound) > 1.0
    with torch.no_grad():                                              # ... and the camera is the torch module's
        ref = model.spatial_transformer(torch.from_numpy(np.concatenate([r["coarse"], g2], 1))).numpy()
    assert np.abs(ref.reshape(3, 4, 3) - y).max() <= 1e-5 * max(1.0, np.abs(y).max())


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    names = H.declared("list_coarse.h")
    assert names == sorted(coarse.COARSE_EXPORTS) and len(names) == 7
    lib = coarse.load()
    exported = H.exported(hip.LIB_PATH)
    assert {n for n in exported if n.startswith("list_coarse_")} == set(names)
    assert not set(names) & set(hip.EXPORTS)
    for n in names:
        assert getattr(lib, n) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9


def test_buffer_sizes_match_their_closed_forms():
    for f, d, kw in ((DEFAULT_F, DEFAULT_D, {}), (cc.SMALL["features"], cc.SMALL["degrees"], {"has_camera": False}),
                     ([16, 256, 3], [7, 9], {"has_mlp": False, "has_camera": False}),
                     ([256, 3], [1], {"g2": 1024, "hidden": 256})):
        s = coarse.shape_of(f, d, **kw)
        assert coarse.weight_bytes(s) == coarse.weight_bytes_closed_form(s) > 0
        for B in (1, 8, 17):
            assert coarse.workspace_bytes(s, B) == coarse.workspace_bytes_closed_form(s, B) > 0
    s = coarse.shape_of(DEFAULT_F, DEFAULT_D)
    assert coarse.weight_bytes(s) < 8 << 20            # no second copy of the 268 MB W_branch
    # B = 1: levels of 2 x 128, 4 x 256, 8 x 256, 16 x 256, 32 x 128, 64 x 128 floats and 64 tiles x 512 maxima
    assert coarse.workspace_bytes(s, 1) == 4 * (256 + 1024 + 2048 + 4096 + 4096 + 8192 + 64 * 512)
    assert coarse.load().list_coarse_n_steps(C.byref(s)) == 12 == len(coarse.step_names(s))


def _clone(io):
    out = coarse._IO()
    C.memmove(C.byref(out), C.byref(io), C.sizeof(io))
    return out


def test_refusals_carry_a_message_without_a_gpu():
    lib = coarse.load()
    for f, d, word in (([128, 40, 3], [2, 2], "multiple of 16"), ([128, 128, 3], [2, 2, 2], "one longer than degrees"),
                       ([128, 3], [0], "at least 1"), ([128, 4], [2], "3 coordinates"), ([512, 3], [2], "at most 256")):
        s = coarse.shape_of(f, d)
        assert lib.list_coarse_weight_bytes(C.byref(s)) == 0 and word in coarse.last_error(), coarse.last_error()
        with pytest.raises(hip.ListError, match=word):
            coarse.weight_bytes(s)
        assert lib.list_coarse_workspace_bytes(C.byref(s), 1) == 0 and lib.list_coarse_n_steps(C.byref(s)) == 0
    s = coarse.shape_of(DEFAULT_F, DEFAULT_D)
    assert lib.list_coarse_weight_bytes(None) == 0 and "shape is NULL" in coarse.last_error()
    assert lib.list_coarse_workspace_bytes(C.byref(s), 0) == 0 and "B = 0" in coarse.last_error()
    # NULL pointers, R and short buffers are refused on the host, before any HIP call (the dummies are never read)
    io = coarse._IO()
    io.B, io.R, io.bb_min, io.bb_extent = 1, 32, -0.5, 1.0
    for name in ("feat_g", "feat_g2", "packed", "workspace", "pc", "coarse", "trans_mat", "occ"):
        setattr(io, name, 256)
    for l in range(7):
        io.w_branch[l] = 256
    io.packed_bytes = io.workspace_bytes = 1 << 30
    assert lib.list_coarse_forward(C.byref(s), None, None) == hip.ERR_ARG and "io is NULL" in coarse.last_error()
    for name in ("feat_g", "packed", "workspace", "pc"):
        bad = _clone(io)
        setattr(bad, name, None)
        assert lib.list_coarse_forward(C.byref(s), C.byref(bad), None) == hip.ERR_ARG
        assert f"{name} is NULL" in coarse.last_error()
    bad = _clone(io)
    bad.w_branch[6] = None
    assert lib.list_coarse_forward(C.byref(s), C.byref(bad), None) == hip.ERR_ARG
    assert "w_branch[6] is NULL" in coarse.last_error()
    bad.w_branch[6] = 260
    assert lib.list_coarse_forward(C.byref(s), C.byref(bad), None) == hip.ERR_ARG and "aligned" in coarse.last_error()
    bad = _clone(io)
    bad.R = 257
    assert lib.list_coarse_forward(C.byref(s), C.byref(bad), None) == hip.ERR_SHAPE and "R = 257" in coarse.last_error()
    bad = _clone(io)
    bad.workspace_bytes = coarse.workspace_bytes(s, 1) - 1
    assert lib.list_coarse_forward(C.byref(s), C.byref(bad), None) == hip.ERR_WORKSPACE
    assert "list_coarse_workspace_bytes" in coarse.last_error()
    bad = _clone(io)
    bad.packed_bytes = 16
    assert lib.list_coarse_forward(C.byref(s), C.byref(bad), None) == hip.ERR_WORKSPACE
    assert "packed holds 16 bytes" in coarse.last_error()
    assert lib.list_coarse_forward_steps(C.byref(s), C.byref(io), 3, 13, None) == hip.ERR_ARG
    assert "steps [3, 13)" in coarse.last_error()
    assert lib.list_coarse_prep_weights(C.byref(s), None, 256, 1 << 30, None) == hip.ERR_ARG
    assert "params is NULL" in coarse.last_error()
    nocam = coarse.shape_of(DEFAULT_F, DEFAULT_D, has_camera=False)
    assert lib.list_coarse_forward(C.byref(nocam), C.byref(io), None) == hip.ERR_ARG and "no camera" in coarse.last_error()
    with pytest.raises(hip.ListError, match="at most 8 layers"):
        coarse.shape_of([16] * 9 + [3], [1] * 9)


# ---- the model option ------------------------------------------------------------------------------------------------
def test_model_option_defaults_to_torch_and_leaves_the_cpu_alone(cfg):
    assert arguments.default_config().coarse_stage == "torch"
    assert arguments.get_args(["--coarse_stage", "hip"]).coarse_stage == "hip"
    with pytest.raises(SystemExit):
        arguments.get_args(["--coarse_stage", "triton"])
    LIST, CoarseNet = utils.get_class("network.models.LIST"), utils.get_class("network.models.CoarseNet")
    for cls in (LIST, CoarseNet):
        with pytest.raises(ValueError, match="coarse_stage"):
            cls(arguments.default_config(vox_res=32, train_batch_size=2, coarse_stage="triton"))
    base = fill.fill_state(LIST(cfg), seed=2).eval()
    opt = fill.fill_state(LIST(arguments.default_config(vox_res=32, train_batch_size=2, coarse_stage="hip")), seed=2).eval()
    assert (base.coarse_stage, opt.coarse_stage) == ("torch", "hip")
    assert list(opt.state_dict()) == list(base.state_dict())
    img = torch.from_numpy(synth.uniform(78, (2, 3, 64, 64)))
    with torch.no_grad():                                              # tensors on the CPU: the torch modules, as before
        a, b = base.encode(img), opt.encode(img)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


def test_forward_refuses_training_mode_and_gradients(cfg):
    net = utils.get_class("network.models.LIST")(cfg)
    g, g2 = torch.zeros(2, 128), torch.zeros(2, 128)
    net.train()
    with pytest.raises(RuntimeError, match="training mode"):
        coarse.forward(net, g, g2, 32)
    net.eval()
    with pytest.raises(RuntimeError, match="no backward"):
        coarse.forward(net, g, g2, 32)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        coarse.forward(net, g, g2, 32)                               # a CPU model: an error, never the torch modules
