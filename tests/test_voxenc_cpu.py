"""CPU: the numpy restatement of the HIP occupancy encoder (voxenc.encode_cpu) against the torch module and the
reference's golden, the C ABI of include/list_voxenc.h without a GPU (exports, sizes, refusals), and the model option."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import fill, synth
from list_amd import arguments, hip, utils, voxenc
from list_amd.network.modules import VoxelEncoder2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [1, 1, 1, 1, 16, 32, 64, 128, 128]


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def random_occ(seed, B, R, p=0.03):
    return (np.random.default_rng(seed).random((B, R, R, R)) < p).astype(np.float32)


def face_occ(B, R):
    """Ones on all six faces of the grid (and a few inside): every padded side of the convolutions is exercised."""
    occ = np.zeros((B, R, R, R), dtype=np.float32)
    occ[:, 0, 3:9, 5:7] = 1
    occ[:, R - 1, 10:12, 1:20] = 1
    occ[:, 4:6, 0, 2:9] = 1
    occ[:, 20:23, R - 1, 7] = 1
    occ[:, 7, 7:19, 0] = 1
    occ[:, 9:30, 9, R - 1] = 1
    occ[:, 0, 0, 0] = occ[:, R - 1, R - 1, R - 1] = 1
    occ[:, R // 2, R // 2, R // 2] = 1
    return occ


@pytest.mark.parametrize("kind", ["random", "faces"])
def test_exact_restatement_is_the_torch_module(kind):
    """float64 restatement against VoxelEncoder2.double().eval(): <= 1e-10 of each level's maximum (sums of at most
    3456 float64 terms).  fill_state gives non-trivial BN statistics, so a misplaced BN, ReLU or pad fails here."""
    m = fill.fill_state(VoxelEncoder2(LAYERS), seed=2).double().eval()
    occ = random_occ(5, 2, 32) if kind == "random" else face_occ(2, 32)
    with torch.no_grad():
        ref = m(torch.from_numpy(occ).double())
    got = voxenc.encode_cpu(occ, voxenc.params_of(m), storage="exact")
    assert len(got) == 6
    for k, (a, b) in enumerate(zip(got, ref)):
        b = b.numpy()
        assert a.shape == b.shape and a.dtype == np.float64
        err, top = float(np.abs(a - b).max()), float(np.abs(b).max())
        print(f"level {k}: max|restatement - torch fp64| = {err:.3e}, max|level| = {top:.3e}")
        assert top > 0 and err <= 1e-10 * top, (k, err, top)


def test_fp16_restatement_level0_is_the_reference_golden(golden_dir):
    """Level 0 passes through fp32 layers only: the half-precision storage must not show against list_vox0."""
    g = np.load(os.path.join(golden_dir, "models.npz"))
    cfg = arguments.default_config(vox_res=32, train_batch_size=2)
    net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval()
    with torch.no_grad():
        occ = net.encode(torch.from_numpy(synth.uniform(78, (2, 3, 64, 64))))[4]
    levels = voxenc.encode_cpu(occ.numpy(), voxenc.params_of(net.vox_encoder), storage="fp16")
    assert levels[0].dtype == np.float32 and all(v.dtype == np.float16 for v in levels[1:])
    assert [v.shape[1:] for v in levels] == [(1, 32, 32, 32), (16, 32, 32, 32), (32, 16, 16, 16), (64, 8, 8, 8),
                                            (128, 4, 4, 4), (128, 2, 2, 2)]
    err = float(np.abs(levels[0][:, :, ::4, ::4, ::4] - g["list_vox0"]).max())
    print(f"max|level 0 (fp16 restatement) - list_vox0| = {err:.3e}")
    assert err <= 1e-5


def test_header_symbols_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "list_voxenc.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = set(re.findall(r"\b(list_voxenc_\w+)\s*\(", body))
    assert len(declared) >= 5 and "list_voxenc_forward" in declared
    assert declared == set(voxenc.VOXENC_EXPORTS)
    lib = voxenc.load()
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.list_abi_version() == 9
    assert not any(n.startswith("list_voxenc") for n in hip.EXPORTS)


def _closed_weight_bytes(layers):
    al = lambda n: (n + 255) // 256 * 256
    wpk = lambda ci, co: (14 if ci == 16 else ci // 32 * 27) * (co // 16) * 1024
    n = 0
    for l in range(8):
        ci, co = layers[l], layers[l + 1]
        n += al(co * 27 * 4 if ci == 1 else wpk(ci, co)) + al(co * 4) + (2 * al(co * 4) if l < 2 else 0)
        if l >= 3:
            n += al(wpk(co, co)) + 3 * al(co * 4)
    return n


def _closed_workspace_bytes(B, R, layers):
    al = lambda n: (n + 255) // 256 * 256
    n = 2 * al(B * R ** 3 * 4) + al(max(B * (R >> (l - 3)) ** 3 * layers[l + 1] * 2 for l in range(3, 8)))
    return n + sum(al(B * (R >> (l - 2)) ** 3 * layers[l + 1] * 2) for l in range(3, 7))


def test_buffer_sizes_match_their_closed_forms():
    assert voxenc.weight_bytes(LAYERS) == _closed_weight_bytes(LAYERS) == voxenc.weight_bytes_closed_form(LAYERS)
    # the default network: 13 MFMA operands (27 K-steps per 32 input channels, 14 for 16) and 41 small fp32 arrays
    assert voxenc.weight_bytes(LAYERS) == 3538176
    for B, R in ((2, 32), (1, 128), (8, 128)):
        assert voxenc.workspace_bytes(B, R, LAYERS) == _closed_workspace_bytes(B, R, LAYERS) \
            == voxenc.workspace_bytes_closed_form(B, R, LAYERS)
    # B = 1, R = 128: two fp32 volumes (8 MiB each), the 16-channel fp16 activation (64 MiB), four pooled levels
    assert voxenc.workspace_bytes(1, 128, LAYERS) == 2 * 8388608 + 67108864 + 8388608 + 2097152 + 524288 + 131072


def test_refusals_carry_a_message_without_a_gpu():
    lib = voxenc.load()
    arr = (C.c_int32 * 9)(*LAYERS)
    for R, word in ((40, "multiple of 16"), (272, "at most 256")):
        assert lib.list_voxenc_workspace_bytes(1, R, arr, 9) == 0
        assert word in voxenc.last_error()
        with pytest.raises(hip.ListError, match=word):
            voxenc.workspace_bytes(1, R, LAYERS)
    bad = [1, 1, 1, 1, 24, 32, 64, 128, 128]
    assert lib.list_voxenc_weight_bytes((C.c_int32 * 9)(*bad), 9) == 0
    assert "layers[4] = 24" in voxenc.last_error() and "16" in voxenc.last_error()
    with pytest.raises(hip.ListError, match="layers\\[4\\] = 24"):
        voxenc.weight_bytes(bad)
    assert lib.list_voxenc_weight_bytes(arr, 8) == 0 and "n_layers = 8" in voxenc.last_error()
    # NULL pointers are refused on the host, before any HIP call (the other arguments are dummies never dereferenced)
    one = C.c_void_p(256)
    outs = (C.c_void_p * 6)(*[256] * 6)
    rc = lib.list_voxenc_forward(None, 1, 32, arr, 9, one, 1 << 30, one, 1 << 30, outs, None)
    assert rc == hip.ERR_ARG and "occ is NULL" in voxenc.last_error()
    outs[3] = None
    rc = lib.list_voxenc_forward(one, 1, 32, arr, 9, one, 1 << 30, one, 1 << 30, outs, None)
    assert rc == hip.ERR_ARG and "levels_out[3] is NULL" in voxenc.last_error()
    rc = lib.list_voxenc_forward(one, 1, 40, arr, 9, one, 1 << 30, one, 1 << 30, outs, None)
    assert rc == hip.ERR_SHAPE and "R = 40" in voxenc.last_error()
    rc = lib.list_voxenc_prep_weights(None, arr, 9, one, 1 << 30, None)
    assert rc == hip.ERR_ARG and "stages is NULL" in voxenc.last_error()
    outs[3] = 256
    rc = lib.list_voxenc_forward(one, 1, 32, arr, 9, one, 16, one, 1 << 30, outs, None)
    assert rc == hip.ERR_WORKSPACE and "packed holds 16 bytes" in voxenc.last_error()


def test_model_option_defaults_to_torch_and_leaves_the_cpu_alone():
    assert arguments.default_config().vox_encoder == "torch"
    assert arguments.get_args(["--vox_encoder", "hip"]).vox_encoder == "hip"
    LIST = utils.get_class("network.models.LIST")
    with pytest.raises(ValueError, match="vox_encoder"):
        LIST(arguments.default_config(vox_res=32, train_batch_size=2, vox_encoder="triton"))
    base = fill.fill_state(LIST(arguments.default_config(vox_res=32, train_batch_size=2)), seed=2).eval()
    opt = fill.fill_state(LIST(arguments.default_config(vox_res=32, train_batch_size=2, vox_encoder="hip")),
                          seed=2).eval()
    assert opt.vox_encoder_kind == "hip" and base.vox_encoder_kind == "torch"
    assert list(opt.state_dict()) == list(base.state_dict())
    img = torch.from_numpy(synth.uniform(78, (2, 3, 64, 64)))
    with torch.no_grad():
        a, b = base.encode(img), opt.encode(img)
    for x, y in zip(a[1], b[1]):
        assert x.dtype == torch.float32 and torch.equal(x, y)
    assert torch.equal(a[2], b[2]) and torch.equal(a[4], b[4])
    # train() on the CPU: still the torch module, gradients and batch statistics included
    base.train(), opt.train()
    fa, fb = base.encode(img)[1], opt.encode(img)[1]
    for x, y in zip(fa, fb):
        assert y.requires_grad and torch.equal(x, y)


def test_forward_refuses_training_mode_and_gradients():
    m = VoxelEncoder2(LAYERS)
    occ = torch.zeros(1, 32, 32, 32)
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        voxenc.forward(m, occ)
    m.eval()
    with pytest.raises(RuntimeError, match="no backward"):
        voxenc.forward(m, occ)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        voxenc.forward(m, occ)                              # a CPU module: an error, never the torch module
