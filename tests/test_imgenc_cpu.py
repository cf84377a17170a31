"""CPU: the numpy restatement of the HIP image encoder (imgenc.encode_cpu) against the torch ResEncoder, the C ABI of
include/list_imgenc.h without a GPU (exports, sizes, refusals), the model option, and the per-launch checker on itself."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fill, synth
from list_amd import arguments, hip, imgenc, utils
from list_amd.network.modules import ResEncoder

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H  # noqa: E402
import _imgenc_check as ic  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


@pytest.fixture(scope="module")
def encoder():
    m = fill.fill_state(ResEncoder(), seed=3).eval()
    return m, imgenc.params_of(m)


def image(seed, B, H, W):
    return synth.uniform(seed, (B, 3, H, W)).astype(np.float32)


# ---- restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 32, 48), (1, 64, 64)])
def test_exact_restatement_is_the_torch_module_in_float64(encoder, shape):
    """float64 restatement against ResEncoder.double().eval(): <= 1e-10 of each tensor's maximum (both sides are float64
    and differ in summation order only).  fill_state gives non-trivial BN statistics, so a misplaced BN, ReLU, pad,
    stride phase or identity fails here."""
    m, params = encoder
    img = image(7, *shape)
    with torch.no_grad():
        vec, levels = copy.deepcopy(m).double()(torch.from_numpy(img).double())
    got = imgenc.encode_cpu(params, img, arithmetic="exact")
    assert len(got["levels"]) == 5 and got["vec"].dtype == np.float64
    for name, a, b in [("vec", got["vec"], vec.numpy())] + [(f"f{k}", a, b.numpy()) for k, (a, b) in
                                                          enumerate(zip(got["levels"], levels))]:
        assert a.shape == b.shape and a.dtype == np.float64
        err, top = float(np.abs(a - b).max()), float(np.abs(b).max())
        print(f"{shape} {name}: max|restatement - torch fp64| = {err:.3e}, max|tensor| = {top:.3e}")
        assert top > 0 and err <= 1e-10 * top, (name, err, top)
    B, Hh, Ww = shape
    assert [v.shape for v in got["levels"]] == [(B, c, Hh >> k, Ww >> k) for k, c in enumerate(imgenc.LEVEL_CHANNELS)]


def test_composed_head_is_the_uncomposed_one_in_float64(encoder):
    """fc and fc1 have no nonlinearity between them: one [128,512] float64 matrix and one bias equal the two Linears to
    1e-12 of the largest |vec|."""
    _, params = encoder
    st = params["state"]
    mean = np.abs(synth.uniform(9, (5, 512))).astype(np.float64) * 3
    w0, b0 = st["fc.weight"].astype(np.float64), st["fc.bias"].astype(np.float64)
    w1, b1 = st["fc1.weight"].astype(np.float64), st["fc1.bias"].astype(np.float64)
    two = (mean @ w0.T + b0) @ w1.T + b1
    wc, bc = imgenc.compose_head(st, np.float64)
    one = mean @ wc.T + bc
    err, top = float(np.abs(one - two).max()), float(np.abs(two).max())
    print(f"max|composed - uncomposed| = {err:.3e}, max|vec| = {top:.3e}")
    assert wc.shape == (128, 512) and top > 0 and err <= 1e-12 * top
    w32, b32 = imgenc.compose_head(st)
    assert w32.dtype == np.float32 and np.abs(w32 - wc).max() <= 2.0 ** -24 * np.abs(wc).max()


@pytest.mark.parametrize("shape", [(1, 32, 48)])
def test_fp32_device_arithmetic_stays_within_the_derived_bound_of_exact(encoder, shape):
    """The device's graph without the fp16 roundings (storage="fp32") against float64, tensor by tensor and element by
    element, within the forward error bound ic.fp32_graph_bound derives -- nothing measured goes into it."""
    _, params = encoder
    img = image(7, *shape)
    ex = imgenc.encode_cpu(params, img, arithmetic="exact")
    dv = imgenc.encode_cpu(params, img, arithmetic="device", storage="fp32")
    bound = ic.fp32_graph_bound(params, img)
    assert dv["vec"].dtype == np.float32 and dv["layer2_0_down"].dtype == np.float32
    for name in imgenc.step_names()[:-1] + ["vec"]:
        q = np.abs(dv[name].astype(np.float64) - ex[name]) / np.maximum(bound[name], 1e-300)
        print(f"{name:15s} max error / bound = {q.max():.3f}   (bound up to {bound[name].max():.2e})")
        assert q.max() <= 1.0, name
    # ... and the bound is not slack where it starts: the fp16 copy of the stem's output (half an ulp, 2^-12 relative,
    # against 150 roundings of 2^-24) already leaves it.  Further down it is a worst case that grows with every layer
    # (each convolution multiplies an input error by up to sum |w| |s|), which is why the device is judged launch by launch
    dh = imgenc.encode_cpu(params, img, arithmetic="device", storage="fp16")
    assert dh["stem"].dtype == np.float16 and dh["levels"][0].dtype == np.float32
    q = np.abs(dh["stem"].astype(np.float64) - ex["stem"]) / bound["stem"]
    assert q.max() > 1.0


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------
TABLE = ["list_imgenc_forward", "list_imgenc_forward_steps", "list_imgenc_last_error", "list_imgenc_n_steps",
         "list_imgenc_prep_weights", "list_imgenc_weight_bytes", "list_imgenc_workspace_bytes"]


def test_header_table_and_library_agree():
    names = H.declared("list_imgenc.h")
    assert names == TABLE == sorted(imgenc.IMGENC_EXPORTS)
    lib = imgenc.load()
    exported = H.exported(hip.LIB_PATH)
    assert {n for n in exported if n.startswith("list_imgenc_")} == set(names)
    assert not set(names) & set(hip.EXPORTS)
    for n in names:
        assert getattr(lib, n) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9


def test_n_steps_is_the_length_of_step_names():
    names = imgenc.step_names()
    assert imgenc.n_steps() == len(names) == 22 and len(set(names)) == 22
    assert names[0] == "stem" and names[1] == "pool" and names[-1] == "head"
    assert sum(n.endswith("_down") for n in names) == 3 and len(imgenc.CONV_STEPS) == imgenc.N_CONVS == 20


def _closed_workspace(B, Hh, Ww):
    al = lambda n: (n + 255) // 256 * 256
    n = al(B * Hh * Ww * 64 * 2) + 5 * al(B * (Hh // 2) * (Ww // 2) * 64 * 2)
    for L, c in ((2, 128), (3, 256), (4, 512)):
        n += 5 * al(B * (Hh >> L) * (Ww >> L) * c * 2)
    return n


def test_buffer_sizes_match_their_closed_forms():
    al = lambda n: (n + 255) // 256 * 256
    convs = [(64, 64, 3)] * 4
    for c in (64, 128, 256):
        convs += [(c, 2 * c, 3), (c, 2 * c, 1)] + [(2 * c, 2 * c, 3)] * 3
    w = al(147 * 64 * 4) + 2 * al(256) + sum(al(ci * k * k * co * 2) + 2 * al(co * 4) for ci, co, k in convs)
    w += al(512 * 128 * 4) + al(512)
    assert imgenc.weight_bytes() == imgenc.weight_bytes_closed_form() == w
    for B, Hh, Ww in ((1, 32, 32), (1, 32, 48), (3, 64, 80), (2, 96, 96), (1, 224, 224), (8, 224, 224), (1, 512, 512)):
        assert imgenc.workspace_bytes(B, Hh, Ww) == imgenc.workspace_bytes_closed_form(B, Hh, Ww) \
            == _closed_workspace(B, Hh, Ww) > 0


def _io(B=1, Hh=32, Ww=48):
    io = imgenc._IO()
    io.B, io.H, io.W = B, Hh, Ww
    io.img_sb, io.img_sc, io.img_sh, io.img_sw = 3 * Hh * Ww, Hh * Ww, Ww, 1
    for name in ("img", "packed", "workspace", "vec"):
        setattr(io, name, 256)
    for k in range(5):
        io.levels_out[k] = 256
    io.packed_bytes = io.workspace_bytes = 1 << 40
    return io


def _clone(io):
    out = imgenc._IO()
    C.memmove(C.byref(out), C.byref(io), C.sizeof(io))
    return out


def test_refusals_carry_a_message_without_a_gpu():
    """Everything here is refused on the host, before any HIP call: the dummy pointers are never dereferenced."""
    lib = imgenc.load()
    for B, Hh, Ww, word in ((1, 40, 64, "H = 40: must be a multiple of 16"), (1, 16, 64, "H = 16: must be in \\[32, 512\\]"),
                            (1, 64, 528, "W = 528: must be in \\[32, 512\\]"), (0, 64, 64, "B = 0")):
        assert lib.list_imgenc_workspace_bytes(B, Hh, Ww) == 0
        with pytest.raises(hip.ListError, match=word):
            imgenc.workspace_bytes(B, Hh, Ww)
        bad = _io(max(B, 0), Hh, Ww)
        bad.B = B
        assert lib.list_imgenc_forward(C.byref(bad), None) == hip.ERR_SHAPE
        assert word.replace("\\", "") in imgenc.last_error()
    io = _io()
    assert lib.list_imgenc_forward(None, None) == hip.ERR_ARG and "io is NULL" in imgenc.last_error()
    for name in ("img", "packed", "workspace", "vec"):
        bad = _clone(io)
        setattr(bad, name, None)
        assert lib.list_imgenc_forward(C.byref(bad), None) == hip.ERR_ARG and f"{name} is NULL" in imgenc.last_error()
    bad = _clone(io)
    bad.levels_out[3] = None
    assert lib.list_imgenc_forward(C.byref(bad), None) == hip.ERR_ARG and "levels_out[3] is NULL" in imgenc.last_error()
    bad.levels_out[3] = 264
    assert lib.list_imgenc_forward(C.byref(bad), None) == hip.ERR_ARG
    assert "levels_out[3] is not 16-byte aligned" in imgenc.last_error()
    bad = _clone(io)
    bad.workspace = 258
    assert lib.list_imgenc_forward(C.byref(bad), None) == hip.ERR_ARG
    assert "workspace is not 16-byte aligned" in imgenc.last_error()
    bad = _clone(io)
    bad.workspace_bytes = imgenc.workspace_bytes(1, 32, 48) - 1
    assert lib.list_imgenc_forward(C.byref(bad), None) == hip.ERR_WORKSPACE
    assert "list_imgenc_workspace_bytes" in imgenc.last_error()
    bad = _clone(io)
    bad.packed_bytes = 16
    assert lib.list_imgenc_forward(C.byref(bad), None) == hip.ERR_WORKSPACE
    assert "packed holds 16 bytes" in imgenc.last_error()
    for b, e in ((5, 3), (-1, 4), (3, 23)):
        assert lib.list_imgenc_forward_steps(C.byref(io), b, e, None) == hip.ERR_ARG
        assert f"steps [{b}, {e})" in imgenc.last_error()
    assert lib.list_imgenc_prep_weights(None, 256, 1 << 30, None) == hip.ERR_ARG and "params is NULL" in imgenc.last_error()
    p = imgenc._Params()
    assert lib.list_imgenc_prep_weights(C.byref(p), 256, 16, None) == hip.ERR_WORKSPACE
    assert lib.list_imgenc_prep_weights(C.byref(p), 256, 1 << 30, None) == hip.ERR_ARG
    assert "conv[0].w is NULL" in imgenc.last_error()


# ---- the model option ------------------------------------------------------------------------------------------------
def test_model_option_defaults_to_torch_and_leaves_the_cpu_alone():
    assert arguments.default_config().img_encoder == "torch"
    assert arguments.get_args(["--img_encoder", "hip"]).img_encoder == "hip"
    with pytest.raises(SystemExit):
        arguments.get_args(["--img_encoder", "triton"])
    LIST, CoarseNet = utils.get_class("network.models.LIST"), utils.get_class("network.models.CoarseNet")
    for cls in (LIST, CoarseNet):
        with pytest.raises(ValueError, match="img_encoder"):
            cls(arguments.default_config(vox_res=32, train_batch_size=2, img_encoder="triton"))
    base = fill.fill_state(LIST(arguments.default_config(vox_res=32, train_batch_size=2)), seed=2).eval()
    opt = fill.fill_state(LIST(arguments.default_config(vox_res=32, train_batch_size=2, img_encoder="hip")), seed=2).eval()
    assert (base.img_encoder_kind, opt.img_encoder_kind) == ("torch", "hip")
    assert list(opt.state_dict()) == list(base.state_dict())
    img = torch.from_numpy(synth.uniform(78, (2, 3, 64, 64)))
    with torch.no_grad():                                              # tensors on the CPU: the torch modules, bit for bit
        a, b = base.encode(img), opt.encode(img)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x, y)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    cb = fill.fill_state(CoarseNet(arguments.default_config(vox_res=32, train_batch_size=2)), seed=1).eval()
    co = fill.fill_state(CoarseNet(arguments.default_config(vox_res=32, train_batch_size=2, img_encoder="hip")), seed=1).eval()
    with torch.no_grad():
        assert torch.equal(cb(img), co(img))
    opt.train()                                                        # train() on the CPU: still the torch module
    assert opt.encode(img)[0][0].requires_grad


def test_forward_refuses_training_mode_gradients_and_a_cpu_module():
    m = ResEncoder()
    img = torch.zeros(1, 3, 32, 32)
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        imgenc.forward(m, img)
    m.eval()
    with pytest.raises(RuntimeError, match="no backward"):
        imgenc.forward(m, img)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        imgenc.forward(m, img)                              # a CPU module: an error, never the torch module


# ---- the per-launch check (tests/_imgenc_check.py) has teeth ---------------------------------------------------------
@pytest.fixture(scope="module")
def emulated(encoder):
    """The device's arithmetic launch by launch at 32 x 80 (levels 16 x 40 -- a partial tile along x --, 8 x 20, 4 x 10,
    2 x 5), computed once."""
    _, params = encoder
    img = image(11, 1, 32, 80)
    Ls = ic.launches(params)
    return params, img, Ls, ic.run_emulated(Ls, img)


def test_chained_emulation_is_the_restatement_and_passes_its_own_check(emulated):
    params, img, Ls, run = emulated
    ref = imgenc.encode_cpu(params, img, arithmetic="device", storage="fp16")
    for L, (x, idt, act, level) in zip(Ls, run):
        assert np.array_equal(act, ref[L.name if L.kind != "head" else "vec"], equal_nan=True), L.name
        if level is not None:
            assert np.array_equal(np.moveaxis(level, 3, 1), ref["levels"][L.step.level]), L.name
        q = ic.check(L, x, idt, act=act, level=level)
        print(f"{L.name:15s} the device's arithmetic restated: max error / bound = {q:.3f}")
        assert q <= 1.0, (L.name, q)


def _with(L, **kw):
    M = copy.copy(L)
    for k, v in kw.items():
        setattr(M, k, v)
    return M


def _fault_tap(L, x, idt, act, level):
    """One tap (ky, kx) = (1, 0) dropped for all channels."""
    w = L.w.copy()
    w[:, :, 1, 0] = 0
    return ic.emulate(_with(L, w=w), x, idt)


def _fault_phase(L, x, idt, act, level):
    """A stride-2 launch reads x[2i + 1, 2j + 1] where x[2i, 2j] is meant."""
    xs = np.zeros_like(x)
    xs[:, :-1, :-1] = x[:, 1:, 1:]
    return ic.emulate(L, xs, idt)


def _fault_no_identity(L, x, idt, act, level):
    return ic.emulate(L, x, np.zeros_like(idt))


def _fault_identity_before_downsample(L, x, idt, act, level, block_input=None):
    """The first block of layers 2 .. 4 adds its INPUT at the stride-2 positions (channels repeated to the new width) in
    place of the downsample's output."""
    wrong = np.concatenate([block_input[:, ::2, ::2]] * 2, axis=3)
    assert wrong.shape == idt.shape
    return ic.emulate(L, x, wrong)


def _fault_shift(L, x, idt, act, level):
    """BN shift set to zero in the weakest channel: the one with the smallest largest output (a channel the ReLU leaves all
    zero shows no shift and is passed over)."""
    top = np.abs(act.astype(np.float64)).max(axis=(0, 1, 2))
    c = int(np.argmin(top + ((L.t == 0) | (top == 0)) * 1e30))
    t = L.t.copy()
    t[c] = 0
    return ic.emulate(_with(L, t=t), x, idt)


def _fault_replicate(L, x, idt, act, level):
    """Replicate padding in place of zeros."""
    p = L.step.ks // 2
    return ic.emulate(L, np.pad(np.asarray(x, np.float64), ((0, 0), (p, p), (p, p), (0, 0)), mode="edge"), idt, pad=0)


def _fault_tiles(L, x, idt, act, level):
    """Output channels 0 .. 15 and 16 .. 31 swapped."""
    outs = []
    for y in (act, level):
        if y is not None:
            y = y.copy()
            y[..., 0:16], y[..., 16:32] = y[..., 16:32].copy(), y[..., 0:16].copy()
        outs.append(y)
    return tuple(outs)


def _fault_partial_tile(L, x, idt, act, level):
    """The last, partial tile along x never written: a sentinel stays."""
    Wd = act.shape[2]
    assert Wd % 16 != 0
    outs = []
    for y in (act, level):
        if y is not None:
            y = y.copy()
            y[:, :, Wd // 16 * 16:] = 1234.0
        outs.append(y)
    return tuple(outs)


def _fault_bf16(L, x, idt, act, level):
    """Weights rounded to bf16 instead of fp16."""
    w = torch.from_numpy(L.w32.astype(np.float32)).bfloat16().double().numpy()
    return ic.emulate(_with(L, w=w), x, idt)


_FAULTS = [(_fault_tap, ("layer1_0_conv1", "layer2_0_conv1", "layer3_1_conv2")),
           (_fault_phase, ("layer2_0_conv1", "layer2_0_down", "layer4_0_down")),
           (_fault_no_identity, ("layer1_0_conv2", "layer2_0_conv2", "layer4_1_conv2")),
           (_fault_identity_before_downsample, ("layer2_0_conv2", "layer3_0_conv2")),
           (_fault_shift, ("stem", "layer1_1_conv1", "layer2_0_down", "layer3_0_conv2")),
           (_fault_replicate, ("stem", "layer1_0_conv1", "layer2_0_conv1", "layer3_1_conv1")),
           (_fault_tiles, ("layer1_1_conv2", "layer2_0_down", "layer4_1_conv2")),
           (_fault_partial_tile, ("layer1_0_conv1", "layer1_1_conv2", "layer2_0_conv1", "layer3_1_conv2")),
           (_fault_bf16, ("layer1_1_conv2",))]


def test_per_launch_check_rejects_wrong_layers(emulated):
    """Each deliberately wrong launch is rejected (largest error / bound > 1) on the activations the right pipeline
    produces.

    What the check cannot see, written down: (1) the max-pool's pad value.  Its input is the stem's ReLU output, never
    negative, so padding with 0 gives the same maxima as padding with -inf (shown below; it differs only on an input
    with negative values, which the device never feeds it).  (2) A single wrong product among the K = 4608 of a
    512-channel layer moves z by about A / K = 2e-4 A, the size of the accumulation term (K + 2) 2^-23 A; and where |y|
    is not small the fp16 storage term 2^-11 |y| hides differences of that size too.  bf16 weights move z by about
    2^-9 A / sqrt(3 K), which at K = 4608 passes for the same reason: that fault is looked for where it can be seen,
    on the fp32 level of a 64-channel layer (K = 576, no storage term)."""
    params, img, Ls, run = emulated
    by_name = {L.name: i for i, L in enumerate(Ls)}
    for fault, names in _FAULTS:
        for name in names:
            i = by_name[name]
            L, (x, idt, act, level) = Ls[i], run[i]
            kw = {}
            if fault is _fault_identity_before_downsample:
                kw["block_input"] = run[L.step.idt][0]                      # the downsample launch's own input
            bad_act, bad_level = fault(L, x, idt, act, level, **kw)
            if fault is _fault_bf16:
                bad_act = None                                              # judged on the fp32 level
            q = ic.check(L, x, idt, act=bad_act, level=bad_level)
            print(f"{fault.__name__:34s} at {name:15s}: max error / bound = {q:.3g}")
            assert q > 1.0, (fault.__name__, name, q)
    # (1): zero padding of the pool is invisible behind the ReLU, visible on a signed input
    pool, f0 = Ls[1], run[1][0]

    def pool_zero_pad(v):
        H2, W2 = v.shape[1], v.shape[2]
        vp = np.pad(v, ((0, 0), (1, 1), (1, 1), (0, 0)))
        return np.max([vp[:, dy:dy + H2 - 1:2, dx:dx + W2 - 1:2] for dy in range(3) for dx in range(3)], axis=0)
    assert (f0 >= 0).all() and ic.check(pool, f0, act=pool_zero_pad(f0)) == 0.0
    assert ic.check(pool, f0 - np.float16(1.0), act=pool_zero_pad(f0 - np.float16(1.0))) == np.inf


def test_per_launch_check_compares_non_finite_values_by_class(emulated):
    params, img, Ls, run = emulated
    L = Ls[2]                                                                # layer1_0_conv1
    x = run[2][0][:, :8, :8].copy()
    x[0, 1, 1, 3], x[0, 6, 6, 5] = np.nan, np.inf
    act, _ = ic.emulate(L, x)
    assert np.isnan(act[0, 0:3, 0:3]).all() and not np.isnan(act[0, 4:, 4:]).any() and np.isinf(act[0, 5:, 5:]).any()
    assert ic.check(L, x, act=act) <= 1.0
    for bad in (np.float16(1.0), np.float16(np.inf)):
        z = act.copy()
        z[0, 1, 1, 0] = bad                                                  # a NaN lost
        assert ic.check(L, x, act=z) == np.inf
    z = act.copy()
    z[np.isinf(act)] = np.float16(65504)                                     # an infinity saturated
    assert ic.check(L, x, act=z) == np.inf
    z = act.copy()
    z[0, 7, 0, 0] = np.nan                                                   # a NaN from nowhere
    assert ic.check(L, x, act=z) == np.inf
    # the pool: a NaN wins, and an fp16 overflow of the storage rounding is accepted only where the bound reaches 65520
    p = run[1][0][:, :8, :8].copy()
    p[0, 3, 3, 2] = np.nan
    out, _ = ic.emulate(Ls[1], p)
    assert np.isnan(out[0, 1:3, 1:3, 2]).all() and ic.check(Ls[1], p, act=out) == 0.0
