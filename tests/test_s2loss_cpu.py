"""CPU: the numpy restatement of stage 2's loss (s2loss.*_cpu) against the reference's own SDFLoss record, the executor's
torch expressions and torch autograd; the C ABI of include/list_s2loss.h without a GPU (symbols, refusals before any HIP
call); the --stage2_loss / --occ_dtype options."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from list_amd import arguments, hip, s2loss as S, utils
from list_amd.network import executors
from oracle import dataset_fixture as DF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H  # noqa: E402
from _s2loss_case import case  # noqa: E402


def torch_path(occ, gt, pred, sdf, scale, dtype):
    """LIST.calc_loss as it stands (the default: torch expressions) on CPU tensors of `dtype`."""
    ex = executors.LIST.__new__(executors.LIST)
    ex.stage2_loss, ex.sdf_scale, ex.loss_sdf = "torch", scale, executors.L.SDFLoss(scale)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    return ex.calc_loss((t(occ), t(pred)), (t(gt), t(sdf)))


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_sdf_values_match_the_reference_record(golden_dir):
    """tests/golden/aux.npz holds the reference SDFLoss's own outputs for sdf_scale = 2."""
    a = np.load(os.path.join(golden_dir, "aux.npz"))
    pred, sdf = a["loss_outputs"], a["loss_targets"]
    got = S.stage2_loss_cpu(np.full(4, 0.5, np.float32), np.ones(4, np.float32), pred, sdf, 2.0)
    for k in S.KEYS[1:]:
        np.testing.assert_allclose(got[k], a["loss_" + k], rtol=2e-6)


@pytest.mark.parametrize("n_occ,B,N,scale,soft", [(1, 1, 1, 1.0, False), (4097, 3, 101, 2.0, False),
                                                  (1 << 16, 2, 2000, 1.0, True)])
def test_loss_cpu_is_the_torch_expression_in_float64(n_occ, B, N, scale, soft):
    """Both sides in float64 on float64 inputs: they differ in summation order only, n * 2^-53 at the very worst is below
    1e-12 for these sizes (and every sum is of one sign)."""
    occ, gt, pred, sdf = (a.astype(np.float64) for a in case(n_occ, B, N, seed=n_occ, soft=soft))
    want = torch_path(occ, gt, pred, sdf, scale, torch.float64)
    got = S.stage2_loss_cpu(occ, gt, pred, sdf, scale)
    assert sorted(got) == sorted(want) == sorted(S.KEYS)
    for k in S.KEYS[:3]:
        assert got[k].dtype == np.float64 and want[k].dtype == torch.float64
        np.testing.assert_allclose(got[k], float(want[k]), rtol=1e-12, atol=0)
    # SDFLoss takes the accuracy as the mean of same_side.float(): a float32 whatever the inputs are
    assert want[S.KEYS[3]].dtype == torch.float32 and np.float32(got[S.KEYS[3]]) == float(want[S.KEYS[3]])


def test_loss_cpu_against_the_torch_expression_in_float32():
    """A pairwise float32 sum of 2^21 same-sign terms errs by at most about 21 * 2^-24, plus logf: 1e-5."""
    occ, gt, pred, sdf = case(1 << 21, 4, 5000, seed=5)
    want = torch_path(occ, gt, pred, sdf, 1.0, torch.float32)
    got = S.stage2_loss_cpu(occ, gt, pred, sdf, 1.0)
    for k in S.KEYS:
        np.testing.assert_allclose(got[k], float(want[k]), rtol=1e-5, atol=0)
    dev = S.stage2_loss_cpu(occ, gt, pred, sdf, 1.0, device=True)        # the library's float32 constants and rounding
    for k in S.KEYS:
        assert dev[k].dtype == np.float32
        np.testing.assert_allclose(dev[k], got[k], rtol=1e-6)


def test_saturated_and_invalid_occupancies_behave_as_in_torch():
    one = np.ones((1, 1), np.float32)
    for o, t in ((0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (1.0, 1.0), (1e-9, 1.0)):
        occ, gt = np.array([o], np.float32), np.array([t], np.float32)
        want = float(torch_path(occ, gt, one, one, 1.0, torch.float32)["occ_loss"])
        got = float(S.stage2_loss_cpu(occ, gt, one, one, 1.0)["occ_loss"])
        assert np.isfinite(want) and abs(got - want) <= 1e-6 * abs(want) + 1e-12, (o, t, got, want)
    assert abs(float(S.stage2_loss_cpu([0.0], [1.0], one, one, 1.0)["occ_loss"]) - 900 * -np.log(np.float32(1e-8))) < 1e-3
    for o in (np.nan, -1e-3, 1.001):
        occ = np.array([0.5, o, 0.25], np.float32)
        gt = np.array([1, 0, 1], np.float32)
        assert np.isnan(float(torch_path(occ, gt, one, one, 1.0, torch.float32)["occ_loss"]))
        assert np.isnan(S.stage2_loss_cpu(occ, gt, one, one, 1.0)["occ_loss"])
        g = S.stage2_grad_cpu(occ, gt, one, one, 1.0)[0]
        assert np.isfinite(g[[0, 2]]).all()


@pytest.mark.parametrize("soft", [False, True])
def test_grad_cpu_is_float64_autograd(soft):
    occ, gt, pred, sdf = (a.astype(np.float64) for a in case(5000, 3, 70, seed=21 + soft, soft=soft))
    occ = np.clip(occ, 1e-4, 1 - 1e-4)
    ex = executors.LIST.__new__(executors.LIST)
    ex.stage2_loss, ex.sdf_scale, ex.loss_sdf = "torch", 2.0, executors.L.SDFLoss(2.0)
    to, tp = torch.from_numpy(occ).requires_grad_(), torch.from_numpy(pred).requires_grad_()
    loss = ex.calc_loss((to, tp), (torch.from_numpy(gt), torch.from_numpy(sdf)))
    (3.0 * loss["occ_loss"] + 0.25 * loss["sdf_loss"]).backward()
    g_occ, g_sdf = S.stage2_grad_cpu(occ, gt, pred, sdf, 2.0, grad_out=(3.0, 0.25))
    assert g_occ.shape == occ.shape and g_sdf.shape == pred.shape and g_occ.dtype == np.float64
    np.testing.assert_allclose(g_occ, to.grad.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(g_sdf, tp.grad.numpy(), rtol=1e-12, atol=0)


def test_targets_of_every_dtype_are_the_same_numbers():
    occ, gt, pred, sdf = case(1000, 2, 10, seed=2)
    want = S.stage2_loss_cpu(occ, gt, pred, sdf, 1.0)
    for other in (gt.astype(np.uint8), gt.astype(bool)):
        got = S.stage2_loss_cpu(occ, other, pred, sdf, 1.0)
        assert all(got[k] == want[k] for k in S.KEYS)
        assert np.array_equal(S.stage2_grad_cpu(occ, other, pred, sdf, 1.0)[0], S.stage2_grad_cpu(occ, gt, pred, sdf, 1.0)[0])


def test_the_kernels_logarithm_against_libm_on_the_host(tmp_path):
    """csrc/s2loss_math.h is plain C++: compiled for the host (no contraction into fma beyond the explicit ones, as the
    library is built) and held to libm's log at the 4 float64 ulps its header derives, with libm's non-finite cases."""
    import subprocess
    from _host_cxx import host_cxx
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "s2loss_log_host")
    csrc = os.path.join(root, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")
    subprocess.run([host_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-I", csrc,
                    os.path.join(root, "tests", "csrc", "s2loss_log_host.cpp"), "-o", exe, "-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout
    print(out)
    f = dict(line.split(" ", 1) for line in out.strip().splitlines())
    assert int(f["values"]) > 9_000_000 and float(f["worst_ulps"]) <= 4.0
    assert f["specials"].split() == ["-inf", "-inf", "nan", "nan", "inf", "0"] or \
        f["specials"].split() == ["-inf", "-inf", "-nan", "nan", "inf", "0"]


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return S.load()


def test_header_table_and_library_agree(lib):
    names = H.declared("list_s2loss.h")
    assert names == sorted(S.S2LOSS_EXPORTS) == ["list_s2loss_bwd", "list_s2loss_fwd", "list_s2loss_last_error",
                                                 "list_s2loss_log", "list_s2loss_workspace_bytes"]
    exported = H.exported(hip.LIB_PATH)
    assert {n for n in exported if n.startswith("list_s2loss_")} == set(names)
    assert not set(names) & set(hip.EXPORTS)
    for header, (_, _, prefixes) in H.SECTIONS.items():                 # no other section owns the prefix
        assert not prefixes or not any(n.startswith(prefixes) for n in names), header
    for n in names:
        assert getattr(lib, n) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9


def test_refusals_come_before_any_hip_call(lib):
    fake = 256                                    # never dereferenced: every refusal below is a host check
    ws = lib.list_s2loss_workspace_bytes(8 * 128 ** 3, 8, 20000)
    assert 0 < ws == lib.list_s2loss_workspace_bytes(1, 1, 1) < 1 << 16           # partials only: no per-element scratch
    err = lambda: lib.list_s2loss_last_error().decode()

    def fwd(n_occ=100, B=2, N=50, kind=0, wb=ws, **null):
        p = dict(occ=fake, occ_gt=fake, sdf_pred=fake, sdf_gt=fake, out=fake, workspace=fake)
        p.update(null)
        return lib.list_s2loss_fwd(p["occ"], p["occ_gt"], kind, n_occ, p["sdf_pred"], p["sdf_gt"], B, N, 1.0, 0.9,
                                   p["out"], p["workspace"], wb, None)

    def bwd(n_occ=100, B=2, N=50, kind=0, **null):
        p = dict(occ=fake, occ_gt=fake, sdf_pred=fake, sdf_gt=fake, grad_out=fake, grad_occ=fake, grad_sdf_pred=fake)
        p.update(null)
        return lib.list_s2loss_bwd(p["occ"], p["occ_gt"], kind, n_occ, p["sdf_pred"], p["sdf_gt"], B, N, 1.0, 0.9,
                                   p["grad_out"], p["grad_occ"], p["grad_sdf_pred"], None)

    for call in (fwd, bwd):
        assert call(n_occ=0) == hip.ERR_SHAPE and "n_occ = 0" in err()
        assert call(n_occ=(1 << 36) + 1) == hip.ERR_SHAPE and "2^36" in err()
        assert call(B=1, N=(1 << 36) + 1) == hip.ERR_SHAPE and f"N = {(1 << 36) + 1}" in err()
        assert call(B=1 << 20, N=(1 << 16) + 1) == hip.ERR_SHAPE and "B*N <= 2^36" in err()
        assert call(B=0) == hip.ERR_SHAPE and "B = 0" in err()
        assert call(kind=2) == hip.ERR_SHAPE and "occ_gt_kind = 2" in err()
        for name in ("occ", "occ_gt", "sdf_pred", "sdf_gt"):
            assert call(**{name: None}) == hip.ERR_ARG and f"{name} is NULL" in err()
    assert fwd(out=None) == hip.ERR_ARG and "out is NULL" in err()
    assert fwd(workspace=None) == hip.ERR_ARG and "workspace is NULL" in err()
    assert fwd(wb=ws - 1) == hip.ERR_WORKSPACE and "list_s2loss_workspace_bytes" in err()
    assert bwd(grad_out=None) == hip.ERR_ARG and "grad_out is NULL" in err()
    assert bwd(grad_occ=None, grad_sdf_pred=None) == hip.ERR_ARG and "both NULL" in err()
    assert lib.list_s2loss_log(fake, 0, fake, None) == hip.ERR_SHAPE and "n = 0" in err()
    assert lib.list_s2loss_log(None, 5, fake, None) == hip.ERR_ARG and "x is NULL" in err()
    assert lib.list_s2loss_log(fake, 5, None, None) == hip.ERR_ARG and "out is NULL" in err()
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), ((1 << 36) + 1, 1, 1), (1, 1, (1 << 36) + 1)):
        assert lib.list_s2loss_workspace_bytes(*bad) == 0 and err()
    assert lib.list_s2loss_workspace_bytes(1 << 36, 1 << 18, 1 << 18) == ws       # the largest accepted


def test_a_refused_call_leaves_the_other_sections_text_alone(lib):
    from list_amd import chamfer
    assert chamfer.load().list_chamfer_workspace_bytes(0, 5, 5) == 0
    before = lib.list_loss_last_error()
    assert lib.list_s2loss_workspace_bytes(0, 1, 1) == 0 and b"n_occ" in lib.list_s2loss_last_error()
    assert lib.list_loss_last_error() == before and b"B = 0" in before
    assert "list_s2loss.h" in __import__("list_amd.build", fromlist=["x"]).PUBLIC_HEADERS


# ---- stage2_loss on CPU tensors, and the options ----------------------------------------------------------------------
def test_stage2_loss_refuses_cpu_tensors_and_bad_shapes():
    occ, gt, pred, sdf = (torch.from_numpy(a) for a in case(64, 2, 5))
    with pytest.raises(ValueError, match="stage2_loss_cpu"):
        S.stage2_loss(occ, gt, pred, sdf, 1.0)
    for args in ((occ[:5], gt, pred, sdf), (occ, gt, pred, sdf[:1]), (occ.long(), gt, pred, sdf), (occ[:0], gt[:0], pred, sdf),
                 (occ.numpy(), gt, pred, sdf)):
        with pytest.raises(ValueError):
            S.stage2_loss(*args, 1.0)


def test_options_default_to_torch_and_float32():
    cfg = arguments.default_config()
    assert (cfg.stage2_loss, cfg.occ_dtype) == ("torch", "float32")
    got = arguments.get_args(["--stage2_loss", "hip", "--occ_dtype", "uint8"])
    assert (got.stage2_loss, got.occ_dtype) == ("hip", "uint8")
    for bad in (["--stage2_loss", "triton"], ["--occ_dtype", "bool"]):
        with pytest.raises(SystemExit):
            arguments.get_args(bad)
    with pytest.raises(ValueError, match="stage2_loss"):
        executors.LIST(arguments.default_config(stage2_loss="triton"), None)
    assert executors.LIST(arguments.default_config(stage2_loss="hip"), None).stage2_loss == "hip"


def test_executor_on_cpu_tensors_keeps_the_torch_path_with_either_option():
    """CPU tensors take the torch expressions whatever --stage2_loss says, bit for bit; uint8 and bool targets give what
    their float32 copy gives."""
    occ, gt, pred, sdf = case(4096, 2, 50, seed=8)
    want = torch_path(occ, gt, pred, sdf, 1.0, torch.float32)
    ex = executors.LIST(arguments.default_config(stage2_loss="hip"), None)
    t = torch.from_numpy
    for target in (t(gt), t(gt.astype(np.uint8)), t(gt.astype(bool))):
        o = t(occ).requires_grad_()
        got = ex.calc_loss((o, t(pred)), (target, t(sdf)))
        assert all(torch.equal(got[k], want[k]) for k in S.KEYS)
        got["occ_loss"].backward()
        assert torch.isfinite(o.grad).all()


def test_synthetic_dataset_hands_out_the_occupancy_in_the_configured_dtype():
    kw = dict(vox_res=16, img_res=16, sample_point_density=64, synthetic_len=2)
    f32 = utils.get_class("datasets.Datasets.SyntheticIM2SDF")(arguments.default_config(**kw), "train")[1]["occ"]
    u8 = utils.get_class("datasets.Datasets.SyntheticIM2SDF")(arguments.default_config(occ_dtype="uint8", **kw), "train")[1]["occ"]
    assert f32.dtype == torch.float32 and u8.dtype == torch.uint8 and u8.shape == f32.shape == (1, 16, 16, 16)
    assert torch.equal(u8.float(), f32) and 0 < int(u8.sum()) < u8.numel()
    with pytest.raises(ValueError, match="occ_dtype"):
        utils.get_class("datasets.Datasets.SyntheticIM2SDF")(arguments.default_config(occ_dtype="bool", **kw), "train")


def test_file_dataset_hands_out_the_occupancy_in_the_configured_dtype(tmp_path):
    shape_ids = ["shape_a", "shape_b"]
    image_dir, h5_dir = DF.write_tree(str(tmp_path), shape_ids)
    split = tmp_path / "split"
    split.mkdir()
    (split / f"{DF.CAT}_train.lst").write_text("\n".join(shape_ids) + "\n")
    items = {}
    for name in ("float32", "uint8"):
        cfg = arguments.default_config(cuda=False, split_dir=str(split) + "/", occ_dtype=name,
                                       **DF.config_fields(image_dir, h5_dir))
        random.seed(333)
        ds = utils.get_class("datasets.Datasets.IM2SDF")(cfg, "train")
        assert type(ds).__name__ == "FileIM2SDF" and len(ds) == 2
        items[name] = [ds[i] for i in range(2)]
    for a, b in zip(items["float32"], items["uint8"]):
        assert a["occ"].dtype == torch.float32 and b["occ"].dtype == torch.uint8
        assert a["occ"].shape == b["occ"].shape == (1, DF.VOX_RES, DF.VOX_RES, DF.VOX_RES)
        assert torch.equal(b["occ"].float(), a["occ"]) and 0 < int(b["occ"].sum()) < b["occ"].numel()
        assert torch.equal(a["points"], b["points"]) and a["values"].dtype == b["values"].dtype == torch.float32
