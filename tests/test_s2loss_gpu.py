"""GPU: stage 2's loss in HIP (include/list_s2loss.h, s2loss.stage2_loss) against its numpy restatement on the device's own
inputs, against the torch expressions and float64 autograd, and through executors.LIST.calc_loss.

Bounds.  Every sum behind a loss value is of one sign, so the float64 error of the sums (n * 2^-53 at worst) and of log
(an ulp of float64) is invisible after the rounding to float32: the four values are within 2 float32 ulps of the
restatement (one for a rounding that falls the other way, one to spare), the accuracy -- an integer count over B*N --
exactly equal.  A gradient element is one float64 expression rounded once: within 1 ulp.  Non-finite values are equal
as non-finite."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _s2loss_case import case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = 0.9


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()


def _S():
    from list_amd import s2loss
    return s2loss


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ordered(a):
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(got, want):
    """Largest distance in float32 ulps; inf where a non-finite value is not matched by the same non-finite value."""
    got, want = np.atleast_1d(np.asarray(got, np.float32)), np.atleast_1d(np.asarray(want, np.float32))
    assert got.shape == want.shape
    fin = np.isfinite(got) & np.isfinite(want)
    other = ~fin
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want)))
    if not same[other].all():
        return np.inf
    return float(np.abs(_ordered(got[fin]) - _ordered(want[fin])).max()) if fin.any() else 0.0


def run(occ, gt, pred, sdf, scale, grad_out=(1.0, 1.0), want_occ=True, want_sdf=True):
    """Device tensors (views included: they are read where they lie) -> ([4] values, grad_occ, grad_sdf_pred) as numpy."""
    S = _S()
    o = occ.detach().requires_grad_(want_occ)
    p = pred.detach().requires_grad_(want_sdf)
    out = S.stage2_loss(o, gt, p, sdf, scale, W)
    (grad_out[0] * out["occ_loss"] + grad_out[1] * out["sdf_loss"]).backward()
    vals = np.array([float(out[k].detach()) for k in S.KEYS], np.float32)
    return vals, (o.grad.cpu().numpy() if want_occ else None), (p.grad.cpu().numpy() if want_sdf else None)


def check(occ, gt, pred, sdf, scale=1.0, grad_out=(1.0, 1.0), label=""):
    """One forward and backward on device tensors against the restatement on their host copies, at the module's bounds."""
    S = _S()
    vals, g_occ, g_sdf = run(occ, gt, pred, sdf, scale, grad_out)
    host = [t.cpu().numpy() for t in (occ, gt, pred, sdf)]
    want = S.stage2_loss_cpu(*host, scale, W, device=True)
    w_occ, w_sdf = S.stage2_grad_cpu(*host, scale, W, grad_out=grad_out, device=True)
    d = [ulps(vals[i], want[k]) for i, k in enumerate(S.KEYS)]
    dg = ulps(g_occ, w_occ), ulps(g_sdf, w_sdf)
    print(f"{label}: values {vals}, ulps from the restatement {d}; gradients {dg}")
    assert max(d[:3]) <= 2 and d[3] == 0, (label, d, vals, want)
    assert dg[0] <= 1 and dg[1] <= 1, (label, dg)
    return vals, g_occ, g_sdf


GRID = 1024 * 256 * 4            # elements the occupancy grid covers with one item per lane (s2loss.grid_elements())
SWEEP = 4 * GRID                 # ... and with the four items a lane keeps in flight: one pass of the main loop
SDF_SWEEP = 4 * 64 * 256 * 4     # the same for the 64 workgroups of the SDF sums

# (n_occ, B x N).  n_occ: below and around one workgroup; B = 2 at R = 16; one item per lane of the fixed grid + 3 and two
# + 5 (the one-item loop alone, once and twice); R = 128 at B = 1; one pass of the main loop + 7 (main loop, then one more
# item for lane 0 and a tail of 3); two and a half passes + 5 (main loop twice, the one-item loop twice, one more item and
# a tail of 1).  B x N: one element, the golden's shape, an odd shape of the one-item loop, one pass of the SDF main loop + 7.
SHAPES = [(1, (1, 1)), (3, (2, 50)), (255, (3, 1001)), (257, (1, 1)), (2 * 16 ** 3, (2, 50)), (GRID + 3, (3, 1001)),
          (2 * GRID + 5, (1, 1)), (128 ** 3, (2, 50)), (SWEEP + 7, (1, SDF_SWEEP + 7)), (2 * SWEEP + 2 * GRID + 5, (3, 1001))]


def test_the_shapes_mean_what_they_say():
    S = _S()
    assert GRID == S.grid_elements() and SWEEP == S.sweep_elements() and SDF_SWEEP == S.sweep_elements(S.SDF_GROUPS)
    assert S.IN_FLIGHT == 4 and max(n for n, _ in SHAPES[:8]) < SWEEP < SHAPES[8][0] and 2 * SWEEP < SHAPES[9][0]


@pytest.mark.parametrize("i", range(len(SHAPES)))
@pytest.mark.parametrize("kind", ["float32", "uint8"])
def test_values_and_gradients_against_the_restatement(i, kind):
    n, (B, N) = SHAPES[i]
    occ, gt, pred, sdf = case(n, B, N, seed=100 + i)
    check(_t(occ), _t(gt.astype(kind)), _t(pred), _t(sdf), scale=2.0 if i % 2 else 1.0, grad_out=(1.0, 1.0 + i),
          label=f"n_occ = {n}, {B} x {N}, {kind}")


def test_golden_sdf_record_on_the_device(golden_dir):
    import os
    a = np.load(os.path.join(golden_dir, "aux.npz"))
    occ, gt, _, _ = case(100, 1, 1, seed=1)
    vals, _, _ = check(_t(occ), _t(gt), _t(a["loss_outputs"]), _t(a["loss_targets"]), scale=2.0, label="golden 2 x 50")
    assert a["loss_outputs"].shape == (2, 50)
    for i, k in enumerate(_S().KEYS[1:], 1):
        np.testing.assert_allclose(vals[i], a["loss_" + k], rtol=2e-6)


@pytest.mark.parametrize("kind", ["float32", "uint8"])
@pytest.mark.parametrize("n", [2, 7, 1030, 70001, SWEEP + 7])
def test_buffers_entered_one_element_past_an_aligned_base(kind, n):
    """buf[1:]: every pointer 4 bytes (uint8 target: 1 byte) past a 256-byte boundary -- three head elements, then the
    vector path, and a tail (the largest n runs the main loop of both forward kernels that way); the gradient goes to
    a fresh (aligned) buffer, so the backward's cut differs from the forward's
    (test_backward_into_gradient_views_one_element_past_an_aligned_base is the backward's own).  The same numbers entered at the aligned base give the same gradients and, to the bounds, values."""
    occ, gt, pred, sdf = case(n + 1, 1, n + 1, seed=n)
    d_occ, d_gt, d_pred, d_sdf = _t(occ), _t(gt.astype(kind)), _t(pred.reshape(-1)), _t(sdf.reshape(-1))
    assert d_occ.data_ptr() % 256 == 0 and d_gt.data_ptr() % 256 == 0
    views = d_occ[1:], d_gt[1:], d_pred[1:].view(1, n), d_sdf[1:].view(1, n)
    assert views[0].data_ptr() % 16 == 4 and views[1].data_ptr() % 16 == (4 if kind == "float32" else 1)
    v1, g1, s1 = check(*views, label=f"buf[1:], n = {n}, {kind}")
    v2, g2, s2 = check(*(v.clone() for v in views), label=f"the same at an aligned base, n = {n}, {kind}")
    assert np.array_equal(g1, g2) and np.array_equal(s1, s2) and ulps(v1, v2) <= 2
    # only the target off its phase (occ aligned): the element-wise path
    v3, g3, _ = check(views[0].clone(), views[1], views[2], views[3], label=f"target alone off its phase, n = {n}, {kind}")
    assert np.array_equal(g3, g1) and ulps(v3, v1) <= 2


def test_saturated_tiny_and_soft_values():
    """occ exactly 0 and exactly 1 against both targets, 1e-9, soft targets; SDF values exactly at the 0.5 threshold."""
    occ, gt, pred, sdf = case(1000, 3, 1001, seed=4, soft=True)
    occ[:9] = [0, 0, 1, 1, 1e-9, 1e-9, 0.3, 0, 1]
    gt[:9] = [0, 1, 0, 1, 0, 1, 0.3, 0.3, 0.3]
    pred[0, :4], sdf[0, :4] = [0.5, 0.5, 0.6, 0.4], [0.5, 0.6, 0.5, 0.5]
    vals, g_occ, _ = check(_t(occ), _t(gt), _t(pred), _t(sdf), label="saturated, tiny, soft")
    assert np.isfinite(vals).all() and np.isfinite(g_occ).all()
    assert abs(g_occ[1] / (-0.9 / 1e-8) - 1) < 1e-6 and abs(g_occ[2] / (0.1 / 1e-8) - 1) < 1e-6       # 1000 / n = 1
    # the same with 0 / 1 targets as float32, uint8 and bool: the same bits
    hard = (gt > 0.5)
    ref = run(_t(occ), _t(hard.astype(np.float32)), _t(pred), _t(sdf), 1.0)
    for other in (hard.astype(np.uint8), hard):
        got = run(_t(occ), _t(other), _t(pred), _t(sdf), 1.0)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("bad", [np.nan, -1e-3])
@pytest.mark.parametrize("n,at", [(5000, 4321), (7, 0)])
def test_one_invalid_element_gives_a_nan_loss_and_one_nan_gradient(bad, n, at):
    occ, gt, pred, sdf = case(n, 2, 50, seed=9)
    occ[at], gt[at] = bad, 1.0
    vals, g_occ, g_sdf = check(_t(occ), _t(gt), _t(pred), _t(sdf), label=f"occ[{at}] = {bad}")
    assert np.isnan(vals[0]) and np.isfinite(vals[1:]).all() and np.isfinite(g_sdf).all()
    if np.isnan(bad):
        assert np.isnan(g_occ[at]) and np.isfinite(np.delete(g_occ, at)).all()
    else:                                            # log of a negative number is NaN; its derivative 1 / a is finite
        assert np.isfinite(g_occ).all()
    with torch.no_grad():                            # ... as the torch expression has it
        o, t = _t(occ), _t(gt)
        ref = 1000 * (-W * torch.mean(t * torch.log(o + 1e-8)) - (1 - W) * torch.mean((1 - t) * torch.log(1 - o + 1e-8)))
    assert torch.isnan(ref)


def test_two_calls_give_the_same_bits():
    occ, gt, pred, sdf = case(SWEEP + 77, 1, SDF_SWEEP + 77, seed=12)
    args = _t(occ), _t(gt), _t(pred), _t(sdf)
    a, b = run(*args, 1.0, (3.0, 0.5)), run(*args, 1.0, (3.0, 0.5))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.isfinite(a[0]).all()


def test_against_the_torch_expressions_and_float64_autograd():
    """Losses: the float32 torch path on the GPU at rtol 1e-5 (its own pairwise float32 sums and logf).  Gradients: per
    element against autograd of the same expressions in float64 -- what the torch path approximates.  With 0 / 1 targets
    a gradient element is one quotient, and the device differs from float64 by: the float32 formation of a (one rounding)
    or b (two), 2 * 2^-24; the final rounding, 2^-24; and w, which the C ABI takes as a float32: |float32(0.9) - 0.9| is at
    most half an ulp of 0.9, 2^-25, which is 2^-25 / 0.1 < 5 * 2^-24 of the factor 1 - w.  Together 8 * 2^-24."""
    from list_amd.network import executors
    occ, gt, pred, sdf = case(2 * 16 ** 3, 2, 50, seed=31)
    occ = occ.reshape(2, 1, 16, 16, 16)
    gt = gt.reshape(occ.shape)
    ex = executors.LIST.__new__(executors.LIST)
    ex.stage2_loss, ex.sdf_scale, ex.loss_sdf = "torch", 2.0, executors.L.SDFLoss(2.0)
    S = _S()
    vals, g_occ, g_sdf = run(_t(occ), _t(gt), _t(pred), _t(sdf), 2.0, (2.0, 1.0))
    ref32 = ex.calc_loss((_t(occ), _t(pred)), (_t(gt), _t(sdf)))
    for i, k in enumerate(S.KEYS):
        print(k, vals[i], float(ref32[k]))
        np.testing.assert_allclose(vals[i], float(ref32[k]), rtol=1e-5, atol=0)
    o64, p64 = _t(occ).double().requires_grad_(), _t(pred).double().requires_grad_()
    ref64 = ex.calc_loss((o64, p64), (_t(gt).double(), _t(sdf).double()))
    (2.0 * ref64["occ_loss"] + ref64["sdf_loss"]).backward()
    for got, want in ((g_occ, o64.grad), (g_sdf, p64.grad)):
        want = want.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want) / np.abs(want)
        print("largest relative gradient error against float64 autograd:", err.max())
        assert got.shape == want.shape and err.max() <= 8 * 2.0 ** -24


def test_autograd_plumbing():
    S = _S()
    occ, gt, pred, sdf = case(2 * 16 ** 3, 2, 50, seed=41)
    host = occ, gt, pred, sdf
    o, p = _t(occ).requires_grad_(), _t(pred).requires_grad_()
    out = S.stage2_loss(o, _t(gt), p, _t(sdf), 1.0, W)
    assert sorted(out) == sorted(S.KEYS) and all(v.shape == () and v.dtype == torch.float32 for v in out.values())
    assert out["occ_loss"].requires_grad and out["sdf_loss"].requires_grad
    assert not out["ignore_sdf_loss_realvalue"].requires_grad and not out["ignore_sdf_accuracy"].requires_grad
    (0.125 * (2 * out["occ_loss"] + out["sdf_loss"])).backward()                # a non-trivial upstream scale
    w_occ, w_sdf = S.stage2_grad_cpu(*host, 1.0, W, grad_out=(0.25, 0.125), device=True)
    assert ulps(o.grad.cpu().numpy(), w_occ) <= 1 and ulps(p.grad.cpu().numpy(), w_sdf) <= 1
    # occ not requiring grad: no gradient buffer for it, the other side as before
    o2, p2 = _t(occ), _t(pred).requires_grad_()
    out2 = S.stage2_loss(o2, _t(gt), p2, _t(sdf), 1.0, W)
    (0.125 * (2 * out2["occ_loss"] + out2["sdf_loss"])).backward()
    assert o2.grad is None and torch.equal(p2.grad, p.grad)
    o3, p3 = _t(occ).requires_grad_(), _t(pred)
    out3 = S.stage2_loss(o3, _t(gt), p3, _t(sdf), 1.0, W)
    out3["occ_loss"].backward()
    assert p3.grad is None and ulps(o3.grad.cpu().numpy(), S.stage2_grad_cpu(*host, 1.0, W, device=True)[0]) <= 1
    with torch.no_grad():
        assert not S.stage2_loss(o, _t(gt), p, _t(sdf), 1.0, W)["occ_loss"].requires_grad
    # other dtypes and layouts are converted, and the gradient comes back in the input's own
    o4 = _t(occ).double().reshape(64, 128).t().requires_grad_()
    gt4 = _t(gt).reshape(64, 128).t().to(torch.int32)
    out4 = S.stage2_loss(o4, gt4, _t(pred).double(), _t(sdf).double(), 1.0, W)
    out4["occ_loss"].backward()
    assert o4.grad.dtype == torch.float64 and o4.grad.shape == (128, 64)
    want4 = S.stage2_grad_cpu(np.ascontiguousarray(occ.reshape(64, 128).T), np.ascontiguousarray(gt.reshape(64, 128).T),
                              pred, sdf, 1.0, W, device=True)[0]
    assert ulps(o4.grad.float().cpu().numpy(), want4) <= 1


def test_executor_takes_its_local_terms_from_hip_when_asked():
    from list_amd import arguments
    from list_amd.network import executors
    S = _S()
    occ, gt, pred, sdf = case(2 * 16 ** 3, 2, 50, seed=51)
    occ, gt = occ.reshape(2, 1, 16, 16, 16), gt.reshape(2, 1, 16, 16, 16)
    want = S.stage2_loss_cpu(occ, gt, pred, sdf, 1.0, W, device=True)
    ex_hip = executors.LIST(arguments.default_config(stage2_loss="hip"), None)
    ex_def = executors.LIST(arguments.default_config(), None)
    for target in (gt, gt.astype(np.uint8)):
        o, p = _t(occ).requires_grad_(), _t(pred).requires_grad_()
        got = ex_hip.calc_loss((o, p), (_t(target), _t(sdf)))
        assert sorted(got) == sorted(S.KEYS)
        d = [ulps(float(got[k].detach()), want[k]) for k in S.KEYS]
        print("calc_loss with stage2_loss = 'hip': ulps from the restatement", d)
        assert max(d[:3]) <= 2 and d[3] == 0
        (got["occ_loss"] + got["sdf_loss"]).backward()
        w_occ, w_sdf = S.stage2_grad_cpu(occ, gt, pred, sdf, 1.0, W, device=True)
        assert ulps(o.grad.cpu().numpy(), w_occ) <= 1 and ulps(p.grad.cpu().numpy(), w_sdf) <= 1
    # the default: the torch expressions' bits, unchanged
    o, t, p, s = _t(occ), _t(gt), _t(pred), _t(sdf)
    got = ex_def.calc_loss((o, p), (t, s))
    occ_loss = 1000 * (-W * torch.mean(t * torch.log(o + 1e-8)) - (1 - W) * torch.mean((1 - t) * torch.log(1 - o + 1e-8)))
    sdf_terms = executors.L.SDFLoss(1.0)(p, s)
    assert torch.equal(got["occ_loss"], occ_loss) and all(torch.equal(got[k], sdf_terms[k]) for k in S.KEYS[1:])
    got8 = ex_def.calc_loss((o, p), (_t(gt.astype(np.uint8)), s))                 # uint8 targets on the torch path
    assert torch.equal(got8["occ_loss"], occ_loss)


@pytest.mark.parametrize("kind", ["float32", "uint8"])
@pytest.mark.parametrize("n", [7, 1030, SWEEP + 7])
def test_backward_into_gradient_views_one_element_past_an_aligned_base(kind, n):
    """list_s2loss_bwd through ctypes with every buffer, the two gradients included, entered at buf[1:]: three head
    elements, then 16-byte loads and stores, then a tail.  stage2_loss itself never gets here (its gradients are fresh,
    aligned buffers).  The elements in front of and behind the views stay as they were."""
    S = _S()
    occ, gt, pred, sdf = case(n + 1, 1, n + 1, seed=n + 1)
    d = [_t(occ), _t(gt.astype(kind)), _t(pred.reshape(-1)), _t(sdf.reshape(-1))]
    g_occ = torch.full((n + 2,), 7.0, dtype=torch.float32, device=DEV)
    g_sdf = torch.full((n + 2,), 7.0, dtype=torch.float32, device=DEV)
    g = _t(np.array([0.75, 3.0, 100.0, 100.0], np.float32))
    v = [t[1:] for t in d] + [g_occ[1:n + 1], g_sdf[1:n + 1]]
    assert all(t.data_ptr() % 16 == (1 if t.dtype == torch.uint8 else 4) for t in v)
    with torch.cuda.device(DEV):
        rc = S.load().list_s2loss_bwd(v[0].data_ptr(), v[1].data_ptr(), 0 if kind == "float32" else 1, n, v[2].data_ptr(),
                                      v[3].data_ptr(), 1, n, 2.0, W, g.data_ptr(), v[4].data_ptr(), v[5].data_ptr(),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, S._section.last_error()
    w_occ, w_sdf = S.stage2_grad_cpu(occ[1:], gt[1:], pred[:, 1:], sdf[:, 1:], 2.0, W, grad_out=(0.75, 3.0), device=True)
    got_occ, got_sdf = g_occ.cpu().numpy(), g_sdf.cpu().numpy()
    dg = ulps(got_occ[1:n + 1], w_occ), ulps(got_sdf[1:n + 1], w_sdf.reshape(-1))
    print(f"gradient views at buf[1:], n = {n}, {kind}: ulps {dg}")
    assert dg[0] <= 1 and dg[1] <= 1
    assert got_occ[0] == got_occ[-1] == got_sdf[0] == got_sdf[-1] == 7.0


def test_the_devices_logarithm_is_held_to_what_the_hosts_is():
    """csrc/s2loss_math.h as the device compiles it (its frexp, fma and division), through list_s2loss_log, against
    numpy's float64 log at the 4 float64 ulps its header derives: every 29th float32 in [2^-31, 4) -- which holds every
    occ + 1e-8f of a valid occupancy --, every 8191st of the other positive ones (subnormals included), and libm's
    non-finite cases."""
    S = _S()
    bits = np.concatenate([np.arange(1, 0x30000000, 8191, dtype=np.int64), np.arange(0x30000000, 0x40800000, 29, dtype=np.int64),
                           np.arange(0x40800000, 0x7F800000, 8191, dtype=np.int64)]).astype(np.uint32)
    x = bits.view(np.float32)
    got = S.device_log(_t(x)).cpu().numpy()
    want = np.log(x.astype(np.float64))
    assert got.dtype == np.float64 and np.isfinite(got).all()
    ulp = np.spacing(np.abs(want))
    err = np.where(want == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - want) / ulp)
    print(f"{x.size} float32 arguments: the device's logarithm is within {err.max():.3f} float64 ulps of numpy's")
    assert x.size > 9_000_000 and err.max() <= 4.0
    special = np.array([0.0, -0.0, -1e-3, np.nan, np.inf, -np.inf, 1.0], np.float32)
    with np.errstate(all="ignore"):
        want = np.log(special.astype(np.float64))
    got = S.device_log(_t(special)).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True) and got[6] == 0.0 and got[0] == got[1] == -np.inf
