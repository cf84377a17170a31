"""GPU: the ragged-batch resize (list_resize_fwd through resize.apply and called directly between guard bands) against the
numpy restatement apply_cpu, every element bit for bit: every branch of the pass order in one call, both memory formats,
odd packed offsets, an untouched source, a reused workspace; the executors on a Pix3D batch.  No Pillow is needed here:
apply_cpu is held to it by tests/test_resize_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resize_case as RC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096                                            # bytes (uint8) / elements (float32) on either side


def _mods():
    import __graft_entry__ as ge
    ge.build()
    from list_amd import augment, hip, resize
    return augment, resize, hip


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def odd_pack(R, images):
    """The images packed so that every one starts on an odd byte."""
    offsets, at = [], 1
    for im in images:
        offsets.append(at)
        at += im.size
        at += 1 - at % 2
    data = np.full(at + 1, 0x5A, np.uint8)
    for o, im in zip(offsets, images):
        data[o:o + im.size] = im.reshape(-1)
    assert all(o % 2 == 1 for o in offsets)
    return R.RaggedImages(torch.from_numpy(data), [im.shape[:2] for im in images], offsets)


def run_guarded(R, hip, ragged_dev, out_h, out_w, params, cl, ws=None):
    """list_resize_fwd on buffers carved out of larger ones -> (out tensor [B,3,out_h,out_w], check()): check asserts, after
    the work, that the bytes around the output and the workspace are as they were filled."""
    lib, rec, B = R.load(), ragged_dev.records(), len(ragged_dev)
    buf = R.plan(ragged_dev, out_h, out_w)
    need = lib.list_resize_workspace_bytes(rec.ctypes.data, B, out_h, out_w)
    assert need == int(R.parse_plan(buf)[0]["workspace_bytes"]) > 0
    n = B * 3 * out_h * out_w
    out_buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    out_buf[:GUARD], out_buf[GUARD + n:] = -7.0, -7.0
    if ws is None:
        ws = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.numel() >= need + 2 * GUARD
    plan_dev = torch.from_numpy(buf).to(DEV)
    p_dev = None if params is None else torch.from_numpy(params.view(np.uint8).reshape(B, -1)).to(DEV)
    rc = lib.list_resize_fwd(ragged_dev.data.data_ptr(), ragged_dev.data.numel(), buf.ctypes.data, plan_dev.data_ptr(), buf.size,
                             None if params is None else params.ctypes.data, None if params is None else p_dev.data_ptr(),
                             out_buf.data_ptr() + 4 * GUARD, int(cl), ws.data_ptr() + GUARD, need, hip._stream())
    assert rc == 0, lib.list_resize_last_error()
    body = out_buf[GUARD:GUARD + n]
    out = body.view(B, out_h, out_w, 3).permute(0, 3, 1, 2) if cl else body.view(B, 3, out_h, out_w)

    def check():
        assert bool((out_buf[:GUARD] == -7.0).all()) and bool((out_buf[GUARD + n:] == -7.0).all())
        assert bool((ws[:GUARD] == 0xA5).all()) and bool((ws[GUARD + need:] == 0xA5).all())
        assert not bool(torch.isnan(body).any())            # every element was written
        return plan_dev, p_dev                              # (kept alive until here)

    return out, check, ws


def compare(got, want, what):
    bad = np.argwhere(bits(got.cpu().numpy()) != bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("out_h,out_w", [(16, 12), (24, 24)])
@pytest.mark.parametrize("cl", [False, True])
def test_every_branch_in_one_ragged_batch(out_h, out_w, cl):
    """B = 9: 1 x 1, a skipped pass on either axis, the copy, up-scaling, a reduction, a long filter, the tall rule and
    its border; all-255 and checkerboard images, flips and jitters in several orders; every image starts on an odd byte."""
    A, R, hip = _mods()
    images, params = RC.branch_batch(A, out_h, out_w)
    ragged = odd_pack(R, images)
    stages = [R.stages_cpu(h, w, out_h, out_w)[0] for h, w in ragged.sizes.tolist()]
    assert {(0, 0), (1, 0), (2, 0), (1, 2), (2, 1)} == set(stages) and stages[7] == (2, 1) and stages[8] == (1, 2)
    assert R.coeffs_cpu(700, out_h)[1].shape[1] == 2 * -(-700 // out_h) + 1 and R.coeffs_cpu(13, out_h)[1].shape[1] == 3
    want = R.apply_cpu(ragged, out_h, out_w, params)
    dev = ragged.to(DEV)
    before = dev.data.clone()
    out, check, _ = run_guarded(R, hip, dev, out_h, out_w, params, cl)
    torch.cuda.synchronize()
    check()
    compare(out, want, "guarded")
    assert torch.equal(dev.data, before)                    # src is never written
    via = R.apply(dev, out_h, out_w, params, channels_last=cl)
    assert via.shape == (9, 3, out_h, out_w) and via.dtype == torch.float32 and via.device == dev.device
    assert via.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    compare(via, want, "apply")
    compare(R.apply(dev, out_h, out_w, None, channels_last=cl), R.apply_cpu(ragged, out_h, out_w), "plain")


@pytest.mark.parametrize("out_h,out_w", [(16, 12), (24, 24)])
@pytest.mark.parametrize("which", [0, 3, 5, 6, 7])
def test_a_batch_of_one(out_h, out_w, which):
    A, R, hip = _mods()
    images, params = RC.branch_batch(A, out_h, out_w, seed=1)
    ragged, p = odd_pack(R, images[which:which + 1]), params[which:which + 1]
    want = R.apply_cpu(ragged, out_h, out_w, p)
    for cl in (False, True):
        out, check, _ = run_guarded(R, hip, ragged.to(DEV), out_h, out_w, p, cl)
        torch.cuda.synchronize()
        check()
        compare(out, want, cl)


@pytest.mark.parametrize("out_h", [303, 320])
def test_the_tall_rule_needs_a_smaller_height(out_h):
    """303 x 3 with out_h >= H: H > 100 * W, but the height does not shrink, so the horizontal pass comes first (or alone)."""
    A, R, hip = _mods()
    images = [RC.pixels("random", 303, 3, 5), RC.pixels("checker", 303, 3)]
    params = np.concatenate([A.make_params(15, (2, 3, 0, 1), 0.9, 1.4, 33), A.make_params(A.FLIP)])
    ragged = odd_pack(R, images)
    assert R.stages_cpu(303, 3, out_h, 8)[0] == ((1, 0) if out_h == 303 else (1, 2))
    want = R.apply_cpu(ragged, out_h, 8, params)
    out, check, _ = run_guarded(R, hip, ragged.to(DEV), out_h, 8, params, False)
    torch.cuda.synchronize()
    check()
    compare(out, want, out_h)


def test_700_rows_to_8_take_177_taps():
    A, R, hip = _mods()
    images = [RC.pixels("random", 700, 3, 6), RC.pixels("ones", 700, 3), RC.pixels("random", 3000, 17, 6)]
    params = np.concatenate([A.make_params(A.FLIP | A.SATURATION, saturation=1.5), A.make_params(0), A.make_params(A.HUE, shift=90)])
    ragged = odd_pack(R, images)
    assert R.coeffs_cpu(700, 8)[1].shape[1] == 177 and R.stages_cpu(700, 3, 8, 8)[0] == (2, 1)
    want = R.apply_cpu(ragged, 8, 8, params)
    assert np.array_equal(want[1], np.ones((3, 8, 8), np.float32))
    out, check, _ = run_guarded(R, hip, ragged.to(DEV), 8, 8, params, True)
    torch.cuda.synchronize()
    check()
    compare(out, want, "8 x 8")


def test_pix3d_like_sizes_to_224():
    A, R, hip = _mods()
    images = [RC.pixels("random", 480, 640, 2), RC.pixels("random", 224, 300, 2), RC.pixels("checker", 501, 333)]
    params = A.draw_params(3, True, True, torch.Generator().manual_seed(224))
    ragged = R.RaggedImages.pack(images)
    want = R.apply_cpu(ragged, 224, 224, params)
    for cl in (False, True):
        compare(R.apply(ragged.to(DEV), 224, 224, params, channels_last=cl), want, cl)


def test_a_second_batch_reuses_the_workspace_behind_the_first():
    """Two calls back to back on one stream and one workspace, nothing waited for in between."""
    A, R, hip = _mods()
    first, p1 = RC.branch_batch(A, 16, 12, seed=3)
    second, p2 = RC.branch_batch(A, 24, 24, seed=4)
    second, p2 = second[::-1], np.ascontiguousarray(p2[::-1])
    r1, r2 = odd_pack(R, first), odd_pack(R, second)
    d1, d2 = r1.to(DEV), r2.to(DEV)
    need = max(R.load().list_resize_workspace_bytes(r.records().ctypes.data, 9, h, w) for r, h, w in ((r1, 16, 12), (r2, 24, 24)))
    ws = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    out1, check1, _ = run_guarded(R, hip, d1, 16, 12, p1, False, ws)
    out2, check2, _ = run_guarded(R, hip, d2, 24, 24, p2, True, ws)
    torch.cuda.synchronize()
    assert bool((ws[:GUARD] == 0xA5).all()) and bool((ws[GUARD + need:] == 0xA5).all())
    compare(out1, R.apply_cpu(r1, 16, 12, p1), "first")
    compare(out2, R.apply_cpu(r2, 24, 24, p2), "second")


# ---- the executors ----------------------------------------------------------------------------------------------------------
class Recorder(torch.nn.Module):
    """The model behind a wrapper that keeps the image tensor it was called with."""

    def __init__(self, module):
        super().__init__()
        self.module, self.images = module, []

    def forward(self, img, *rest):
        self.images.append(img)
        return self.module(img, *rest)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from list_amd import synthetic
    return synthetic.make_pix3d_tree(str(tmp_path_factory.mktemp("pix3d")))


@pytest.mark.parametrize("kind,res", [("LIST", 64), ("CoarseNet", 128)])
def test_executor_trains_on_a_pix3d_batch_resized_on_the_device(tree, kind, res):
    """One train step on a batch of raw images of two sizes from Datasets.collate (--augment hip): the model sees
    apply_cpu's tensor under the executor's first draw, bit for bit, and the loss is finite and differentiable."""
    A, R, hip = _mods()
    from list_amd import arguments, utils
    from list_amd.datasets import Datasets
    torch.manual_seed(0)
    cfg = arguments.default_config(model=f"network.models.{kind}", dataset="datasets.Datasets.Pix3D", data_dir=tree["data_dir"],
                                   catlist=["chair", "table"], img_res=res, vox_res=32, train_batch_size=2,
                                   sample_point_density=200, coarse_point_density=300, augment="hip", color_jitter=True,
                                   random_h_flip=True)
    model = Recorder(utils.get_class(cfg.model)(cfg).to(DEV))
    model.train()
    ds = utils.get_class(cfg.dataset)(cfg, "train")
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=Datasets.collate)))
    ragged = batch["rgb_image"]
    assert isinstance(ragged, R.RaggedImages) and ragged.sizes.tolist() == [[37, 53], [64, 48]]
    ex = utils.get_class(f"network.executors.{kind}")(cfg, model)
    _, losses = ex.train(batch)
    loss = sum(v for k, v in losses.items() if "ignore" not in k)
    want = R.apply_cpu(ragged, res, res, A.draw_params(2, True, True, torch.Generator().manual_seed(333)))
    seen = model.images[0]
    assert seen.shape == (2, 3, res, res) and seen.dtype == torch.float32 and seen.is_cuda
    compare(seen, want, kind)
    assert bool(torch.isfinite(loss)) and loss.requires_grad
