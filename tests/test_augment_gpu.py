"""GPU: the augmentation kernel (list_augment_fwd through augment.apply) against the numpy restatement apply_cpu, every
element bit for bit, in both memory formats and on both load paths; every colour through the device against the host's
compilation of csrc/augment_math.h; the executors on a uint8 batch.  No Pillow is needed here: apply_cpu is held to it by
tests/test_augment_cpu.py."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_case as AC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _A():
    import __graft_entry__ as ge
    ge.build()
    from list_amd import augment
    return augment


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(images, params, source=None):
    """apply on the device (from `source`, a device tensor holding `images`, when given) == apply_cpu, NCHW and
    channels-last."""
    A = _A()
    want = A.apply_cpu(images, params)
    src = torch.from_numpy(images).to(DEV) if source is None else source
    B, H, W, _ = images.shape
    for cl in (False, True):
        out = A.apply(src, params, channels_last=cl)
        assert out.shape == (B, 3, H, W) and out.dtype == torch.float32 and out.device == src.device
        assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        got = out.cpu().numpy()
        bad = np.argwhere(bits(got) != bits(want))
        assert bad.size == 0, (cl, len(bad), bad[:4].tolist())
    return want


def three_records(A):
    """Flip with every colour step, the colour steps without the flip in another order, the flip alone."""
    return np.concatenate([A.make_params(15, (3, 0, 2, 1), 0.7, 1.5, 127), A.make_params(14, (2, 1, 0, 3), 1.3, 0.5, 255),
                           A.make_params(A.FLIP)])


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (2, 4), (1, 5), (3, 8), (2, 13)])
def test_small_shapes_on_both_load_paths(H, W):
    """W = 4 and 8 take the dword path, the others the byte path with its row tail; flips at odd and even W."""
    A = _A()
    images = np.random.default_rng(100 * H + W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    want = check(images, three_records(A))
    if W > 1:
        assert np.array_equal(want[2], (images[2, :, ::-1].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def test_a_training_batch_of_224():
    A = _A()
    images = np.random.default_rng(224).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    check(images, three_records(A)[:2])
    check(images, A.draw_params(2, True, True, torch.Generator().manual_seed(224)))
    check(images, None)                                 # plain ToTensor
    assert torch.equal(A.apply(torch.from_numpy(images).to(DEV)).cpu(),
                       torch.from_numpy(images).permute(0, 3, 1, 2).float() / 255)


def test_a_source_one_byte_past_an_aligned_address():
    A = _A()
    images = np.random.default_rng(8).integers(0, 256, (3, 3, 8, 3), dtype=np.uint8)
    buffer = torch.zeros(images.size + 1, dtype=torch.uint8, device=DEV)
    buffer[1:] = torch.from_numpy(images.reshape(-1)).to(DEV)
    source = buffer[1:].view(3, 3, 8, 3)
    assert source.data_ptr() % 4 == 1 and source.is_contiguous()
    check(images, three_records(A), source)


@pytest.mark.parametrize("W", [8, 5])
def test_every_order_with_every_ops_mask(W):
    """24 orders (the six orders of the three live steps with the no-op slot in each of its four positions) x 16 masks,
    one image each, in one launch."""
    A = _A()
    rng = np.random.default_rng(W)
    records = [A.make_params(ops, order, rng.uniform(0.7, 1.3), rng.uniform(0.5, 1.5), int(rng.integers(0, 256)))
               for order in itertools.permutations(range(4)) for ops in range(16)]
    images = rng.integers(0, 256, (len(records), 3, W, 3), dtype=np.uint8)
    check(images, np.concatenate(records))


def test_shifts_and_factors_at_their_ends():
    A = _A()
    records = [A.make_params(A.JITTER, (0, 1, 2, 3), b, s, shift)
               for shift in (0, 1, 127, 128, 255) for b in (0.7, 1.0, 1.3) for s in (0.5, 1.0, 1.5)]
    rng = np.random.default_rng(45)
    images = rng.integers(0, 256, (len(records), 16, 16, 3), dtype=np.uint8)
    images[:, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [128, 128, 128]]
    check(images, np.concatenate(records))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return AC.build_host(tmp_path_factory.mktemp("augment_host"))


@pytest.fixture(scope="module")
def colours_on_device():
    return torch.from_numpy(AC.all_colours()[None]).to(DEV)


@pytest.mark.parametrize("step,value", [("hue", 127), ("saturation", 1.37), ("brightness", 1.23)])
def test_every_colour_through_the_device(host_exe, colours_on_device, tmp_path, step, value):
    """All 2^24 colours as one 4096 x 4096 image against the host's bytes: the device's float32 division and float64
    fmod, floor and rint round as the host's do."""
    A = _A()
    p = {"hue": A.make_params(A.HUE, shift=value), "saturation": A.make_params(A.SATURATION, saturation=value),
         "brightness": A.make_params(A.BRIGHTNESS, brightness=value)}[step]
    want = AC.run_host(host_exe, step, value, tmp_path).transpose(2, 0, 1)
    out = A.apply(colours_on_device, p)[0].cpu().numpy()
    levels = np.rint(out * np.float32(255))
    wrong = int((levels != want).sum())
    assert wrong == 0, f"{step}: {wrong} of {want.size} levels differ from the host's"
    assert np.array_equal(bits(out), bits(want.astype(np.float32) / np.float32(255)))


# ---- the executors ----------------------------------------------------------------------------------------------------------
class Recorder(torch.nn.Module):
    """The model behind a wrapper that keeps the image tensor it was called with."""

    def __init__(self, module):
        super().__init__()
        self.module, self.images = module, []

    def forward(self, img, *rest):
        self.images.append(img)
        return self.module(img, *rest)


def _executor(kind, res):
    from list_amd import arguments, utils
    torch.manual_seed(0)
    names = {"LIST": "SyntheticIM2SDF", "CoarseNet": "SyntheticIM2PointFarthest"}
    cfg = arguments.default_config(model=f"network.models.{kind}", dataset=f"datasets.Datasets.{names[kind]}", img_res=res,
                                   vox_res=32, train_batch_size=2, synthetic_len=2, sample_point_density=200,
                                   augment="hip", color_jitter=True, random_h_flip=True)
    model = Recorder(utils.get_class(cfg.model)(cfg).to(DEV))
    model.train()
    batch = next(iter(torch.utils.data.DataLoader(utils.get_class(cfg.dataset)(cfg, "train"), batch_size=2)))
    return utils.get_class(f"network.executors.{kind}")(cfg, model), batch


@pytest.fixture
def deterministic_convolutions():
    """Two passes of a model over one image tensor are compared bit for bit below.  By default the convolution library
    may pick its algorithm anew from one pass to the next (seen on an MI355X: sdf_loss 7.549064 against 7.549160 on
    bit-identical images, while four passes in a row over one tensor agreed), so it is asked for its deterministic
    algorithms while they run."""
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


@pytest.mark.parametrize("kind,res", [("LIST", 64), ("CoarseNet", 128)])
def test_executor_augments_a_uint8_batch_on_the_device(kind, res, deterministic_convolutions):
    """A uint8 batch in hip mode == the same batch augmented with apply_cpu under the same draws and fed as float: the
    model sees the identical tensor, so the loss is the same bits.  A float batch reaches the model as it is."""
    A = _A()
    ex, batch = _executor(kind, res)
    images = np.random.default_rng(res).integers(0, 256, (2, res, res, 3), dtype=np.uint8)
    params = A.draw_params(2, True, True, torch.Generator().manual_seed(333))       # the executor's first draw
    as_float = torch.from_numpy(A.apply_cpu(images, params))
    with torch.no_grad():
        ex.train(batch)                                 # (the synthetic float batch: every shape has run once)
        _, loss_u8 = ex.train(dict(batch, rgb_image=torch.from_numpy(images)))
        _, loss_f = ex.train(dict(batch, rgb_image=as_float))
    seen = ex.model.images
    assert torch.equal(seen[0].cpu(), batch["rgb_image"]) and seen[0].stride() == batch["rgb_image"].stride()
    assert seen[1].dtype == torch.float32 and seen[1].stride() == seen[2].stride() and seen[1].device == seen[2].device
    assert np.array_equal(bits(seen[1].cpu().numpy()), bits(as_float.numpy()))
    assert torch.equal(seen[2].cpu(), as_float)
    assert sorted(loss_u8) == sorted(loss_f) and len(loss_u8) >= 1
    for k in loss_u8:
        print(k, float(loss_u8[k]), float(loss_f[k]))
        assert torch.equal(loss_u8[k], loss_f[k]), k
