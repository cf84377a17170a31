"""CPU: the training-image augmentation (list_amd.augment) against Pillow, which is the judge: csrc/augment_math.h as the
host compiles it over every colour, the numpy restatement apply_cpu against jitter_pil + ToTensor bit for bit, the
parameter draws, the datasets in host and hip mode, and the C ABI of include/list_augment.h without a GPU."""
import ctypes
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from list_amd import arguments, augment as A, hip, utils
from list_amd.datasets import Datasets
from list_amd.network import executors
from oracle import dataset_fixture as DF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_case as AC  # noqa: E402
import _capi_headers as H  # noqa: E402


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return AC.build_host(tmp_path_factory.mktemp("augment_host"))


@pytest.fixture(scope="module")
def colours():
    a = AC.all_colours()
    a.setflags(write=False)
    return a


# ---- the math header against Pillow, no tolerance ---------------------------------------------------------------------------
def pil_hue(image, shift):
    h, s, v = Image.fromarray(image).convert("HSV").split()
    h = Image.fromarray(((np.asarray(h).astype(np.int32) + shift) % 256).astype(np.uint8))
    return np.asarray(Image.merge("HSV", (h, s, v)).convert("RGB"))


@pytest.mark.parametrize("shift", [0, 1, 127, 255])
def test_hue_step_equals_pillow_on_every_colour(host_exe, colours, tmp_path, shift):
    got = AC.run_host(host_exe, "hue", shift, tmp_path)
    assert np.array_equal(got, pil_hue(colours, shift))
    if shift == 0:
        assert (got != colours).any()           # the round trip through HSV is lossy, and is made all the same


def test_brightness_step_equals_pillow_on_every_level(host_exe, tmp_path):
    level = np.arange(256)
    image = np.stack([level, 255 - level, level ^ 0x55], -1).astype(np.uint8)[None]      # each channel holds every level
    for f in np.linspace(0.7, 1.3, 61).astype(np.float32):
        want = np.asarray(ImageEnhance.Brightness(Image.fromarray(image)).enhance(float(f)))
        assert np.array_equal(AC.run_host(host_exe, "brightness", f, tmp_path, image), want), f


def test_saturation_step_equals_pillow_on_a_colour_lattice(host_exe, tmp_path):
    lv = np.rint(np.arange(64) * 255 / 63).astype(np.uint8)
    image = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(512, 512, 3)
    for f in np.array([0.5, 0.61, 0.99, 1.0, 1.01, 1.37, 1.5], np.float32):
        want = np.asarray(ImageEnhance.Color(Image.fromarray(image)).enhance(float(f)))
        assert np.array_equal(AC.run_host(host_exe, "saturation", f, tmp_path, image), want), f


# ---- apply_cpu against jitter_pil + ToTensor --------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("H,W", [(13, 9), (32, 48)])
def test_apply_cpu_equals_pillow_bit_for_bit(H, W):
    """All 24 orders x every ops mask (the flip bit on and off with every subset of the colour steps), drawn factors."""
    rng = np.random.default_rng(H)
    image = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    for order in itertools.permutations(range(4)):
        for ops in range(16):
            p = A.make_params(ops, order, rng.uniform(0.7, 1.3), rng.uniform(0.5, 1.5), A.hue_shift(rng.uniform(-0.5, 0.5)))
            got = A.apply_cpu(image, p)
            want = A.to_tensor(A.jitter_pil(image[0], p)).numpy()
            assert got.shape == (1, 3, H, W) and got.dtype == np.float32
            assert np.array_equal(bits(got[0]), bits(want)), (order, ops, p)
    plain = A.apply_cpu(image)                                             # no parameters: ToTensor
    assert np.array_equal(bits(plain[0]), bits((image[0].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)))


def test_a_batch_takes_one_record_per_image_and_cpu_tensors_take_apply_cpu():
    rng = np.random.default_rng(3)
    images = rng.integers(0, 256, (3, 6, 5, 3), dtype=np.uint8)
    p = A.draw_params(3, True, True, torch.Generator().manual_seed(9))
    got = A.apply_cpu(images, p)
    for i in range(3):
        assert np.array_equal(bits(got[i]), bits(A.to_tensor(A.jitter_pil(images[i], p[i:i + 1])).numpy()))
    for cl in (False, True):
        t = A.apply(torch.from_numpy(images), p, channels_last=cl)
        assert t.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        assert np.array_equal(bits(t.numpy()), bits(got))
    for bad in (images.astype(np.float32), images[..., :2], images[0]):
        with pytest.raises(ValueError):
            A.apply_cpu(bad)
    with pytest.raises(ValueError, match="record"):
        A.apply_cpu(images, p[:2])
    for field, value in (("ops", 16), ("order", (0, 1, 2, 2)), ("brightness", 1.31), ("saturation", 0.49), ("hue_shift", 256)):
        q = p.copy()
        q[field][1] = value
        with pytest.raises(ValueError, match=rf"params\[1\]\.{field}"):
            A.apply_cpu(images, q)


# ---- the draws --------------------------------------------------------------------------------------------------------------
def test_draw_params_is_deterministic_and_covers_its_distribution():
    a = A.draw_params(4000, True, True, torch.Generator().manual_seed(5))
    b = A.draw_params(4000, True, True, torch.Generator().manual_seed(5))
    assert a.dtype == A.PARAMS and a.shape == (4000,) and np.array_equal(a, b)
    assert not np.array_equal(a, A.draw_params(4000, True, True, torch.Generator().manual_seed(6)))
    assert (np.sort(a["order"], axis=1) == np.arange(4)).all()
    assert len({tuple(o) for o in a["order"]}) == 24
    assert set(a["ops"]) == {A.JITTER, A.JITTER | A.FLIP} and 1500 < int((a["ops"] & A.FLIP).sum()) < 2500
    assert (a["brightness"] >= np.float32(0.7)).all() and (a["brightness"] <= np.float32(1.3)).all()
    assert (a["saturation"] >= np.float32(0.5)).all() and (a["saturation"] <= np.float32(1.5)).all()
    assert a["brightness"].max() - a["brightness"].min() > 0.55 and a["saturation"].max() - a["saturation"].min() > 0.95
    # hue in [-0.5, 0.5] reaches the shifts 0 ... 127 and 129 ... 255
    assert set(a["hue_shift"]) <= set(range(128)) | set(range(129, 256)) and len(set(a["hue_shift"])) > 240
    assert [A.hue_shift(h) for h in (0.0, 0.5, -0.5, 1.5 / 255, -1.5 / 255, 0.0039)] == [0, 127, 129, 1, 255, 0]
    # the order of the draws: the coin, the permutation, then the three uniforms
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    one = A.draw_params(1, True, True, g)[0]
    coin = float(torch.rand(1, generator=h)) < 0.5
    order = torch.randperm(4, generator=h).numpy()
    u = [float(torch.empty(1).uniform_(lo, hi, generator=h)) for lo, hi in ((0.7, 1.3), (0.5, 1.5), (-0.5, 0.5))]
    assert bool(one["ops"] & A.FLIP) == coin and np.array_equal(one["order"], order)
    assert (one["brightness"], one["saturation"], one["hue_shift"]) == (np.float32(u[0]), np.float32(u[1]), A.hue_shift(u[2]))
    # flags off: nothing is drawn, the records do nothing
    g = torch.Generator().manual_seed(5)
    state = g.get_state()
    assert np.array_equal(A.draw_params(3, False, False, g), A.identity_params(3)) and torch.equal(g.get_state(), state)
    assert set(A.draw_params(200, True, False, g)["ops"]) == {0, A.FLIP}


def test_draw_jitter_takes_its_draws_from_the_rng_it_is_handed():
    a, b = A.draw_jitter(random.Random(4)), A.draw_jitter(random.Random(4))
    assert np.array_equal(a, b) and a.shape == (1,) and int(a["ops"][0]) == A.JITTER
    orders = set()
    rng = np.random.RandomState(2)                      # a numpy state serves as well
    for _ in range(2000):
        p = A.draw_jitter(rng)[0]
        orders.add(tuple(p["order"]))
        assert sorted(p["order"]) == [0, 1, 2, 3]
        assert np.float32(0.7) <= p["brightness"] <= np.float32(1.3) and np.float32(0.5) <= p["saturation"] <= np.float32(1.5)
        assert p["hue_shift"] in range(256) and p["hue_shift"] != 128
    assert len(orders) == 24


# ---- the datasets -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("augment_tree")
    shape_ids = ["shape_a", "shape_b"]
    image_dir, h5_dir = DF.write_tree(str(root), shape_ids)
    split = root / "split"
    split.mkdir()
    for status in ("train", "test"):
        (split / f"{DF.CAT}_{status}.lst").write_text("\n".join(shape_ids) + "\n")
    files = [os.path.join(image_dir, DF.CAT, s, "easy", "00.png") for s in shape_ids]
    return dict(fields=dict(cuda=False, split_dir=str(split) + "/", **DF.config_fields(image_dir, h5_dir)), files=files)


def pixels(fn):
    return np.asarray(Image.open(fn).convert("RGB"))


def parent_item(fn):
    """What the loader returned before this option existed: uint8 / 255, planes first."""
    a = np.asarray(Image.open(fn).convert("RGB"), dtype=np.float32) / np.float32(255.0)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


DATASETS = ["datasets.Datasets.IM2SDF", "datasets.Datasets.IM2PointFarthest"]


def dataset(name, tree, status="train", **flags):
    fields = dict(tree["fields"])
    fields.update(flags)
    ds = utils.get_class(name)(arguments.default_config(**fields), status)
    assert type(ds).__name__.startswith("File") and len(ds) == 2
    return ds


@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("flip", [False, True])
def test_host_mode_jitters_with_pillow_under_the_rng_draws(tree, name, flip):
    ds = dataset(name, tree, color_jitter=True, random_h_flip=flip)
    flipped = set()
    for seed in range(6):
        random.seed(seed)
        item = ds[1]["rgb_image"]
        random.seed(seed)
        random.randint(0, 0)                            # the camera index comes first (viewnum = 1)
        img = Image.open(tree["files"][1]).convert("RGB")
        if flip and random.random() < 0.5:
            img = img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
            flipped.add(seed)
        want = A.to_tensor(A.jitter_pil(img, A.draw_jitter(random)))
        assert item.dtype == torch.float32 and item.shape == (3, DF.IMG, DF.IMG)
        assert torch.equal(item, want) and not torch.equal(item, parent_item(tree["files"][1]))
    assert bool(flipped) == flip and len(flipped) < 6


@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("mode", ["host", "hip"])
def test_both_flags_off_is_the_parents_item_in_either_mode(tree, name, mode):
    ds = dataset(name, tree, augment=mode)
    for i in range(2):
        item = ds[i]["rgb_image"]
        assert item.dtype == torch.float32 and torch.equal(item, parent_item(tree["files"][i]))


def test_flip_alone_in_host_mode_is_the_parents_flip(tree):
    ds = dataset(DATASETS[0], tree, random_h_flip=True)
    seen = set()
    for seed in range(8):
        random.seed(seed)
        item = ds[0]["rgb_image"]
        random.seed(seed)
        random.randint(0, 0)
        flip = random.random() < 0.5
        seen.add(flip)
        want = parent_item(tree["files"][0])
        assert torch.equal(item, want.flip(2) if flip else want)
    assert seen == {False, True}


@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("flags", [dict(color_jitter=True), dict(random_h_flip=True), dict(color_jitter=True, random_h_flip=True)])
def test_hip_mode_hands_out_the_files_pixels_and_draws_nothing(tree, name, flags):
    ds = dataset(name, tree, augment="hip", **flags)
    for i in range(2):
        random.seed(i)
        item = ds[i]["rgb_image"]
        after = random.getstate()
        random.seed(i)
        random.randint(0, 0)                            # the camera index, and no coin behind it
        assert random.getstate() == after
        assert item.dtype == torch.uint8 and item.shape == (DF.IMG, DF.IMG, 3)
        assert np.array_equal(item.numpy(), pixels(tree["files"][i]))
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2)))["rgb_image"]
    assert batch.dtype == torch.uint8 and batch.shape == (2, DF.IMG, DF.IMG, 3)


@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("mode", ["host", "hip"])
def test_test_status_is_unaffected(tree, name, mode):
    ds = dataset(name, tree, status="test", augment=mode, color_jitter=True, random_h_flip=True)
    state = random.getstate()
    for i in range(2):
        assert torch.equal(ds[i]["rgb_image"], parent_item(tree["files"][i]))
    got = ds.get_testdata(DF.CAT, "shape_a", 0)
    image = got["rgb_image"] if isinstance(got, dict) else got[0]
    assert torch.equal(image, parent_item(tree["files"][0]).unsqueeze(0))
    random.setstate(state)


def test_load_image_refuses_an_unknown_mode(tree):
    cfg = arguments.default_config(augment="device", color_jitter=True)
    with pytest.raises(ValueError, match="augment"):
        Datasets._load_image(tree["files"][0], cfg, True, random)


def test_the_option_defaults_to_host():
    assert arguments.default_config().augment == "host"
    assert arguments.get_args(["--augment", "hip", "--color_jitter"]).augment == "hip"
    with pytest.raises(SystemExit):
        arguments.get_args(["--augment", "torchvision"])


def test_executors_pass_a_float_batch_through_and_augment_a_uint8_batch():
    """On CPU tensors (apply takes apply_cpu there): the draws come from the executor's own generator, seeded once."""
    cfg = arguments.default_config(augment="hip", color_jitter=True, random_h_flip=True)
    images = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 8, 8, 3), dtype=np.uint8))
    f = torch.rand(2, 3, 8, 8)
    for ex in (executors.LIST(cfg, None), executors.CoarseNet(cfg, None)):
        g = torch.Generator().manual_seed(333)
        got = [ex.train_images(images, torch.device("cpu")) for _ in range(2)]
        want = [A.apply_cpu(images.numpy(), A.draw_params(2, True, True, g)) for _ in range(2)]
        assert all(np.array_equal(bits(a.numpy()), bits(b)) for a, b in zip(got, want))
        assert not torch.equal(got[0], got[1])          # the generator moves on from batch to batch
        assert ex.train_images(f, torch.device("cpu")) is f


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return A.load()


def test_header_table_and_library_agree(lib):
    names = H.declared("list_augment.h")
    assert names == sorted(A.AUGMENT_EXPORTS) == ["list_augment_fwd", "list_augment_last_error", "list_augment_pixel"]
    exported = H.exported(hip.LIB_PATH)
    assert {n for n in exported if n.startswith("list_augment_")} == set(names)
    assert not set(names) & set(hip.EXPORTS)
    for header, (_, _, prefixes) in H.SECTIONS.items():                 # no other section owns the prefix
        assert not prefixes or not any(n.startswith(prefixes) for n in names), header
    for n in names:
        assert getattr(lib, n) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9
    build = __import__("list_amd.build", fromlist=["x"])
    assert "list_augment.h" in build.PUBLIC_HEADERS and "augment_kernels.hip" in build.SOURCES
    assert "augment_math.h" in build.HEADERS
    text = open(os.path.join(H.ROOT, "include", "list_augment.h")).read()                 # the record the binding mirrors
    assert "int32_t ops;" in text and "int32_t order[4];" in text and A.PARAMS.itemsize == 32
    assert [A.PARAMS.fields[k][1] for k in ("ops", "order", "brightness", "saturation", "hue_shift")] == [0, 4, 20, 24, 28]


def test_refusals_come_before_any_hip_call(lib):
    fake = 256                                    # never dereferenced: every refusal below is a host check
    err = lambda: lib.list_augment_last_error().decode()
    good = A.draw_params(2, True, True, torch.Generator().manual_seed(0))

    def fwd(B=2, H=4, W=4, cl=0, p=good, **null):
        a = dict(src=fake, dst=fake, params_host=p.ctypes.data, params_device=fake)
        a.update(null)
        return lib.list_augment_fwd(a["src"], a["dst"], B, H, W, cl, a["params_host"], a["params_device"], None)

    for name in ("src", "dst", "params_host", "params_device"):
        assert fwd(**{name: None}) == hip.ERR_ARG and f"{name} is NULL" in err()
    for dims in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=65537), dict(W=65537)):
        assert fwd(**dims) == hip.ERR_SHAPE and "need 1 <= B" in err()
    big = A.identity_params(65536)
    assert fwd(B=65536, p=big) == hip.ERR_SHAPE and "B = 65536" in err()
    assert fwd(cl=2) == hip.ERR_SHAPE and "channels_last = 2" in err()

    def bad(field, value, ops=A.JITTER):
        p = good.copy()
        p["ops"][1] = ops
        p[field][1] = value
        return fwd(p=p)

    assert bad("ops", 16, 16) == hip.ERR_ARG and "params[1].ops = 16" in err()
    for order in ((0, 1, 2, 2), (0, 1, 2, 4), (-1, 1, 2, 3), (0, 0, 0, 0)):
        assert bad("order", order) == hip.ERR_ARG and "not a permutation" in err() and "params[1]" in err()
    for field, values in (("brightness", (0.69, 1.31, np.nan)), ("saturation", (0.49, 1.51, np.inf)), ("hue_shift", (-1, 256))):
        for v in values:
            assert bad(field, v) == hip.ERR_ARG and f"params[1].{field}" in err(), (field, v)
    # a factor is read only while its step is enabled
    for field, v in (("brightness", 5.0), ("saturation", -1.0), ("hue_shift", 999)):
        p = A.identity_params(1)
        p[field][0] = v
        levels = np.empty(3, np.uint8)
        rgb = np.array([9, 8, 7], np.uint8)
        assert lib.list_augment_pixel(rgb.ctypes.data, p.ctypes.data, levels.ctypes.data, None) == 0       # step off: unread
        assert levels.tolist() == [9, 8, 7]
    rgb = np.zeros(3, np.uint8)
    assert lib.list_augment_pixel(None, good.ctypes.data, None, None) == hip.ERR_ARG and "rgb_in is NULL" in err()
    assert lib.list_augment_pixel(rgb.ctypes.data, None, None, None) == hip.ERR_ARG and "p is NULL" in err()
    p = good.copy()
    p["order"][0] = (3, 3, 3, 3)
    assert lib.list_augment_pixel(rgb.ctypes.data, p.ctypes.data, None, None) == hip.ERR_ARG and "permutation" in err()


def test_the_library_runs_the_header_on_one_pixel(lib):
    """list_augment_pixel (the host's compilation inside the library) against the numpy restatement, full records."""
    rng = np.random.default_rng(11)
    g = torch.Generator().manual_seed(11)
    for p in A.draw_params(300, False, True, g):
        rgb = rng.integers(0, 256, 3, dtype=np.uint8)
        levels, values = A.pixel(rgb, p)
        want = A.colour_cpu(rgb, p)
        assert levels.tolist() == want.tolist()
        assert np.array_equal(bits(values), bits(want.astype(np.float32) / np.float32(255)))


def test_a_refused_call_leaves_the_other_sections_text_alone(lib):
    from list_amd import chamfer
    assert chamfer.load().list_chamfer_workspace_bytes(0, 5, 5) == 0
    before = lib.list_loss_last_error()
    assert lib.list_augment_pixel(None, None, None, None) == hip.ERR_ARG and b"rgb_in" in lib.list_augment_last_error()
    assert lib.list_loss_last_error() == before and b"B = 0" in before
