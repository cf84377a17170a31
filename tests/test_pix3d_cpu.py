"""CPU: datasets.Datasets.Pix3D on synthetic.make_pix3d_tree: the listing rules, the items, the reference's draw order, the
host image path against Pillow's own pipeline, the raw items through collate and resize.apply_cpu bit for bit against the
host path, test.py's enumeration and one CoarseNet step."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from list_amd import arguments, augment as A, resize as R, synthetic, utils
from list_amd.datasets import Datasets
from list_amd.network import executors

RES, POINTS, COARSE, VOX = 24, 200, 300, 16


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return synthetic.make_pix3d_tree(str(tmp_path_factory.mktemp("pix3d")))


def config(tree, **flags):
    fields = dict(data_dir=tree["data_dir"], catlist=["chair", "table"], sample_point_density=POINTS, coarse_point_density=COARSE,
                  vox_res=VOX, img_res=RES, cuda=False, dataset="datasets.Datasets.Pix3D")
    fields.update(flags)
    return arguments.default_config(**fields)


def dataset(tree, mode="train", **flags):
    return utils.get_class("datasets.Datasets.Pix3D")(config(tree, **flags), mode)


def bits(t):
    return np.ascontiguousarray(t, dtype=np.float32).view(np.uint32)


# ---- listing ----------------------------------------------------------------------------------------------------------------
def test_listing_rules(tree, capsys):
    ds = dataset(tree)
    assert "1/7 missing samples" in capsys.readouterr().out            # the 'flipped' name is not among the 7
    assert len(ds) == 6 and ds.skipped == 1 and [d["sample_id"] for d in ds.datalist] == list(range(6))
    for d in ds.datalist:
        cat = tree["records"][d["sample_id"]]["category"]
        assert (d["cat_id"], d["shape_id"], d["img_id"]) == (cat, tree["model_folders"][cat], f"{d['sample_id']:04d}.png")
        assert d["img_path"].endswith(os.path.join("img", cat, d["shape_id"], f"{d['sample_id']:04d}.npy"))
        assert d["mesh_path_norm"].endswith("isosurf_scaled.obj") and d["mesh_path_orig"].endswith("mesh_org.ply")
    chairs = dataset(tree, catlist=["chair"])
    assert [d["sample_id"] for d in chairs.datalist] == [0, 2, 4] and chairs.skipped == 1
    assert len(dataset(tree, catlist=["table"])) == 3 and dataset(tree, catlist=["table"]).skipped == 0
    assert len(dataset(tree, catlist=["sofa"])) == 0


def test_val_reads_the_test_split_and_a_missing_file_unlists_its_item(tree, tmp_path):
    other = synthetic.make_pix3d_tree(str(tmp_path / "t"), n_images=3)
    with open(os.path.join(other["data_dir"], "splits", "test.json"), "w") as f:
        json.dump(["img/chair/0002.png", "img/chair/0002_flipped.png"], f)
    assert [d["sample_id"] for d in dataset(other, "val").datalist] == [2] == [d["sample_id"] for d in dataset(other, "test").datalist]
    assert len(dataset(other, "train")) == 3
    os.remove(os.path.join(other["data_dir"], "data", "img", "table", other["model_folders"]["table"], "0001.npy"))
    ds = dataset(other, "train")
    assert [d["sample_id"] for d in ds.datalist] == [0, 2] and ds.skipped == 2
    os.remove(os.path.join(other["data_dir"], "data", "isosurface", "chair", other["model_folders"]["chair"], "mesh_org.ply"))
    assert len(dataset(other, "train")) == 0


# ---- items ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occ_dtype", ["float32", "uint8"])
def test_item_keys_shapes_and_dtypes(tree, occ_dtype):
    ds = dataset(tree, occ_dtype=occ_dtype)
    item = ds[1]
    assert sorted(item) == ["occ", "pc", "points", "rgb_image", "values"]
    assert item["rgb_image"].shape == (3, RES, RES) and item["rgb_image"].dtype == torch.float32
    assert item["points"].shape == (POINTS, 3) and item["values"].shape == (POINTS,) and item["pc"].shape == (COARSE, 3)
    assert all(item[k].dtype == torch.float32 for k in ("points", "values", "pc"))
    assert item["occ"].shape == (1, VOX, VOX, VOX) and item["occ"].dtype == getattr(torch, occ_dtype)
    assert set(np.unique(item["occ"].numpy()).tolist()) <= {0, 1} and float(item["occ"].sum()) > 0
    got = ds.get_testdata("table", tree["model_folders"]["table"], "0001")
    assert sorted(got) == ["gt_mesh", "pc", "rgb_image"] and got["rgb_image"].shape == (1, 3, RES, RES)
    assert got["gt_mesh"] == ds.datalist[1]["mesh_path_norm"] and os.path.exists(got["gt_mesh"]) and got["pc"].shape == (COARSE, 3)
    want = A.to_tensor(Image.fromarray(tree["images"][1]).resize((RES, RES), Image.Resampling.BILINEAR))
    assert torch.equal(got["rgb_image"][0], want)


def test_the_draws_are_the_references_sequence(tree):
    """RandomState(333); per item, per sigma one randint over its table's rows, then one randint over grid_points."""
    ds = dataset(tree)
    rng = np.random.RandomState(333)
    counts = np.rint(np.asarray([0.5, 0.49, 0.01]) * POINTS).astype(np.uint32)
    for index in (3, 0, 3):
        item = ds[index]
        tables = np.load(os.path.splitext(ds.datalist[index]["query_path"])[0] + ".npz")
        rows = []
        for s, num in zip((0.003, 0.01, 0.07), counts):
            q = tables[f"query_points_sigma_{s}"]
            rows.extend(q[rng.randint(0, q.shape[0], num)])
        rows = np.asarray(rows, dtype=np.float32)
        pc = tables["grid_points"][rng.randint(0, tables["grid_points"].shape[0], COARSE)]
        assert np.array_equal(item["points"].numpy(), rows[:, :3]) and np.array_equal(item["values"].numpy(), rows[:, 3])
        assert np.array_equal(item["pc"].numpy(), pc.astype(np.float32))


def test_an_image_that_is_not_uint8_hw3_is_refused_by_name(tree, tmp_path):
    other = synthetic.make_pix3d_tree(str(tmp_path / "t"), n_images=2)
    ds = dataset(other)
    for bad in (np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.uint8), np.zeros((4, 5, 4), np.uint8)):
        np.save(ds.datalist[0]["img_path"], bad)
        with pytest.raises(ValueError, match="0000.npy"):
            ds[0]


# ---- the image paths ----------------------------------------------------------------------------------------------------------
def pillow_pipeline(pixels, flip, params):
    img = Image.fromarray(pixels)
    if flip:
        img = img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    if params is not None:
        img = A.jitter_pil(img, params)
    return A.to_tensor(img.resize((RES, RES), Image.Resampling.BILINEAR))


def test_host_path_is_pillows_own_pipeline_and_the_device_form_equals_it_bit_for_bit(tree):
    """Host mode: the coin, the jitter draws, Pillow's operations, Pillow's resize.  Hip mode hands out the raw pixels and
    draws nothing; collate packs them and resize.apply_cpu under the same parameters gives the host path's tensors."""
    host = dataset(tree, color_jitter=True, random_h_flip=True)
    raw = dataset(tree, color_jitter=True, random_h_flip=True, augment="hip")
    host_items, records, flipped = [], [], 0
    for i in range(6):
        random.seed(40 + i)
        host_items.append(host[i]["rgb_image"])
        random.seed(40 + i)
        flip = random.random() < 0.5
        flipped += flip
        p = A.draw_jitter(random)
        assert torch.equal(host_items[-1], pillow_pipeline(tree["images"][i], flip, p)), i
        p["ops"] |= A.FLIP if flip else 0
        records.append(p)
    assert 0 < flipped < 6
    state = random.getstate()
    raw_items = [raw[i] for i in range(6)]
    assert random.getstate() == state                                  # hip mode draws nothing
    for i, item in enumerate(raw_items):
        assert item["rgb_image"].dtype == torch.uint8 and np.array_equal(item["rgb_image"].numpy(), tree["images"][i])
    batch = Datasets.collate(raw_items)
    ragged = batch["rgb_image"]
    assert isinstance(ragged, R.RaggedImages) and ragged.sizes.tolist() == [list(tree["images"][i].shape[:2]) for i in range(6)]
    assert batch["points"].shape == (6, POINTS, 3) and batch["pc"].shape == (6, COARSE, 3) and batch["occ"].shape == (6, 1, VOX, VOX, VOX)
    got = R.apply_cpu(ragged, RES, RES, np.concatenate(records))
    assert np.array_equal(bits(got), bits(torch.stack(host_items).numpy()))
    # without the flags: plain resize on both sides; test mode is the host resize in either mode
    plain_host, plain_raw = dataset(tree), dataset(tree, augment="hip")
    got = R.apply_cpu(Datasets.collate([plain_raw[i] for i in range(6)])["rgb_image"], RES, RES)
    assert np.array_equal(bits(got), bits(torch.stack([plain_host[i]["rgb_image"] for i in range(6)]).numpy()))
    assert torch.equal(dataset(tree, "test", augment="hip", color_jitter=True)[2]["rgb_image"], pillow_pipeline(tree["images"][2], False, None))


def test_collate_leaves_float_batches_to_default_collate(tree):
    ds = dataset(tree)
    batch = Datasets.collate([ds[0], ds[1]])
    assert isinstance(batch["rgb_image"], torch.Tensor) and batch["rgb_image"].shape == (2, 3, RES, RES)
    loader = torch.utils.data.DataLoader(dataset(tree, augment="hip"), batch_size=3, collate_fn=Datasets.collate)
    sizes = [b["rgb_image"].sizes.tolist() for b in loader]
    assert len(sizes) == 2 and all(isinstance(b["rgb_image"], R.RaggedImages) for b in loader) and sizes[0][2] == [120, 31]


# ---- the entry points -------------------------------------------------------------------------------------------------------
def test_test_py_enumerates_the_datalist_by_image_stem(tree):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "learning-implicitly-from-spatial-transformers-network_amd"))
    from list_amd import test as T
    ds = dataset(tree, "test")
    items = T.test_items(ds)
    assert items == [{"cat_id": d["cat_id"], "shape_id": d["shape_id"], "cam_id": f"{d['sample_id']:04d}"} for d in ds.datalist]
    batch = ds.get_testdata(items[4]["cat_id"], items[4]["shape_id"], items[4]["cam_id"])
    assert batch["rgb_image"].shape == (1, 3, RES, RES)
    synthetic_ds = Datasets.SyntheticIM2SDF(arguments.default_config(synthetic_len=5), "test")
    assert T.test_items(synthetic_ds) == [{"cat_id": "synthetic", "shape_id": f"{i:04d}", "cam_id": i} for i in range(2)]


@pytest.mark.parametrize("mode", ["host", "hip"])
def test_a_coarsenet_epoch_on_the_tree(tree, mode):
    from list_amd import train as TR
    torch.manual_seed(0)
    cfg = config(tree, model="network.models.CoarseNet", img_res=32, augment=mode, color_jitter=True, random_h_flip=True,
                 train_batch_size=3, max_steps=2, plot_every_batch=1, epochs=1, exp_name="pix3d_cpu")
    cfg.device = torch.device("cpu")
    model = TR._Module(utils.get_class(cfg.model)(cfg))
    ds = utils.get_class(cfg.dataset)(cfg, "train")
    loader = torch.utils.data.DataLoader(ds, batch_size=3, drop_last=True, collate_fn=Datasets.collate)
    ex = executors.CoarseNet(cfg, model)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-4)
    before = [p.detach().clone() for p in model.parameters()]
    loss = TR.train_epoch(0, ex, optimizer, loader, cfg)
    assert np.isfinite(loss) and any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    # the executor's test takes the dataset's dict as well as the tuple
    model.eval()
    got = ds.get_testdata("chair", tree["model_folders"]["chair"], "0000")
    pred, score = ex.test(got, eval_pred=True)
    pred2, score2 = ex.test((got["rgb_image"], got["pc"].unsqueeze(0)), eval_pred=True)
    assert pred.shape[0] == 1 and torch.equal(pred, pred2) and score == score2 and np.isfinite(score["chamfer_l2"])
