#!/usr/bin/env python3
"""Inference entry point (test.py of the reference): for every test item, evaluate the SDF on the
query grid with the HIP path and extract the iso-surface on the GPU (mesh.marching_cubes), written as
<results_dir>test_objs/<cat>/<shape>_<cam>_pred.obj.

    python test.py --model network.models.LIST --dataset datasets.Datasets.SyntheticIM2SDF -e run1 \
        --mcube_znum 256
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 test.py ...    # query axis sharded over GPUs

`--refine_stride s` (2, 4, 8) queries the coarse-to-fine grid of refine.py instead of every grid point: the stride-s
lattice and the fine points near the surface, the rest interpolated (`--refine_band` sets how near).
`--mesh_components K` / `--mesh_min_faces N` drop floating fragments (components.py) and `--mesh_simplify C` then merges
the vertices of every cell of a C^3 grid over the box (simplify.py: vertex clustering on the device); what is saved is
what is rendered and scored.  `--save_volume`
also writes the [res,res,res] SDF volume (<stem>_sdf.npy; with --refine_stride the filled one).  `--render_pred view|canonical|both`
renders the mesh on the device (render.py) from the model's own camera over the input image (<stem>_pred_view.png) and / or
along the three array axes (<stem>_pred_x.png, _y, _z), at `--render_size` pixels a side.  `--eval_pred` scores
every item whose dataset gives a ground-truth mesh (evaluate.eval_mesh on the device: Chamfer-L2, precision / recall / F-score, IoU) and
writes <results_dir>test_objs/<cat>.csv, one row per item and a final `Mean` row, as the reference does; items without
one (the synthetic datasets) are reported as skipped."""
import csv
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
import list_amd                                          # noqa: E402
from list_amd import arguments, evaluate, mesh, render, utils   # noqa: E402
from list_amd.train import wrap_model                   # noqa: E402

import numpy as np                                       # noqa: E402
import torch                                             # noqa: E402
import torch.distributed as dist                         # noqa: E402


def write_scores(path, rows):
    """rows: [(ID, {metric: value})] -> the reference's CSV (pandas' to_csv of its DataFrame: an index column, `ID`,
    the metrics, then a `Mean` row over the items), values rounded to 5 digits."""
    keys = []
    for _, score in rows:
        keys += [k for k in score if k not in keys]
    mean = {}
    for k in keys:
        vals = [score[k] for _, score in rows if k in score and not np.isnan(score[k])]
        mean[k] = float(np.mean(vals)) if vals else float("nan")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "ID"] + keys)
        for i, (ident, score) in enumerate(rows + [("Mean", mean)]):
            w.writerow([i, ident] + [round(score[k], 5) if k in score else "" for k in keys])
    return mean


def test_items(dataset):
    """What is tested when no test list is given: every entry of a dataset whose `datalist` carries 'img_id' (Pix3D; the
    camera id is the image's stem, as in the reference's test.py), else the first two synthetic items."""
    entries = getattr(dataset, "datalist", None) or []
    if entries and all("img_id" in d for d in entries):
        return [{"cat_id": d["cat_id"], "shape_id": d["shape_id"], "cam_id": d["img_id"].split(".")[0]} for d in entries]
    return [{"cat_id": "synthetic", "shape_id": f"{i:04d}", "cam_id": i} for i in range(min(len(dataset), 2))]


def test_all(config, save_volume=None, eval_pred=None):
    save_volume = getattr(config, "save_volume", False) if save_volume is None else save_volume
    eval_pred = getattr(config, "eval_pred", False) if eval_pred is None else eval_pred
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        dist.init_process_group("nccl")
    torch.cuda.set_device(local_rank if world > 1 else config.gpu)
    config.device = torch.device("cuda", torch.cuda.current_device())
    model = utils.get_class(config.model)(config).to(config.device)
    ck = config.checkpoint_dir + config.test_checkpoint
    if os.path.exists(ck):
        utils.load_model(ck, model)
        print("loaded", ck)
    else:
        print("no checkpoint at", ck, "- running with the initial weights")
    model = wrap_model(model, config).eval()
    executor = utils.get_class(config.model.replace("model", "executor"))(config, model)
    dataset = utils.get_class(config.dataset)(config, "test")
    out_dir = utils.ensure_dir(config.results_dir + "test_objs/")
    items = config.testlist or test_items(dataset)
    rank0 = (not dist.is_initialized()) or dist.get_rank() == 0
    scores = {}                                          # cat -> [(ID, score)]
    for it in items:
        batch = dataset.get_testdata(it["cat_id"], it["shape_id"], it["cam_id"])
        t0 = time.time()
        stride = getattr(config, "refine_stride", 0)
        if stride:
            volume, _, _ = executor.predict_grid(batch["rgb_image"].to(config.device), batch.get("transmat"),
                                                 refine=stride, band=getattr(config, "refine_band", None))
        else:
            volume, _, _ = executor.predict_grid(batch["rgb_image"].to(config.device), batch.get("transmat"))
        torch.cuda.synchronize()
        dt = time.time() - t0
        if rank0:
            if stride:
                st = executor.last_grid_stats
                print(f"{it['cat_id']}/{it['shape_id']}: {st['queried']} queries = {100.0 * st['fraction']:.2f} % of "
                      f"the {volume.numel()} grid points (stride {stride}) in {dt:.3f} s "
                      f"({volume.numel() / dt / 1e6:.2f} M grid points/s incl. encoders)")
            else:
                print(f"{it['cat_id']}/{it['shape_id']}: {volume.numel()} queries in {dt:.3f} s "
                      f"({volume.numel() / dt / 1e6:.2f} M points/s incl. encoders)")
            stem = utils.ensure_dir(out_dir + it["cat_id"] + "/") + f"{it['shape_id']}_{it['cam_id']}"
            if save_volume:
                np.save(stem + "_sdf.npy", volume.cpu().numpy())
            t0 = time.time()
            executor.last_components = executor.last_simplify = None
            m = mesh.Mesh(*executor.filter_mesh(*mesh.marching_cubes(volume, 0.0, -0.5, 0.5)))
            dt = time.time() - t0
            t0 = time.time()
            m.export(stem + "_pred.obj")
            dt_obj = time.time() - t0
            print(f"  mesh: {len(m.vertices)} vertices, {len(m.faces)} faces in {dt * 1e3:.1f} ms -> {stem}_pred.obj "
                  f"({os.path.getsize(stem + '_pred.obj')} bytes written in {dt_obj * 1e3:.1f} ms)")
            if getattr(config, "render_pred", "none") != "none":
                t0 = time.time()
                views = executor.render_views(batch, m)
                for name, img in views.items():
                    render.save_png(f"{stem}_pred_{name}.png", img)
                print(f"  rendered {', '.join(views)} at {executor.render_size}^2 in {(time.time() - t0) * 1e3:.1f} ms "
                      f"-> {stem}_pred_<view>.png")
            cc = executor.last_components
            if cc is not None:
                print(f"  components: {cc['K']} found, {len(cc['kept'])} kept, {cc['dropped_faces']} faces dropped")
            sp = executor.last_simplify
            if sp is not None:
                print(f"  simplified on {config.mesh_simplify}^3 cells: {len(sp['vertex_map'])} vertices in {sp['clusters']} "
                      f"clusters, {sp['degenerate_faces']} faces collapsed")
            if eval_pred:
                gt = batch.get("gt_mesh")
                if gt is None:
                    print("  eval: skipped (the dataset gives no ground-truth mesh)")
                    continue
                t0 = time.time()
                score = executor.eval(m, gt)
                dt = time.time() - t0
                scores.setdefault(it["cat_id"], []).append((f"{it['shape_id']}_{str(it['cam_id']).zfill(2)}", score))
                print(f"  eval in {dt * 1e3:.1f} ms: " + ", ".join(f"{k}: {v:.5f}" for k, v in score.items()))
    for cat, rows in scores.items():
        mean = write_scores(out_dir + cat + ".csv", rows)
        print(f"{config.exp_name} {cat} Mean ({len(rows)} items): " + ", ".join(f"{k}: {v:7.3f}" for k, v in mean.items())
              + f" -> {out_dir}{cat}.csv")
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    test_all(arguments.get_args())
