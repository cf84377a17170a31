"""The coarse stage (tree decoder, point MLP, camera, occupancy) in torch and in HIP (list_amd.coarse), at B = 1 and 8,
R = 128, the default decoder: stage time by events, per-launch times, the last tree layer as GB/s of W_branch read,
and encode_ms of the whole model with --coarse_stage off and on.
usage: python tools/coarse_bench.py [--reps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from list_amd import arguments, coarse, utils          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(333)


def timed(fn, reps):
    """Median milliseconds of fn between two events, after two warm-up calls."""
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


print(f"device: {torch.cuda.get_device_name(0)}; median of {args.reps} event-timed calls")
for B in (1, 8):
    cfg = arguments.default_config(vox_res=128, train_batch_size=B, precision="fp16", img_res=224)
    net = utils.get_class("network.models.LIST")(cfg).to(dev).eval()
    hipnet = utils.get_class("network.models.LIST")(
        arguments.default_config(vox_res=128, train_batch_size=B, precision="fp16", img_res=224, coarse_stage="hip"))
    hipnet.load_state_dict(net.state_dict())
    hipnet.to(dev).eval()
    img = torch.rand((B, 3, 224, 224), device=dev)
    with torch.no_grad():
        feat_g, _ = net.im_encoder(img)
        feat_g2, _ = net.im_encoder2(net._apply_memory_format(img)[0])
        packed = coarse.pack(net)

        def torch_stage():
            pc = net.point_decoder([feat_g.unsqueeze(1)])
            code = torch.max(net.point_mlp_coarse(pc), -1)[0].reshape(B, -1)
            tm = net.spatial_transformer(torch.cat([code, feat_g2.reshape(B, -1)], dim=1)).reshape(-1, 4, 3)
            return pc, code, tm, net.create_occ(pc)

        def hip_stage():
            return coarse.decode(packed, feat_g, feat_g2, cfg.vox_res, cfg.bb_min, cfg.bb_max)

        ref, got = torch_stage(), hip_stage()
        t_torch, t_hip = timed(torch_stage, args.reps), timed(hip_stage, args.reps)
        t_dec = timed(lambda: net.point_decoder([feat_g.unsqueeze(1)]), args.reps)
        print(f"\nB = {B}, R = {cfg.vox_res}, P = {ref[0].shape[1]}")
        print(f"  max|pc_hip - pc_torch| = {float((got[0] - ref[0]).abs().max()):.3e}, max|trans_mat diff| = "
              f"{float((got[2] - ref[2]).abs().max()):.3e}, voxels that differ = {int((got[3] != ref[3]).sum())}")
        print(f"  torch stage {t_torch:8.3f} ms   (its TreeGraphDecoder alone {t_dec:8.3f} ms)")
        print(f"  HIP stage   {t_hip:8.3f} ms   ({t_torch / t_hip:.2f}x)"
              + ("" if t_hip < t_torch else "   -- the HIP stage is NOT faster here"))
        steps = coarse.time_steps(packed, feat_g, feat_g2, cfg.vox_res, reps=args.reps)
        names = coarse.step_names(packed.shape)
        for n, t in zip(names, steps):
            print(f"    {n:10s} {t * 1e3:9.1f} us")
        last = packed.branches[-1]
        gb = last.numel() * 4 / 1e9
        print(f"  tree_{len(packed.branches) - 1}: W_branch {gb * 1e3:.1f} MB read once per {coarse.GROUP} images -> "
              f"{gb / (steps[len(packed.branches) - 1] * 1e-3):.0f} GB/s")
        e_off = timed(lambda: net.encode(img), args.reps)
        e_on = timed(lambda: hipnet.encode(img), args.reps)
        print(f"  encode_ms, whole model: --coarse_stage torch {e_off:8.3f}   hip {e_on:8.3f}")
    del net, hipnet, packed
    torch.cuda.empty_cache()
