#!/usr/bin/env python3
"""Time the 3-D occupancy encoder (not part of bench.py): the torch fp32 module, the torch module under autocast fp16
(MIOpen's half kernels) and the HIP encoder (list_amd.voxenc), same process, same weights (oracle.fill.fill_state), at
B = 1 and B = 8, R = 128, runs interleaved; then LIST.encode() as a whole with each encoder, and the HIP path's time
per launch.  Prints one JSON line.

    python tools/voxenc_bench.py [--iters 20] [--warmup 3] [--rounds 3] [--out voxenc_bench.json]

Times are HIP events around whole calls (Python included), median of --iters after --warmup calls, the smallest median
over --rounds interleaved rounds.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch        # noqa: E402

from _timing import interleaved  # noqa: E402

DEV = "cuda:0"
R = 128
LAYERS = [1, 1, 1, 1, 16, 32, 64, 128, 128]


def point_occ(B, n=2048, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ijk = torch.clamp((torch.randn(B, n, 3, generator=g) * 0.15 + 0.5) * (R - 1) + 0.5, 0, R - 1).long()
    occ = torch.zeros(B, R ** 3)
    occ.scatter_(1, (ijk[..., 0] * R + ijk[..., 1]) * R + ijk[..., 2], 1.0)
    return occ.view(B, R, R, R).to(DEV)


def conv_flop(layers, stage, second, D):
    cin = layers[stage + 1] if second else layers[stage]
    return 2.0 * 27 * cin * layers[stage + 1] * D ** 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from oracle import fill
    from list_amd import arguments, utils, voxenc
    result = {"R": R, "device": torch.cuda.get_device_name(0)}
    LIST = utils.get_class("network.models.LIST")
    nets = {}
    for name, kw in (("torch_fp32", {}), ("torch_amp_fp16", {"vox_encoder_precision": "fp16"}),
                     ("hip", {"vox_encoder": "hip"})):
        cfg = arguments.default_config(vox_res=R, train_batch_size=8, precision="fp16", img_res=224, **kw)
        nets[name] = fill.fill_state(LIST(cfg), seed=2).to(DEV).eval()
    for B in (1, 8):
        occ = point_occ(B)
        img = torch.rand((B, 3, 224, 224), device=DEV)
        with torch.no_grad():
            for net in nets.values():
                net.encode(img)                           # memory formats, MIOpen's kernel search, the weight pack
            enc = nets["torch_fp32"].vox_encoder
            packed = voxenc.pack(nets["hip"].vox_encoder)

            def amp():
                with torch.autocast("cuda", dtype=torch.float16):
                    return nets["torch_amp_fp16"].vox_encoder(occ)
            t = interleaved({"torch_fp32": lambda: enc(occ), "torch_amp_fp16": amp,
                             "hip": lambda: voxenc.encode(occ, packed)}, args.iters, args.warmup, args.rounds)
            te = interleaved({k: (lambda n=n: n.encode(img)) for k, n in nets.items()}, args.iters, args.warmup,
                             args.rounds)
            steps = voxenc.time_steps(occ, packed)
        names = voxenc.step_names(LAYERS)
        print(f"B = {B}: vox_encoder  torch fp32 {t['torch_fp32']:.3f} ms   autocast fp16 {t['torch_amp_fp16']:.3f} ms   "
              f"HIP {t['hip']:.3f} ms   ({t['torch_amp_fp16'] / t['hip']:.2f}x over autocast)")
        print(f"B = {B}: encode()     torch fp32 {te['torch_fp32']:.3f} ms   autocast fp16 {te['torch_amp_fp16']:.3f} ms   "
              f"HIP {te['hip']:.3f} ms")
        rows = []
        for i, (nm, ms) in enumerate(zip(names, steps)):
            row = {"layer": nm, "ms": round(ms, 4)}
            if i >= 4:                                    # an MFMA convolution
                stage, second = 3 + (i - 3) // 2, (i - 3) % 2 == 1
                D = R >> (stage - 3)
                cin = LAYERS[stage + 1] if second else LAYERS[stage]
                fl = B * conv_flop(LAYERS, stage, second, D)
                by = B * D ** 3 * 2 * (cin + LAYERS[stage + 1] * (1.125 if second and stage < 7 else 1))
                row.update(tflops=round(fl / ms * 1e-9, 1), gb_per_s=round(by / ms * 1e-6, 1))
            rows.append(row)
            print(f"    {nm:10s} {ms:8.4f} ms" + (f"   {row['tflops']:7.1f} TFLOP/s  {row['gb_per_s']:7.1f} GB/s"
                                                  if "tflops" in row else ""))
        result[f"B{B}"] = {"vox_encoder_ms": t, "encode_ms": te, "hip_steps": rows,
                           "speedup_over_autocast": t["torch_amp_fp16"] / t["hip"],
                           "speedup_over_fp32": t["torch_fp32"] / t["hip"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
