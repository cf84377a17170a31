#!/usr/bin/env python3
"""Time the image encoder (not part of bench.py): the torch ResEncoder in fp32 channels-last, the same module under
autocast fp16 (MIOpen's half kernels) and the HIP encoder (list_amd.imgenc), same process, same weights
(oracle.fill.fill_state), at B = 1 and B = 8, 224^2, runs interleaved; then LIST.encode() as a whole with the flag off
and on, and the HIP path's time per launch with TFLOP/s and GB/s.  Prints one JSON line.

    python tools/imgenc_bench.py [--iters 20] [--warmup 3] [--rounds 3] [--out imgenc_bench.json]

Times are HIP events around whole calls (Python included), median of --iters after --warmup calls, the smallest median
over --rounds interleaved rounds.  The baselines are the torch columns of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch        # noqa: E402

from _timing import interleaved  # noqa: E402

DEV = "cuda:0"
RES = 224


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
    from list_amd import arguments, imgenc, utils
    result = {"res": RES, "device": torch.cuda.get_device_name(0)}
    LIST = utils.get_class("network.models.LIST")
    nets = {}
    for name, kw in (("torch", {}), ("hip", {"img_encoder": "hip"})):
        cfg = arguments.default_config(vox_res=128, train_batch_size=8, precision="fp16", img_res=RES, **kw)
        nets[name] = fill.fill_state(LIST(cfg), seed=2).to(DEV).eval()
    for B in (1, 8):
        img = torch.rand((B, 3, RES, RES), device=DEV)
        with torch.no_grad():
            for net in nets.values():
                net.encode(img)                           # memory formats, MIOpen's kernel search, the weight pack
            enc = nets["torch"].im_encoder2               # (channels-last after the first encode())
            img_cl = img.contiguous(memory_format=torch.channels_last)
            packed = imgenc.pack(nets["hip"].im_encoder2)

            def amp():
                with torch.autocast("cuda", dtype=torch.float16):
                    return enc(img_cl)
            t = interleaved({"torch_fp32_cl": lambda: enc(img_cl), "torch_amp_fp16": amp,
                             "hip": lambda: imgenc.encode(packed, img_cl)}, args.iters, args.warmup, args.rounds)
            te = interleaved({k: (lambda n=n: n.encode(img)) for k, n in nets.items()}, args.iters, args.warmup,
                             args.rounds)
            steps = imgenc.time_steps(packed, img_cl)
        print(f"B = {B}: ResEncoder   torch fp32 channels-last {t['torch_fp32_cl']:.3f} ms   autocast fp16 "
              f"{t['torch_amp_fp16']:.3f} ms   HIP {t['hip']:.3f} ms   ({t['torch_amp_fp16'] / t['hip']:.2f}x over autocast, "
              f"{t['torch_fp32_cl'] / t['hip']:.2f}x over fp32)")
        print(f"B = {B}: encode()     --img_encoder torch {te['torch']:.3f} ms   --img_encoder hip {te['hip']:.3f} ms")
        rows = []
        for nm, ms, fl, by in zip(imgenc.step_names(), steps, imgenc.step_flops(B, RES, RES), imgenc.step_bytes(B, RES, RES)):
            rows.append({"launch": nm, "ms": round(ms, 4), "tflops": round(fl / ms * 1e-9, 1),
                         "gb_per_s": round(by / ms * 1e-6, 1)})
            print(f"    {nm:15s} {ms:8.4f} ms   {rows[-1]['tflops']:7.1f} TFLOP/s  {rows[-1]['gb_per_s']:7.1f} GB/s")
        print(f"    sum of launches {sum(steps):8.4f} ms")
        result[f"B{B}"] = {"encoder_ms": t, "encode_ms": te, "hip_steps": rows, "hip_steps_sum_ms": sum(steps),
                           "speedup_over_autocast": t["torch_amp_fp16"] / t["hip"],
                           "speedup_over_fp32": t["torch_fp32_cl"] / t["hip"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
