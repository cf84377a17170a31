"""Child process of tests/test_fc0_sampled_epilogue_gpu.py: the SDF of a fixed list of fp16 queries on
list_prep_img_proj's map, written to an .npz.  argv: output file, 'sampled' (the default dispatch: k_gather_img on the
kept channels + k_gemm_nt_pp with the sampling epilogue) or 'rowvec' (ListQueryArgs.no_fused_fc0 = 1: k_gather_img
writes row vectors, k_gemm_nt_pp adds them).  The parent compares the two files bit for bit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases                     # noqa: E402  (inputs of the parity cases: test infrastructure)
from list_amd import synthetic as synth      # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class Side:
    def __init__(self, hip, fused):
        self.hip, self.fused, self.res = hip, fused, {}

    def prepare(self, c, map_size):
        hip = self.hip
        vox = hip.prep_vox_maps([dev(m) for m in c["vox_maps"]], "f16")
        packed = hip.prep_mlp_weights({k: dev(v) for k, v in c["weights"].items()}, vox.channels, 1024, "fp16")
        img = hip.prep_img_proj([dev(m) for m in c["img_maps"]], packed, map_size, "fp16")
        return img, vox, packed

    def query(self, prep, q, T, clamp_hi, sort=True, plan=None):
        img, vox, packed = prep
        return self.hip.sdf_query(q, T, img, vox, packed, precision="fp16", clamp_hi=clamp_hi, sort_points=sort,
                                  plan=plan, fused_fc0=self.fused).cpu().numpy()

    def case(self, tag, c, map_size=137, clamp_hi=136.0, sorts=(True, False), split=False):
        prep = self.prepare(c, map_size)
        q, T = dev(c["query"]), dev(c["trans_mat"])
        for sort in sorts:
            plan = {}
            self.res[f"{tag}_{'sorted' if sort else 'unsorted'}"] = self.query(prep, q, T, clamp_hi, sort, plan)
            for k in ("fused_fc0", "img_proj", "fc0_k", "chunks"):
                self.res[f"{tag}_plan_{k}"] = np.int32(plan[k])
        if split:       # the query axis in two calls: every row tile holds other points than in the one call
            half = q.shape[1] // 2
            self.res[f"{tag}_split"] = np.concatenate([self.query(prep, q[:, :half].contiguous(), T, clamp_hi),
                                                       self.query(prep, q[:, half:].contiguous(), T, clamp_hi)], 1)


def main(out_path, side):
    import __graft_entry__ as ge
    ge.build()
    from list_amd import hip
    s = Side(hip, fused=(side == "sampled"))
    for name in ("tiny", "small", "real", "edge") + tuple(cases.NONFINITE_CASE_NAMES):
        s.case(name, cases.build_case(name), split=(name == "small"))
    # NaN coordinates (the point's 256-row tile takes the exact redo), projections piled onto and beyond the clamp
    c = dict(cases.build_case("small"))
    q = np.array(c["query"], copy=True)
    q[0, 3, 1] = np.nan
    s.case("small_nan_coord", dict(c, query=q))
    T = np.array(c["trans_mat"], copy=True)
    T[:, :3, :2] *= 8.0
    s.case("small_on_clamp", dict(c, trans_mat=T))
    seed = 2024
    for tag, B, N, img_res, ms, hi in (("config2", 8, 20000, 224, 137, 136.0), ("config5", 8, 50000, 512, 274, 273.0)):
        c = {"query": synth.make_query(seed, B, N), "img_maps": synth.make_img_maps(seed, B, img_res),
             "vox_maps": synth.make_vox_maps(seed, B, 128), "weights": synth.make_mlp_weights(seed),
             "trans_mat": synth.make_trans_mat(seed, B) * (np.array([[[ms / 137.0, ms / 137.0, 1.0]]], np.float32))}
        s.case(tag, c, ms, hi, split=True)
    np.savez(out_path, **s.res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
