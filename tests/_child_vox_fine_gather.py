"""The cases of tests/test_vox_fine_gather_bits_gpu.py: voxel pyramids whose levels all take k_gather_vox (a stencil
displacement of one voxel and more), sampled at a few hundred awkward points; returns (or, run as a program, writes as
JSON) the SHA-256 of the raw bits of every level's feature columns and of the SDF.  Everything is made from the seeded
generators of list_amd.synthetic, so the digests belong to the arithmetic alone."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from list_amd import synthetic as synth          # noqa: E402

B, N = 2, 300                                    # 600 rows: two whole 256-row tiles and a ragged one
# (C, D, H, W) per level.  The scalar level shares the grid of the level behind it, so that level's kernel carries it
# (TailRide).  Displacements in voxels (0.0722 * (size - 1) / 2): 56 -> 1.985, 40 -> 1.41, 32 -> 1.119, 29 -> 1.01, 57 -> 2.02
PYRAMIDS = {
    "cubes": [(1, 56, 56, 56), (16, 56, 56, 56), (32, 40, 40, 40), (64, 32, 32, 32), (64, 29, 29, 29), (16, 57, 57, 57)],
    "bricks": [(1, 24, 40, 32), (64, 24, 40, 32), (8, 33, 31, 30), (16, 30, 33, 31), (128, 29, 35, 31), (256, 31, 29, 30)],
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.view(np.uint8).tobytes()).hexdigest()


def lattice_coordinate(i, size):
    """The query coordinate that axis_setup (csrc/point_math.h) un-normalises to i, as nearly as float32 has it:
    v = ((2 q + 1) / 2) * (size - 1)."""
    return np.float32(0.5) * (np.float32(2.0 * i / (size - 1)) - np.float32(1.0))


def make_query(seed, shapes):
    q = synth.make_query(seed, B, N).astype(np.float32)
    sizes = sorted({s for sh in shapes for s in sh[1:]})
    row = 0
    for size in sizes:                           # lattice positions (f == 0) and one float32 step to either side
        for i in (0, 1, size // 2, size - 2, size - 1):
            c = lattice_coordinate(i, size)
            for v in (c, np.nextafter(c, np.float32(-1)), np.nextafter(c, np.float32(1))):
                q[0, row % N, row % 3] = v
                q[1, (row + 7) % N, (row + 1) % 3] = v
                row += 1
    # on and beyond the faces of the volume (|2 q| >= 1), corners included
    faces = np.array([[s0, s1, s2] for s0 in (-0.5, 0.5) for s1 in (-0.5, 0.6) for s2 in (-0.75, 0.5)], np.float32)
    q[0, N - 8:] = faces
    q[1, N - 8:] = faces[::-1]
    q[1, N - 9] = (0.5, 0.1, -0.2)
    q[0, N - 10, 1] = np.nan                     # one NaN coordinate: ATen clips it to size - 1
    return q


def make_maps(seed, shapes):
    maps = [synth.uniform(seed + 1000, (B,) + shapes[0])]
    maps += [synth.normalish(seed + 1000 + 13 * i, (B,) + s) for i, s in enumerate(shapes[1:], 1)]
    return maps


def spoil(maps, q):
    """+-inf and NaN voxels where taps land: around the base voxel of a few query points, and on the border planes that
    the skipped (index == size) taps read in their place."""
    maps = [m.copy() for m in maps]
    bad = (np.inf, -np.inf, np.nan)
    for l, m in enumerate(maps):
        D, H, W = m.shape[2:]
        for n, j in enumerate((3, 57, 140, 222, N - 3, N - 6)):
            x, y, z = (2.0 * q[0, j, 2], 2.0 * q[0, j, 1], 2.0 * q[0, j, 0])          # perm (2, 1, 0), scale 2
            ix, iy, iz = (int(np.clip(np.floor((c + 1) / 2 * (s - 1)), 0, s - 1)) for c, s in ((x, W), (y, H), (z, D)))
            m[0, (n + l) % m.shape[1], iz, iy, min(ix + (n & 1), W - 1)] = bad[(n + l) % 3]
        m[1, 0, D - 1, H - 1, W - 1] = bad[l % 3]
        m[1, m.shape[1] - 1, 0, H - 1, 0] = bad[(l + 1) % 3]
    return maps


def run():
    import __graft_entry__ as ge
    ge.build()
    from list_amd import hip
    out = {}
    seed = 4242
    tm = dev(synth.make_trans_mat(seed, B))
    img_maps = [dev(m) for m in synth.make_img_maps(seed, B, 224)]
    for name, shapes in PYRAMIDS.items():
        q = make_query(seed, shapes)
        maps = make_maps(seed, shapes)
        chans = [s[0] for s in shapes]
        for prec in ("fp16", "bf16x3"):
            md = hip.map_dtype_for(prec)
            img = hip.prep_img_maps(img_maps, dtype=md)
            weights = {k: dev(v) for k, v in synth.make_mlp_weights(seed, 7 * sum(chans) + img.channels + 3).items()}
            for kind, these in (("clean", maps), ("spoiled", spoil(maps, q))):
                vox = hip.prep_vox_maps([dev(m) for m in these], dtype=md)
                packed = hip.prep_mlp_weights(weights, vox.channels, img.channels, prec)
                tag = f"{name}/{prec}/{kind}"
                if kind == "clean":              # the feature matrix itself, level by level (reference order: (cbase + c) * 7 + j)
                    feats = hip.gather_features(dev(q), tm, img, vox, packed).cpu().numpy()
                    lo = 0
                    for l, c in enumerate(chans):
                        out[f"{tag}/features_l{l}"] = digest(feats[:, lo:lo + 7 * c])
                        lo += 7 * c
                    out[f"{tag}/features_rest"] = digest(feats[:, lo:])          # the 2-D sample and xyz
                for sort in (True, False):       # spoiled maps: through the exact redo of the flagged tiles
                    sdf = hip.sdf_query(dev(q), tm, img, vox, packed, precision=prec, sort_points=sort)
                    out[f"{tag}/sdf_{'sorted' if sort else 'unsorted'}"] = digest(sdf.cpu().numpy())
                if kind == "clean":
                    sdf, _ = hip.sdf_query(dev(q), tm, img, vox, packed, precision=prec, save_for_backward=True)
                    out[f"{tag}/sdf_training_forward"] = digest(sdf.cpu().numpy())
    return out


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(run(), f, indent=1, sort_keys=True)
        f.write("\n")
