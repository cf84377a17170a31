"""Generate tests/golden/eval_ref.npz by RUNNING THE REFERENCE's inside test and point-cloud metrics (TEST
INFRASTRUCTURE; the authoring container only, see oracle/ref_eval.py for how the reference is built and imported).

    python -m oracle.gen_eval_golden            # write the fixture
    python -m oracle.gen_eval_golden --check    # recompute everything and compare with the committed file

Per case of tests/_eval_cases.py (the reference sees the case's float32 vertices widened to float64):
    <case>.contains, <case>.hole    packed bits of check_mesh_contains(mesh, points, hash_res)
    <case>.occ, <case>.rest         packed bits of implicit_waterproofing(mesh, points): occupancy, holes left after the retries
    <case>.counts                   int64 [5]: Q and the four popcounts
    <case>.sha256                   of the bytes of verts, faces, points and hash_res
Per pair of point clouds:
    pc.<pair>.keys, pc.<pair>.values   the reference's eval_pointcloud dict (float64);  pc.<pair>.sha256
Inputs are not stored.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "eval_ref.npz")


def compute():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _eval_cases as EC
    from . import ref_eval
    R = ref_eval.load()
    out = {}
    with np.errstate(invalid="ignore"):                            # the NaN and infinite query points
        for name in EC.CASE_NAMES:
            c = EC.build(name)
            mesh = R.Mesh(c.verts.astype(np.float64), c.faces.astype(np.int64))
            contains, hole = R.check_mesh_contains(mesh, c.points.copy(), c.res)
            occ, rest = R.implicit_waterproofing(mesh, c.points.copy(), c.res)
            flags = dict(zip(EC.FLAG_KEYS, (contains, hole, occ, rest)))
            counts = [len(c.points)] + [int(np.count_nonzero(flags[k])) for k in EC.FLAG_KEYS]
            if name in EC.NONEMPTY_NAMES:
                assert counts[1] > 0 and counts[2] > 0, (name, counts)
            if name in EC.RETRY_NAMES:
                assert counts[4] > 0, (name, counts)
            for k in EC.FLAG_KEYS:
                out[f"{name}.{k}"] = np.packbits(flags[k])
            out[name + ".counts"] = np.array(counts, dtype=np.int64)
            out[name + ".sha256"] = np.array(c.sha256)
            print(f"{name:18s} res {c.res:3d}  F {len(c.faces):5d}  Q {counts[0]}  contains {counts[1]}  hole {counts[2]}"
                  f"  occupancy {counts[3]}  holes left {counts[4]}")
    for name in EC.CLOUD_NAMES:
        pred, gt = EC.clouds(name)
        d = R.eval_pointcloud(pred.copy(), gt.copy())
        keys = sorted(d)
        out[f"pc.{name}.keys"] = np.array(keys)
        out[f"pc.{name}.values"] = np.array([float(d[k]) for k in keys], dtype=np.float64)
        out[f"pc.{name}.sha256"] = np.array(EC.clouds_sha256(name))
        print(f"pc.{name}: {len(pred)} against {len(gt)} points, chamfer_l2 {d['chamfer_l2']:.6g}")
    return out


def main():
    out = compute()
    if "--check" in sys.argv:
        old = np.load(PATH)
        assert sorted(old.files) == sorted(out), (sorted(set(old.files) ^ set(out)))
        bad = [k for k in out if not np.array_equal(old[k], out[k])]
        assert not bad, bad
        print(f"check: {os.path.relpath(PATH, ROOT)} reproduced, {len(out)} arrays equal")
        return
    np.savez_compressed(PATH, **out)
    print(f"wrote {os.path.relpath(PATH, ROOT)}: {os.path.getsize(PATH)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
