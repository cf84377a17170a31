"""Exact, platform-independent synthetic inputs of the path's shapes: feature-map shapes, the
synthetic camera, Conv1d(k=1)-shaped MLP weights, query points.

Every value is a pure integer hash of (seed, flat index) mapped to a dyadic
rational, so the authoring container, the GPU box and any numpy version produce
the same bits.  No libm call is involved (no Box-Muller): the "normal-ish"
variate is a centred sum of four uniforms, exact in float64.

Lives in the package so that the measurement harness (bench.py's GPU leg, tools/) needs nothing from oracle/;
oracle/synth.py re-exports it for the golden generator and the parity tests, which feed the reference, the
oracle and the HIP path identical inputs.
"""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(z):
    # splitmix64 finaliser on uint64 arrays (wrap-around arithmetic is intended)
    z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def _bits(seed, n, stream=0, chunk=1 << 22):
    out = np.empty(n, dtype=np.uint64)
    base = np.uint64((int(seed) * 0xD1342543DE82EF95 + int(stream) * 0xA0761D6478BD642F)
                     & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            idx = np.arange(s, e, dtype=np.uint64)
            out[s:e] = _mix(_mix(idx ^ base) + base)
    return out


def uniform(seed, shape, lo=0.0, hi=1.0):
    """float32 U[lo,hi) on a 2^-24 lattice."""
    n = int(np.prod(shape))
    u = (_bits(seed, n) >> np.uint64(40)).astype(np.float64) * (1.0 / (1 << 24))
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def normalish(seed, shape, scale=1.0):
    """float32, mean 0, variance scale^2, bell shaped (sum of 4 uniforms)."""
    n = int(np.prod(shape))
    b = _bits(seed, n)
    m16 = np.uint64(0xFFFF)
    s = ((b & m16) + ((b >> np.uint64(16)) & m16) + ((b >> np.uint64(32)) & m16)
         + ((b >> np.uint64(48)) & m16)).astype(np.float64)
    # each term U{0..65535}/65536: mean ~0.5, var 1/12; sum of 4: var 1/3
    z = (s / 65536.0 - 2.0 + 4 * 0.5 / 65536.0) * np.sqrt(3.0)
    return (scale * z).astype(np.float32).reshape(shape)


# ---------------------------------------------------------------------------
# Workload builders (shapes of SURVEY.md section 8a / 8d)
# ---------------------------------------------------------------------------
IMG_CHANNELS = (64, 64, 128, 256, 512)     # ResEncoder maps  (modules.py:1067)
VOX_CHANNELS = (1, 16, 32, 64, 128, 128)   # VoxelEncoder2 maps (modules.py:425-442)


def img_map_shapes(batch, img_res):
    return [(batch, c, max(img_res >> s, 1), max(img_res >> s, 1))
            for c, s in zip(IMG_CHANNELS, range(5))]


def vox_map_shapes(batch, vox_res):
    res = [vox_res, vox_res, vox_res // 2, vox_res // 4, vox_res // 8, vox_res // 16]
    return [(batch, c, max(r, 1), max(r, 1), max(r, 1)) for c, r in zip(VOX_CHANNELS, res)]


def make_img_maps(seed, batch, img_res):
    return [normalish(seed + 11 * i, s) for i, s in enumerate(img_map_shapes(batch, img_res))]


def make_vox_maps(seed, batch, vox_res):
    shapes = vox_map_shapes(batch, vox_res)
    maps = [uniform(seed + 1000, shapes[0])]                      # sigmoid output
    maps += [normalish(seed + 1000 + 13 * i, s) for i, s in enumerate(shapes[1:], 1)]
    return maps


def make_query(seed, batch, n):
    """U(-0.5,0.5)^3, the range of Datasets.py:229."""
    return uniform(seed + 2000, (batch, n, 3), -0.5, 0.5)


def make_trans_mat(seed, batch, jitter=0.05):
    """Synthetic camera of SURVEY 8d: u,v ~ 68 +- 60, Z ~ 1."""
    base = np.array([[60, 0, 0], [0, 60, 0], [0, 0, 0], [68, 68, 1]], dtype=np.float32)
    return (base[None] + normalish(seed + 3000, (batch, 4, 3), jitter)).astype(np.float32)


def make_mlp_weights(seed, feature_size=3610, h_dim=256):
    """Conv1d(k=1)-shaped weights with PyTorch-default-like scale U(+-1/sqrt(fan_in)).

    Keys follow the reference state_dict (modules.py:196-200)."""
    dims = [("fc_0", feature_size, 2 * h_dim), ("fc_1", 2 * h_dim, h_dim),
            ("fc_2", h_dim, h_dim), ("fc_out", h_dim, 1)]
    w = {}
    for i, (name, fin, fout) in enumerate(dims):
        bound = 1.0 / np.sqrt(fin)
        w[name + ".weight"] = uniform(seed + 4000 + 2 * i, (fout, fin, 1), -bound, bound)
        w[name + ".bias"] = uniform(seed + 4001 + 2 * i, (fout,), -bound, bound)
    return w


# ---------------------------------------------------------------------------
# A tiny dataset in Pix3D's on-disk layout (datasets.Datasets.Pix3D)
# ---------------------------------------------------------------------------
PIX3D_SIZES = ((37, 53), (64, 48), (120, 31), (16, 16), (301, 2), (90, 140))     # (H, W) of the generated images, in turn
_CUBE = (np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32),
         np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]]))
_OCTAHEDRON = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32),
               np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]))


def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        f.writelines(f"v {x:.6f} {y:.6f} {z:.6f}\n" for x, y, z in verts.tolist())
        f.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in faces.tolist())


def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n"
                f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        f.writelines(f"{x:.6f} {y:.6f} {z:.6f}\n" for x, y, z in verts.tolist())
        f.writelines(f"3 {a} {b} {c}\n" for a, b, c in faces.tolist())


def make_pix3d_tree(root, n_images=6, categories=("chair", "table"), sigmas=(0.003, 0.01, 0.07), rows=(60, 75, 90),
                    grid_points=400, seed=0):
    """Writes a tiny dataset in Pix3D's layout under `root` (= config.data_dir) and returns its description.

    Two models, one per category (a cube 'chair' and an octahedron 'table', each with mesh_org.ply and isosurf_scaled.obj
    and a sampled_points.npz stand-in holding query_points_sigma_* [rows,4] and grid_points [grid_points,3]); `n_images`
    images uint8 [H,W,3] of the sizes PIX3D_SIZES in turn, alternating between the models; metadata records
    data/pix3d.json for them plus one record whose files are missing; splits/train.json and splits/test.json, each naming
    every record and one 'flipped' name that a reader must skip.  Returns {'data_dir', 'records' (the metadata list),
    'images' {id: uint8 array}, 'missing_id', 'model_folders' {category: folder}}."""
    import json
    import os
    data = os.path.join(root, "data")
    models = {}
    for ci, (cat, (verts, faces)) in enumerate(zip(categories, (_CUBE, _OCTAHEDRON))):
        folder = f"SYN_{cat}_{ci:02d}.model"
        models[cat] = folder
        iso = os.path.join(data, "isosurface", cat, folder)
        pts = os.path.join(data, "sampled_points", cat, folder)
        os.makedirs(iso, exist_ok=True)
        os.makedirs(pts, exist_ok=True)
        os.makedirs(os.path.join(data, "img", cat, folder), exist_ok=True)
        _write_ply(os.path.join(iso, "mesh_org.ply"), verts * np.float32(0.8 + 0.3 * ci), faces)
        _write_obj(os.path.join(iso, "isosurf_scaled.obj"), verts * np.float32(0.3), faces)
        tables = {f"query_points_sigma_{s}": normalish(seed + 8100 + 10 * ci + i, (rows[i], 4), 0.1) for i, s in enumerate(sigmas)}
        tables["grid_points"] = uniform(seed + 8200 + ci, (grid_points, 3), -0.3, 0.3)
        np.savez(os.path.join(pts, "sampled_points.npz"), **tables)
    records, images = [], {}
    for i in range(n_images):
        cat = categories[i % len(categories)]
        folder = models[cat]
        H, W = PIX3D_SIZES[i % len(PIX3D_SIZES)]
        images[i] = (uniform(seed + 8300 + i, (H, W, 3)) * 256).astype(np.uint8)
        np.save(os.path.join(data, "img", cat, folder, f"{i:04d}.npy"), images[i])
        records.append({"img": f"img/{cat}/{i:04d}.png", "category": cat,
                        "model": f"model/{cat}/{folder.split('.')[0]}/model.obj"})
    missing = len(records)                                   # its model has no files
    records.append({"img": f"img/{categories[0]}/{missing:04d}.png", "category": categories[0],
                    "model": f"model/{categories[0]}/SYN_absent/model.obj"})
    with open(os.path.join(data, "pix3d.json"), "w") as f:
        json.dump(records, f)
    os.makedirs(os.path.join(root, "splits"), exist_ok=True)
    names = [f"img/{r['category']}/{i:04d}.png" for i, r in enumerate(records)]
    for split in ("train", "test"):
        with open(os.path.join(root, "splits", split + ".json"), "w") as f:
            json.dump(names + [f"img/{categories[0]}/0000_flipped.png"], f)
    return {"data_dir": root, "records": records, "images": images, "missing_id": missing, "model_folders": models}
