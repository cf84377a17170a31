"""The per-launch, per-element check of the HIP coarse stage (list_amd.coarse), shared by test_coarse_cpu.py (which
applies it to the numpy restatement and to deliberately wrong layers) and test_coarse_gpu.py (which applies it to every
launch of the device).  Plain numpy float64; no GPU here.

A launch is judged on its own: the reference is the float64 evaluation of that one launch on its OWN input as the
device held it, and every output element has its own bound, derived from absolute values as tests/_voxenc_check.py
derives its own.  With u = 2^-24 (fp32's unit roundoff):

  dot product   of length K accumulated in fp32 in ANY order, one rounding per product-and-add (an fmaf chain, which is
                also what v_mfma_f32_32x32x2_f32 computes) and one more for a bias: (K + 2) c u sum|a b|, the classical
                gamma_{K+1} <= (K + 2) u.  c = 1 on the vector ALU; c = 2 on the matrix cores, the allowance
                _voxenc_check.py states for their internal order -- fixed beforehand, not fitted.
  input error   a launch that chains two products (the tree's leaky(leaves @ W_branch), then Wc; the point MLP's three
                layers) carries the first one's bound e through the second as e @ |W|, and |x| + e replaces |x| in the
                second's own accumulation term.
  epilogue      one u |value| per fp32 operation: 0.2 x of the leaky ReLU, the BN scale, the BN shift, a bias add
                outside the accumulator.  ReLU, leaky ReLU and max are 1-Lipschitz.
No measured tolerance anywhere."""
import numpy as np

import _voxenc_check as vc
from list_amd import coarse

U24 = 2.0 ** -24
SMALL = {"features": [32, 16, 48, 3], "degrees": [3, 1, 5]}


SLOPE = float(np.float32(0.2))        # the slope as fp32 holds it (the device's constant, and torch's in fp32)


def leaky(x):
    return np.where(x > 0, x, SLOPE * x)


def _dot(x, ex, W, b, c):
    """x [..,K] with error bound ex, W [O,K], b [O] or None -> (z, e): z = x W^T + b in float64, e its fp32 bound."""
    W = np.asarray(W, np.float64)
    z, A = x @ W.T, (np.abs(x) + ex) @ np.abs(W).T
    if b is not None:
        z, A = z + b, A + np.abs(b)
    return z, (W.shape[1] + 2) * c * U24 * np.where(np.isfinite(A), A, 0.0) + ex @ np.abs(W).T


def tree_reference(params, l, levels):
    """(y, bound) of tree launch l.  levels: the device's levels 0 .. l, [B,nodes,features] each; params: params_of."""
    lay, f64 = params["layers"][l], np.float64
    leaves = np.asarray(levels[l], f64)
    B, node, fin = leaves.shape
    deg = lay["degree"]
    branch = np.asarray(lay["branch"], f64)
    g = np.einsum("bni,nij->bnj", leaves, branch).reshape(B, node * deg, fin)
    Ag = np.einsum("bni,nij->bnj", np.abs(leaves), np.abs(branch)).reshape(B, node * deg, fin)
    r = leaky(g)
    e_r = (fin + 2) * U24 * Ag + U24 * np.abs(r)
    wc = coarse.compose(lay["loop0"], lay["loop1"]).astype(f64)          # what the device holds, bit for bit
    z, A, K = r @ wc.T, (np.abs(r) + e_r) @ np.abs(wc).T, fin
    for lvl, w in zip(levels[:l + 1], lay["root"]):
        lvl, w = np.asarray(lvl, f64), np.asarray(w, f64)
        reps = (node // lvl.shape[1]) * deg
        z = z + np.repeat(lvl @ w.T, reps, axis=1)
        A = A + np.repeat(np.abs(lvl) @ np.abs(w).T, reps, axis=1)
        K += w.shape[1]
    e = (K + 2) * U24 * A + e_r @ np.abs(wc).T
    if lay["activation"]:
        pre = z + np.tile(np.asarray(lay["bias"], f64), (node, 1))
        y = leaky(pre)
        e = e + U24 * (np.abs(pre) + e) + U24 * np.abs(y)
        return y, e
    return z, e


def _folded(lay):
    s, t = coarse.bn_affine(lay["bn"])
    return (np.asarray(lay["w"], np.float64), np.asarray(lay["b"], np.float64), s.astype(np.float64),
            t.astype(np.float64))


def mlp_reference(params, pc):
    """(y, bound) of the point_mlp launch: the per-tile, per-channel maxima [B,tiles,512] of the device's own pc."""
    x = np.asarray(pc, np.float64)
    ex = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, lay in enumerate(params["mlp"]):
            w, b, s, t = _folded(lay)
            z, e = _dot(x, ex, w, b, 1 if k == 0 else 2)
            x = np.where(z * s + t < 0, 0.0, z * s + t)
            ex = np.abs(s) * e + 3 * U24 * (np.abs(s) * (np.where(np.isfinite(z), np.abs(z), 0.0) + e) + np.abs(t))
        P, T = x.shape[1], coarse.TILE
        tiles = (P + T - 1) // T
        y = np.stack([x[:, i * T:min(P, (i + 1) * T)].max(axis=1) for i in range(tiles)], axis=1)
        bound = np.stack([ex[:, i * T:min(P, (i + 1) * T)].max(axis=1) for i in range(tiles)], axis=1)
    return y, bound


def camera_reference(params, coarse_code, feat_g2):
    """(y, bound) of the camera launch on the device's own code: trans_mat [B,4,3]."""
    x = np.concatenate([np.asarray(coarse_code, np.float64), np.asarray(feat_g2, np.float64).reshape(len(feat_g2), -1)], 1)
    ex = np.zeros_like(x)
    for lay in params["cam"][:2]:
        w, b, s, t = _folded(lay)
        z, e = _dot(x, ex, w, b, 1)
        r = leaky(z)
        e_r = e + U24 * np.abs(r)
        x = r * s + t
        ex = np.abs(s) * e_r + 2 * U24 * (np.abs(s) * (np.abs(r) + e_r) + np.abs(t))
    lay = params["cam"][2]
    z, e = _dot(x, ex, np.asarray(lay["w"], np.float64), np.asarray(lay["b"], np.float64), 1)
    return z.reshape(-1, 4, 3), e.reshape(-1, 4, 3)


def worst(got, y, bound):
    """The largest error / bound; inf where a NaN or an infinity does not meet its like."""
    q = vc.ratios(np.asarray(got), y, bound, bound, False)
    return float(q.max()) if q.size else 0.0


def nanmax_tiles(tile_max):
    """The point_max launch exactly: max over the tiles, a NaN winning."""
    return np.asarray(tile_max).max(axis=1)                                # (numpy's max propagates a NaN)


def cloud_with_edge_cases(seed, B, P, R):
    """A cloud for the occupancy launches: random points, points exactly on a rounding tie ((i + 0.5) / (R - 1) - 0.5
    where that is representable), points outside the box on every side, and duplicates."""
    rng = np.random.default_rng(seed)
    pc = (rng.random((B, P, 3)) - 0.5).astype(np.float32)
    n = min(P // 4, 8)
    ties = ((np.arange(n) * 3 % (R - 1) + 0.5) / (R - 1) - 0.5).astype(np.float32)
    pc[:, :n, 0] = ties
    pc[:, n:2 * n, 2] = ties
    pc[:, 2 * n:2 * n + 3] = np.float32([[-0.7, 0.1, 0.2], [0.1, 0.9, -3.0], [0.5, -0.5, 0.5000001]])
    pc[:, 2 * n + 3:2 * n + 6] = pc[:, 2 * n + 6:2 * n + 7]                # duplicates of one point
    return pc
