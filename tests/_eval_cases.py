"""The inputs of tests/golden/eval_ref.npz (numpy only): meshes, triangle soups and query points on which the
reference's inside test (evaluation/libmesh, implicit_waterproofing.py) was recorded by `python -m oracle.gen_eval_golden`,
and two pairs of point clouds for its eval_pointcloud.  The fixture stores answers and a SHA-256 of the inputs, not the
inputs: the tests rebuild them here and assert the hash first.

Everything is built from integer arithmetic (splitmix64 of a counter), np.linspace grids and the counter-based
evaluate.box_samples_cpu -- no numpy random generator, whose streams are no contract.

Soups are pinned to the hash's grid.  Two bounding triangles fix the soup's bounding box to [0, res - 1]^3, so the
reference's scale is exactly 1 and its translate exactly 0.5: a vertex coordinate v lands on the scaled coordinate
v + 0.5, whose cell is its integer part.  Vertices are on integers and half-integers (exact in float32), so half of them
lie on cell borders.  A soup is written in doubled scaled coordinates h = 2 (v + 0.5), integers in [1, 2 res - 1]; the
cell of h is h // 2.  Every soup asserts on the host the property it exists for (`Case.check`): the widest narrow
triangle per axis (the kernel's kx, ky) and the number of wide triangles, computed with evaluate._cell_clamp.
"""
import functools
import hashlib

import numpy as np

from list_amd import evaluate as E
from list_amd import mesh as M

MAX_NARROW = 8                                        # eval_kernels.hip: kMaxNarrow
N_TRI = 400


def _ints(seed, shape):
    """Counter-based uint64 of the given shape: splitmix64(splitmix64(seed) ^ counter)."""
    n = int(np.prod(shape))
    return E.splitmix64(np.arange(n, dtype=np.uint64) ^ np.uint64(E.splitmix64(int(seed)))).reshape(shape)


def _mod(r, k):
    return (r % np.asarray(k).astype(np.uint64)).astype(np.int64)


class Case:
    def __init__(self, name, verts, faces, points, res, expect=None):
        self.name, self.res, self.expect = name, int(res), expect
        self.verts = np.ascontiguousarray(verts, dtype=np.float32)
        self.faces = np.ascontiguousarray(faces, dtype=np.int32)
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        assert np.array_equal(self.verts.astype(np.float64), np.asarray(verts, dtype=np.float64)), name
        if expect is not None:
            self.check()

    @property
    def sha256(self):
        h = hashlib.sha256()
        for a in (self.verts, self.faces, self.points, np.array([self.res], dtype=np.int64)):
            h.update(a.tobytes())
        return h.hexdigest()

    def cell_widths(self, rot=None):
        """Per triangle: its cell widths on x and y and whether the kernel calls it wide (hash_key_kernel's rule), under
        the rotation of a retry when rot is given."""
        res = self.res
        tri = self.verts.astype(np.float64)[self.faces]
        if rot is not None:
            tri = np.stack(E._rotate(np.asarray(rot), tri[..., 0], tri[..., 1], tri[..., 2]), axis=-1)
        lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
        scale = (res - 1) / (hi - lo)
        translate = 0.5 - scale * lo
        t = scale * tri + translate
        x0, x1 = E._cell_clamp(t[:, :, 0].min(axis=1), res), E._cell_clamp(t[:, :, 0].max(axis=1), res)
        y0, y1 = E._cell_clamp(t[:, :, 1].min(axis=1), res), E._cell_clamp(t[:, :, 1].max(axis=1), res)
        wx, wy = x1 - x0, y1 - y0
        return scale, translate, x0, y0, wx, wy, (wx > MAX_NARROW) | (wy > MAX_NARROW)

    def check(self):
        e = self.expect
        scale, translate, x0, y0, wx, wy, wide = self.cell_widths()
        if e.get("pinned", True):
            assert np.all(scale == 1.0) and np.all(translate == 0.5), (self.name, scale, translate)
        assert int(wide.sum()) == e["n_wide"], (self.name, int(wide.sum()))
        if e["kx"] is None:                                         # no narrow triangle, in the retries' frames either
            assert wide.all(), self.name
            for euler in E.EULER_RETRIES:
                assert self.cell_widths(E.rotation_matrix(euler))[-1].all(), (self.name, euler)
        else:
            assert int(wx[~wide].max()) == e["kx"] and int(wy[~wide].max()) == e["ky"], \
                (self.name, int(wx[~wide].max()), int(wy[~wide].max()))
        if e.get("low0"):
            assert np.count_nonzero(~wide & (x0 == 0)) > 50 and np.count_nonzero(~wide & (y0 == 0)) > 50, self.name
            cx = np.floor(self.points[:, 0] + 0.5)
            assert np.count_nonzero((cx >= 0) & (cx <= MAX_NARROW)) > len(self.points) // 2, self.name


# ---- meshes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sphere24():
    a = np.linspace(-0.5, 0.5, 24)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return M.marching_cubes_cpu((0.3 - np.sqrt(x * x + y * y + z * z)).astype(np.float32))


def sphere24_open():
    v, f = sphere24()
    return v, f[~np.all(v[f][:, :, 2] > 0.2, axis=1)]             # the top cap removed: holes, resolved by the retries


def box12():
    v = np.array([[x, y, z] for x in (-0.3, 0.3) for y in (-0.2, 0.25) for z in (-0.35, 0.3)], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return v, f


def _mesh_points(v, seed):
    """Uniform points, every 7th vertex, and a grid (the point sets of test_mesh_contains_bit_exact)."""
    grid = np.stack(np.meshgrid(*[np.linspace(-0.31, 0.31, 24)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([E.box_samples_cpu(50_000, -0.5, 0.5, seed), v[::7].astype(np.float64), grid])


def _mesh_case(name, mesh, res, seed):
    v, f = mesh
    return Case(name, v, f, _mesh_points(v, seed), res)


# ---- soups ------------------------------------------------------------------------------------------------------------
def _bounding_narrow(res):
    """Two small corner triangles (one cell wide at most) that fix the bounding box to [0, res - 1]^3."""
    m = float(res - 1)
    return np.array([[[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0.5]],
                     [[m, m, m], [m - 0.5, m, m], [m, m - 0.5, m - 0.5]]])


def _bounding_wide(res):
    """The same box from two triangles that span the whole grid on x and on y."""
    m = float(res - 1)
    return np.array([[[0, 0, 0], [m, 0, 0.5], [0, m, 0]],
                     [[m, m, m], [0, m, m - 0.5], [m, 0, m]]])


def _axis(r, w, low, res):
    """Doubled coordinates (min, max, mid) of triangles whose cells on this axis are [low, low + w]."""
    hmin = np.maximum(2 * low + _mod(r[:, 0], 2), 1)
    hmax = np.maximum(2 * (low + w) + _mod(r[:, 1], 2), hmin)
    hmid = hmin + _mod(r[:, 2], hmax - hmin + 1)
    assert np.all(hmax <= 2 * res - 1) and np.all(hmin // 2 == low) and np.all(hmax // 2 == low + w)
    return hmin, hmax, hmid


def _soup_triangles(res, seed, wx, wy, low0=False):
    """len(wx) triangles [n, 3, 3] (vertex coordinates) with the given cell widths, low corners drawn from the hash
    (or pinned to row / column 0), z anywhere."""
    n = len(wx)
    r = _ints(seed, (n, 12))
    t = np.arange(n)
    lowx, lowy = _mod(r[:, 0], res - wx), _mod(r[:, 1], res - wy)
    if low0:
        lowx = np.where(t % 4 <= 1, 0, lowx)
        lowy = np.where((t % 4 == 1) | (t % 4 == 2), 0, lowy)
    xmin, xmax, xmid = _axis(r[:, 2:5], wx, lowx, res)
    ymin, ymax, ymid = _axis(r[:, 5:8], wy, lowy, res)
    h = np.empty((n, 3, 3), dtype=np.int64)
    h[:, :, 0] = np.stack([xmin, xmax, xmid], axis=1)
    h[:, :, 1] = np.stack([ymid, ymin, ymax], axis=1)
    h[:, :, 2] = 1 + _mod(r[:, 8:11], 2 * res - 1)
    swap = _mod(r[:, 11], 2) == 1                                  # both windings
    h[swap] = h[swap][:, [0, 2, 1]]
    return (h - 1) / 2.0


def _widths(seed, n, kx, ky):
    """Every third triangle exactly kx wide, every third exactly ky high, the rest anything up to (kx, ky)."""
    r = _ints(seed, (n, 2))
    t = np.arange(n)
    return np.where(t % 3 == 0, kx, _mod(r[:, 0], kx + 1)), np.where(t % 3 == 1, ky, _mod(r[:, 1], ky + 1))


def _soup_points(res, seed, cells=None, n=30_000):
    """2 n + 3 points for a soup on [0, res - 1]^3: n half-integer lattice points of the scaled box [0, res]^3 (cell borders;
    a fifth of them on its six faces, px == 0 and px == res), n uniform points reaching a little outside the box, and three
    points with a NaN, +inf and -inf coordinate.  cells: restrict x and y to the cells [0, cells]."""
    top = 2 * res if cells is None else 2 * (cells + 1)
    r = _ints(seed, (n, 3))
    h = np.stack([_mod(r[:, 0], top + 1), _mod(r[:, 1], top + 1), _mod(r[:, 2], 2 * res + 1)], axis=1)
    j = np.arange(n // 5)
    h[j, j % 3] = np.where((j // 3) % 2 == 0, 0, 2 * res)         # the last 24 000 stay anywhere on the lattice
    lattice = h / 2.0 - 0.5
    uniform = E.box_samples_cpu(n, -0.75, res - 0.25, seed + 1)
    if cells is not None:
        uniform[:, :2] = E.box_samples_cpu(n, -0.5, cells + 0.5, seed + 2)[:, :2]
    c = (res - 1) / 2.0
    odd = np.array([[np.nan, c, c], [c, np.inf, c], [c, c, -np.inf]])
    return np.concatenate([lattice, uniform, odd])


def _soup_case(name, res, seed, kx, ky, n_wide9=0, all_wide=False, low0=False, grid=None, n=30_000):
    """grid: the resolution the geometry is laid out for, when it is not the hash's (hash_res 1 collapses every soup).
    n: half the number of points -- fewer where every point meets most triangles, which the host pays for pair by pair."""
    g = grid or res
    if all_wide:
        # wide on x and on y, by a cell more than the limit asks: a retry's rotation swaps one of the two for z and moves
        # the vertices on cell borders by a rounding, and the triangle must stay wide
        r = _ints(seed + 7, (N_TRI, 2))
        wx = MAX_NARROW + 2 + _mod(r[:, 0], g - 2 - MAX_NARROW)
        wy = MAX_NARROW + 2 + _mod(r[:, 1], g - 2 - MAX_NARROW)
        tris = np.concatenate([_bounding_wide(g), _soup_triangles(g, seed, wx, wy)])
        expect = {"kx": None, "ky": None, "n_wide": N_TRI + 2}
    else:
        wx, wy = _widths(seed + 7, N_TRI, kx, ky)
        tris = [_bounding_narrow(g), _soup_triangles(g, seed, wx, wy, low0)]
        if n_wide9:                                                # a few triangles one cell past the narrow limit
            w9 = np.full(n_wide9, MAX_NARROW + 1)
            rest = _mod(_ints(seed + 8, (n_wide9,)), ky + 1)
            half = n_wide9 // 2
            tris.append(_soup_triangles(g, seed + 9, w9[:half], rest[:half]))
            tris.append(_soup_triangles(g, seed + 10, _mod(_ints(seed + 11, (n_wide9 - half,)), kx + 1), w9[half:]))
        tris = np.concatenate(tris)
        expect = {"kx": kx, "ky": ky, "n_wide": n_wide9, "low0": low0}
    if grid:
        expect = {"kx": 0, "ky": 0, "n_wide": 0, "pinned": False}   # one cell: every triangle is narrow, of width 0
    verts = tris.reshape(-1, 3)
    faces = np.arange(len(verts)).reshape(-1, 3)
    return Case(name, verts, faces, _soup_points(g, seed + 20, cells=MAX_NARROW if low0 else None, n=n), res, expect)


_BUILDERS = {
    "sphere24": lambda: _mesh_case("sphere24", sphere24(), 512, 11),
    "sphere24_open": lambda: _mesh_case("sphere24_open", sphere24_open(), 512, 12),
    "box12_512": lambda: _mesh_case("box12_512", box12(), 512, 13),
    "box12_37": lambda: _mesh_case("box12_37", box12(), 37, 13),
    "soup65_w8": lambda: _soup_case("soup65_w8", 65, 100, 8, 8),
    "soup65_w8_wide9": lambda: _soup_case("soup65_w8_wide9", 65, 200, 8, 8, n_wide9=6),
    "soup65_kx8_ky2": lambda: _soup_case("soup65_kx8_ky2", 65, 300, 8, 2),
    "soup65_kx1_ky7": lambda: _soup_case("soup65_kx1_ky7", 65, 400, 1, 7),
    "soup65_low0": lambda: _soup_case("soup65_low0", 65, 500, 8, 8, low0=True),
    "soup17_wide": lambda: _soup_case("soup17_wide", 17, 600, None, None, all_wide=True, n=15_000),
    "soup33_narrow": lambda: _soup_case("soup33_narrow", 33, 700, 6, 4),
    "soup2": lambda: _soup_case("soup2", 2, 800, 1, 1, n=10_000),
    "soup1": lambda: _soup_case("soup1", 1, 800, 1, 1, grid=2, n=5_000),       # soup2's triangles
}
CASE_NAMES = tuple(_BUILDERS)
SOUP_NAMES = tuple(n for n in CASE_NAMES if n.startswith("soup"))
# hash_res 1 scales every coordinate by (res - 1) / extent = 0: all triangles collapse to the point 0.5, every
# determinant is 0 and no point can be inside or a hole.  Every other soup must have both.
NONEMPTY_NAMES = tuple(n for n in SOUP_NAMES if n != "soup1")
# open soups at hash_res 65 on which some points stay holes after the third rotation
RETRY_NAMES = ("soup65_w8", "soup65_w8_wide9", "soup65_kx8_ky2")


@functools.lru_cache(maxsize=None)
def build(name):
    return _BUILDERS[name]()


# ---- point clouds -----------------------------------------------------------------------------------------------------
CLOUD_NAMES = ("surfaces", "boxes")


@functools.lru_cache(maxsize=None)
def clouds(name):
    """(pred float32 [P,3], gt float32 [G,3]) for eval_pointcloud."""
    if name == "surfaces":
        pred = E.sample_surface_cpu(*sphere24(), 3000, seed=1)[0]
        gt = E.sample_surface_cpu(*sphere24_open(), 2500, seed=2)[0]
    else:
        pred = E.box_samples_cpu(4000, -0.5, 0.5, 5).astype(np.float32)
        gt = E.box_samples_cpu(300, -0.5, 0.5, 6).astype(np.float32)
        pred[::10] = gt[np.arange(400) % 300]                     # exact copies: distance 0, under every threshold
    return np.ascontiguousarray(pred), np.ascontiguousarray(gt)


def clouds_sha256(name):
    h = hashlib.sha256()
    for a in clouds(name):
        h.update(a.tobytes())
    return h.hexdigest()


# ---- the fixture ------------------------------------------------------------------------------------------------------
FLAG_KEYS = ("contains", "hole", "occ", "rest")       # check_mesh_contains' pair, implicit_waterproofing's pair


def unpack(golden, name):
    """The four recorded flag arrays of a case (bool [Q]) and their counts, from the loaded npz."""
    counts = golden[name + ".counts"]
    q = int(counts[0])
    flags = {k: np.unpackbits(golden[f"{name}.{k}"])[:q].astype(bool) for k in FLAG_KEYS}
    for i, k in enumerate(FLAG_KEYS):
        assert int(np.count_nonzero(flags[k])) == int(counts[1 + i]), (name, k)
    return flags, dict(zip(FLAG_KEYS, (int(c) for c in counts[1:])))
