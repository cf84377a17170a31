"""Meshes shared by test_components_cpu.py and test_components_gpu.py: name -> (faces int32 [F,3], V)."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
STRIP_LENGTHS = (255, 256, 257, 1023, 1025, 3001)           # block (256) and wave (64) edges, and a long one
STRIP_ORDERS = ("ascending", "descending", "permuted")


def strip(F, order):
    """A triangle strip of F faces over F + 2 vertices, face i = (p[i], p[i+1], p[i+2]): one component whose label has
    to travel the whole length."""
    V = F + 2
    p = np.arange(V)
    if order == "descending":
        p = p[::-1]
    elif order == "permuted":
        p = np.random.default_rng(1000 + F).permutation(V)
    i = np.arange(F)
    return np.stack([p[i], p[i + 1], p[i + 2]], axis=1).astype(np.int32), V


def many_small(n=700, seed=5):
    """n components of 1-7 triangles (fans), vertex ids permuted over the whole range, faces shuffled: many equal
    face counts."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 8, size=n)
    first = np.cumsum(sizes + 2) - (sizes + 2)               # each fan's first vertex: t triangles over t + 2 vertices
    base = np.repeat(first, sizes)
    k = np.arange(sizes.sum()) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    V = int((sizes + 2).sum())
    perm = rng.permutation(V)
    f = perm[np.stack([base, base + k + 1, base + k + 2], axis=1)]
    return f[rng.permutation(len(f))].astype(np.int32), V


def irregular():
    """Invalid indices, degenerate and duplicate faces, and unreferenced vertices (10-14, 30) in the middle."""
    V = 40
    f = [(0, 1, 2), (2, 3, 4), (0, 1, 2),                    # a duplicate
         (5, 5, 6), (7, 7, 7), (8, 9, 8),                    # degenerate: two nodes, one node, two nodes
         (-1, 0, 1), (3, V, 4), (15, 16, INT32_MAX), (-5, -6, -7), (V + 3, 2, 2),       # invalid
         (15, 16, 17), (17, 18, 19), (25, 20, 21), (22, 23, 24), (24, 25, 26),
         (39, 38, 37), (37, 36, 35), (31, 32, 33), (34, 33, 35), (29, 28, 27), (6, 27, 9)]
    return np.array(f, dtype=np.int32), V


SMALL = {
    "no_faces": (np.zeros((0, 3), dtype=np.int32), 5),
    "one_triangle": (np.array([[0, 1, 2]], dtype=np.int32), 3),
    "two_sharing_a_vertex": (np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32), 5),
    "two_disjoint": (np.array([[3, 4, 5], [0, 1, 2]], dtype=np.int32), 6),
}


def sphere_field(n, r, c):
    a = np.linspace(-0.5, 0.5, n, dtype=np.float64)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def three_spheres(n=40):
    """(s_big, s_small, s_blob): float32 [n,n,n] fields, positive inside, of three well-separated spheres."""
    return (sphere_field(n, 0.25, (-0.15, -0.12, -0.10)), sphere_field(n, 0.10, (0.30, 0.30, 0.25)),
            sphere_field(n, 0.04, (0.30, -0.30, 0.30)))


def cut_cells(field, level=0.0):
    """bool [n-1,n-1,n-1]: the cells whose corners are not all on one side."""
    inside = field > level
    n = inside.shape[0]
    cnt = np.zeros((n - 1,) * 3, dtype=np.int32)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cnt += inside[dx:n - 1 + dx, dy:n - 1 + dy, dz:n - 1 + dz]
    return (cnt > 0) & (cnt < 8)


def label_cases():
    """Every labelling case of the issue that needs no marching cubes."""
    cases = dict(SMALL)
    for F in STRIP_LENGTHS:
        for order in STRIP_ORDERS:
            cases[f"strip_{F}_{order}"] = strip(F, order)
    cases["many_small"] = many_small()
    cases["irregular"] = irregular()
    return cases
