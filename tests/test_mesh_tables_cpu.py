"""CPU: the marching-cubes case tables (csrc/mc_tables.h, tools/gen_mc_tables.py) and the numpy restatement of the
device kernels (mesh.marching_cubes_cpu), checked exhaustively or on analytic fields."""
import importlib.util
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc", "mc_tables.h")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "tools", "gen_mc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mesh():
    from list_amd import mesh
    return mesh


# ---- an independent statement of the cube geometry and of the face rule -----------------------------------------------
def _corners(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def _edge(c1, c2):
    """Edge number (4 * axis + (o1 | o2 << 1)) of the cube edge joining corners c1, c2."""
    a = (c1 ^ c2).bit_length() - 1
    p = _corners(c1)
    o = [p[b] for b in range(3) if b != a]
    return 4 * a + (int(o[0]) | int(o[1]) << 1)


def _cube_faces():
    """Each face as its 4 corners in cyclic order."""
    out = []
    for a in range(3):
        for s in (0, 1):
            cs = [c for c in range(8) if _corners(c)[a] == s]
            b, d = [x for x in range(3) if x != a]
            key = {(0, 0): 0, (1, 0): 1, (1, 1): 2, (0, 1): 3}
            out.append(sorted(cs, key=lambda c: key[(int(_corners(c)[b]), int(_corners(c)[d]))]))
    return out


FACES = _cube_faces()


def _rule(ring, case):
    """Set of unordered segments {e1, e2} the face rule draws on a face: inside corners never joined diagonally."""
    inside = [(case >> c) & 1 for c in ring]
    e = [_edge(ring[i], ring[(i + 1) % 4]) for i in range(4)]
    cut = [i for i in range(4) if inside[i] != inside[(i + 1) % 4]]
    if not cut:
        return set()
    if len(cut) == 4:          # diagonal pair: cut off each inside corner (edges i-1 and i meet at corner i)
        return {frozenset((e[(i - 1) % 4], e[i])) for i in range(4) if inside[i]}
    return {frozenset((e[cut[0]], e[cut[1]]))}


def _ambiguous(case):
    for ring in FACES:
        f = [(case >> c) & 1 for c in ring]
        if f[0] == f[2] and f[1] == f[3] and f[0] != f[1]:
            return True
    return False


def _triangles(case):
    _, count, edges = _mesh().tables()
    return [tuple(int(x) for x in edges[case, 3 * t:3 * t + 3]) for t in range(count[case])]


def _face_of(e1, e2):
    """The cube face containing both edges, if any."""
    for fi, ring in enumerate(FACES):
        fe = {_edge(ring[i], ring[(i + 1) % 4]) for i in range(4)}
        if e1 in fe and e2 in fe:
            return fi
    return None


# ---- tables -----------------------------------------------------------------------------------------------------------
def test_generator_reproduces_committed_header():
    with open(HEADER) as f:
        assert _generator().render() == f.read(), "rerun tools/gen_mc_tables.py and commit csrc/mc_tables.h"


def test_edge_mask_and_counts_are_consistent():
    mask, count, edges = _mesh().tables()
    for case in range(256):
        used = {e for tri in _triangles(case) for e in tri}
        want = {_edge(c1, c2) for c1, c2 in itertools.combinations(range(8), 2)
                if bin(c1 ^ c2).count("1") == 1 and ((case >> c1) & 1) != ((case >> c2) & 1)}
        assert used == want, case
        assert mask[case] == sum(1 << e for e in want), case
        assert count[case] <= 5 and all(x == -1 for x in edges[case, 3 * count[case]:])
    assert count[0] == 0 and count[255] == 0


def test_case_boundary_on_every_face_is_the_face_rule():
    """Watertightness, exhaustively: in each case the triangles' boundary (edges used once) lies on the cube's faces and
    equals, face by face, the segments the face rule draws from that face's 4 corners alone -- so the two cells sharing
    a face agree.  Interior edges are used twice, in opposite directions."""
    for case in range(256):
        directed = {}
        for a, b, c in _triangles(case):
            for u, v in ((a, b), (b, c), (c, a)):
                directed[(u, v)] = directed.get((u, v), 0) + 1
        assert max(directed.values(), default=1) == 1, case            # consistent orientation inside the cell
        boundary = [(u, v) for (u, v) in directed if (v, u) not in directed]
        per_face = {fi: set() for fi in range(6)}
        for u, v in boundary:
            fi = _face_of(u, v)
            assert fi is not None, (case, u, v)
            per_face[fi].add(frozenset((u, v)))
        for fi, ring in enumerate(FACES):
            assert per_face[fi] == _rule(ring, case), (case, fi)


def test_winding_points_toward_decreasing_values():
    """Single-corner cases: the triangle's right-hand normal points away from the one inside corner (and toward it when
    that corner is the one outside), at the edge midpoints."""
    for c in range(8):
        for case, sign in ((1 << c, 1.0), (255 ^ (1 << c), -1.0)):
            (a, b, d), = _triangles(case)
            pos = [np.mean([_corners(x) for x in _edge_corners(e)], axis=0) for e in (a, b, d)]
            n = np.cross(pos[1] - pos[0], pos[2] - pos[0])
            away = np.mean(pos, axis=0) - _corners(c)
            assert sign * float(n @ away) > 0, (case, n, away)


def _edge_corners(e):
    return [(c, d) for c, d in itertools.combinations(range(8), 2) if bin(c ^ d).count("1") == 1 and _edge(c, d) == e][0]


def _canon(tri):
    k = tri.index(min(tri))
    return tri[k:] + tri[:k]


def test_complementary_cases_reverse_the_winding():
    """c and 255 - c cut the same edges; where no face is ambiguous the face rule draws the same segments for both, and
    the triangles are the same with opposite winding.  The exception, by design: a case with an ambiguous face (two
    diagonal inside corners) separates its inside corners there, and its complement separates the other diagonal
    pair -- different segments, so a different (still watertight) surface."""
    mask, _, _ = _mesh().tables()
    n_sym = n_amb = 0
    for case in range(256):
        comp = 255 - case
        assert mask[case] == mask[comp]
        a = sorted(_canon(t) for t in _triangles(case))
        b = sorted(_canon((t[0], t[2], t[1])) for t in _triangles(comp))
        if _ambiguous(case):
            n_amb += 1
            assert a != b, case
        else:
            n_sym += 1
            assert a == b, case
    assert n_amb > 0 and n_sym > 0


# ---- numpy marching cubes -------------------------------------------------------------------------------------------
def _grid(shape, lo=-0.5, hi=0.5):
    axes = [np.linspace(lo, hi, n, dtype=np.float64) for n in shape]
    return np.meshgrid(*axes, indexing="ij")


def sphere(n, r=0.3, shape=None):
    x, y, z = _grid(shape or (n, n, n))
    return (r - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def topology(v, f):
    """(Euler characteristic, max uses of an undirected edge, min uses, max uses of a directed edge, signed volume)."""
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    _, ucnt = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    vol = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)
    return len(v) - len(ucnt) + len(f), int(ucnt.max()), int(ucnt.min()), int(dcnt.max()), vol


def test_cpu_sphere_is_closed_and_oriented():
    v, f = _mesh().marching_cubes_cpu(sphere(40))
    chi, umax, umin, dmax, vol = topology(v, f)
    assert (chi, umax, umin, dmax) == (2, 2, 2, 1)
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * 0.3 ** 3) - 1) < 0.03
    assert v.dtype == np.float32 and f.dtype == np.int32 and np.isfinite(v).all()


def test_cpu_empty_and_nonfinite_fields():
    mesh = _mesh()
    for fill in (1.0, -1.0):
        v, f = mesh.marching_cubes_cpu(np.full((5, 6, 7), fill, np.float32))
        assert v.shape == (0, 3) and f.shape == (0, 3)
    vol = sphere(20)
    vol[3, 4, 5], vol[10, 10, 4], vol[9, 9, 9], vol[10, 9, 10] = np.nan, np.inf, -np.inf, np.nan
    v, f = mesh.marching_cubes_cpu(vol)
    assert len(f) > 0 and np.isfinite(v).all() and f.min() >= 0 and f.max() < len(v)


def test_cpu_shape_limits():
    from list_amd import hip
    mesh = _mesh()
    with pytest.raises(hip.ListError):
        mesh.marching_cubes_cpu(np.zeros((1, 4, 4), np.float32))
    with pytest.raises(hip.ListError):
        mesh.marching_cubes_cpu(np.zeros((4, 4), np.float32))


def test_generate_mesh_falls_back_without_mcubes(monkeypatch, tmp_path):
    from list_amd import mesh, utils
    monkeypatch.setitem(sys.modules, "mcubes", None)           # import mcubes -> ImportError
    monkeypatch.setitem(sys.modules, "trimesh", None)
    vol = sphere(24)
    v, f = utils.generate_mesh(vol, -0.5, 0.5)
    v2, f2 = mesh.marching_cubes_cpu(vol)
    assert np.array_equal(v, v2) and np.array_equal(f, f2)
    m = utils.generate_mesh(vol, -0.5, 0.5, as_trimesh_obj=True)
    assert isinstance(m, mesh.Mesh)
    out = m.export(str(tmp_path / "s.obj"))
    lines = open(out).read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(v) and sum(l.startswith("f ") for l in lines) == len(f)


def test_mesh_export_ply_round_trip(tmp_path):
    mesh = _mesh()
    v, f = mesh.marching_cubes_cpu(sphere(16))
    path = mesh.Mesh(v, f).export(str(tmp_path / "s.ply"))
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    assert f"element vertex {len(v)}".encode() in head and f"element face {len(f)}".encode() in head
    vv = np.frombuffer(body[:12 * len(v)], dtype="<f4").reshape(-1, 3)
    ff = np.frombuffer(body[12 * len(v):], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert np.array_equal(vv, v) and (ff["n"] == 3).all() and np.array_equal(ff["i"], f)
    with pytest.raises(ValueError):
        mesh.Mesh(v, f).export(str(tmp_path / "s.stl"))


def test_capi_refuses_bad_shapes_without_gpu():
    """Shape validation of include/list_mesh.h happens before any HIP call, with list_mesh_last_error set."""
    import __graft_entry__ as ge
    ge.build()
    mesh = _mesh()
    lib = mesh.load()
    assert lib.list_mc_workspace_bytes(1, 8, 8) == 0
    assert b"axis" in lib.list_mesh_last_error()
    assert lib.list_mc_workspace_bytes(1024, 1024, 1024) == 0
    assert b"INT32_MAX" in lib.list_mesh_last_error()
    assert lib.list_mc_count(None, 8, 8, 1, 0.0, None, 0, None, None) == -2
    assert lib.list_mc_count(None, 8, 8, 8, 0.0, None, 0, None, None) == -1
    assert b"NULL" in lib.list_mesh_last_error()
