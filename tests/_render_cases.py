"""Meshes and cameras shared by test_render_cpu.py and test_render_gpu.py, and the host program over csrc/render_math.h
(tests/csrc/render_host.cpp).  Nothing here rasterises: the tests decide what is compared with what."""
import os
import subprocess

import numpy as np

from _host_cxx import host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc")


def _R():
    from list_amd import render
    return render


# ---- cameras ----------------------------------------------------------------------------------------------------------
def pixel_camera():
    """Orthographic, in pixel units: a mesh vertex (z, y, x) lands on pixel (x, y) with depth z, exactly (every product
    of the chain is a multiplication by 2 and by 0.5)."""
    R = _R()
    T = np.zeros((4, 3), dtype=np.float32)
    T[0, 0] = T[1, 1] = T[2, 2] = 0.5
    return R.Camera(T, R.ORTHO, 0, eye=(1, 0, 0, 0))


def list_pixel_camera(size):
    """LIST camera whose map plane is the size x size image itself: vertex (z, y, x) -> u = x / den, v = y / den with
    den = z + 1e-8f."""
    R = _R()
    T = np.zeros((4, 3), dtype=np.float32)
    T[0, 0] = T[1, 1] = T[2, 2] = 0.5
    return R.Camera.from_transmat(T, map_size=size)


def synthetic_list_camera(seed=7):
    from list_amd import synthetic
    return _R().Camera.from_transmat(synthetic.make_trans_mat(seed, 1)[0])


def tri(points):
    """points: [(x, y, z), ...] in pixel units, three per face -> (verts float32 [3n,3] as (z, y, x), faces int32 [n,3])."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    return np.ascontiguousarray(p[:, ::-1]), np.arange(len(p), dtype=np.int32).reshape(-1, 3)


def join(meshes):
    """[(verts, faces), ...] -> one mesh, faces in the given order."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def interleave(a, b):
    """Two meshes -> one whose faces alternate a0, b0, a1, b1, ... (the longer one's rest behind)."""
    v, f = join([a, b])
    na, nb = len(a[1]), len(b[1])
    order = []
    for i in range(max(na, nb)):
        if i < na:
            order.append(i)
        if i < nb:
            order.append(na + i)
    return v, f[np.array(order)]


# ---- meshes in pixel units --------------------------------------------------------------------------------------------------
def small_triangles(n=2000, size=64, seed=11, flat=False):
    """n triangles of 1 - 6 pixels: every clamped bounding box holds at most 7 x 7 centres."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-2.0, size + 2.0, (n, 1, 2))
    extent = rng.uniform(0.5, 3.0, (n, 1, 1))
    xy = centre + rng.uniform(-1.0, 1.0, (n, 3, 2)) * extent
    z = np.full((n, 3, 1), 1.0) if flat else rng.uniform(0.5, 4.0, (n, 3, 1))
    return tri(np.concatenate([xy, z], axis=2))


def large_triangles(n=40, size=64, seed=12, flat=False):
    """n triangles spanning up to the whole image; the first four lie mostly off-screen, one on each side.  Candidates
    whose clamped bounding box would be small or empty are drawn again."""
    R = _R()
    s = float(size)
    fixed = [[(-200, 10, 2), (20, 30, 3), (-150, 50, 1)], [(s + 180, 5, 1), (s - 15, 30, 2), (s + 90, 60, 3)],
             [(10, -300, 1), (30, 12, 2), (50, -120, 3)], [(5, s + 250, 3), (33, s - 14, 1), (60, s + 100, 2)]]
    rng = np.random.default_rng(seed)
    out = [np.asarray(t, dtype=np.float64) for t in fixed]
    cam = pixel_camera()
    while len(out) < n:
        t = np.concatenate([rng.uniform(-0.6 * s, 1.6 * s, (3, 2)), rng.uniform(0.5, 4.0, (3, 1))], axis=1)
        if R.face_outcomes_cpu(*tri(t), cam, size, size)[0] == R.STATS.index("large"):
            out.append(t)
    p = np.stack(out[:n])
    if flat:
        p[:, :, 2] = 1.0
    return tri(p)


def boundary_triangles(size=64):
    """Right triangles with vertices on pixel centres whose clamped bounding boxes hold CAP x CAP, (CAP+1) x CAP,
    CAP x (CAP+1) centres, and one whose box holds CAP x CAP only after clamping to the image -> (mesh, the expected
    STATS names per face)."""
    c = _R().CAP
    t = [[(3, 4, 1), (3 + c - 1, 4, 1), (3, 4 + c - 1, 1)],                 # c x c centres
         [(20, 4, 1), (20 + c, 4, 1), (20, 4 + c - 1, 1)],                  # (c + 1) x c
         [(40, 4, 1), (40 + c - 1, 4, 1), (40, 4 + c, 1)],                  # c x (c + 1)
         [(-9, 30, 1), (c - 1, 30, 1), (c - 1, 30 + c - 1, 1)],             # x from -9: clamped to 0 .. c - 1
         [(size - c, 50, 1), (size + 30, 50, 1), (size - c, 50 + c - 1, 1)]]  # clamped on the right
    return tri(t), ["small", "large", "large", "small", "small"]


def copies(n=5000, seed=13):
    """n copies of one triangle at depth 1, each with its three vertices in one of the six orders."""
    rng = np.random.default_rng(seed)
    v, _ = tri([(5.3, 7.1, 1), (50.2, 20.7, 1), (20.9, 55.4, 1)])
    perms = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]], dtype=np.int32)
    return v, np.ascontiguousarray(perms[rng.integers(0, 6, n)])


def coplanar(n=64, size=64, seed=14):
    """n overlapping triangles in the plane z = 1, small and large ones."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, size, (n, 1, 2)) + rng.uniform(-1, 1, (n, 3, 2)) * rng.uniform(2, 30, (n, 1, 1))
    return tri(np.concatenate([xy, np.ones((n, 3, 1))], axis=2))


def with_dropped_faces(mesh_valid):
    """The valid mesh with one face of each dropped kind spliced in between its faces (orthographic pixel camera) ->
    (verts, faces, {STATS name: count of the added faces})."""
    v, f = mesh_valid
    V = len(v)
    extra_v = np.array([[1, 10, 10], [np.nan, 12, 30], [1, 20, 10],          # V + 0 .. 2: a NaN vertex
                        [1, 10, 40], [np.inf, 30, 40], [1, 30, 50],           # V + 3 .. 5: a vertex at +inf (depth)
                        [1, 5, 5], [1, 5, -np.inf], [1, 9, 9],                # V + 6 .. 8: a vertex at -inf (x)
                        [1, 4, 3.0e6], [1, 8, 2], [1, 2, 9],                  # V + 9 .. 11: beyond the guard band
                        [1, 10, 10], [1, 20, 20], [1, 30, 30],                # V + 12 .. 14: collinear: zero area
                        [1, 10.51, 10.52], [1, 10.53, 10.51], [1, 10.52, 10.53]],    # V + 15 .. 17: snaps to one point
                       dtype=np.float32)
    extra_f = np.array([[V + 0, V + 1, V + 2], [V + 3, V + 4, V + 5], [V + 6, V + 7, V + 8], [V + 9, V + 10, V + 11],
                        [V + 12, V + 13, V + 14], [V + 15, V + 16, V + 17], [0, 1, V + 18], [0, -1, 2], [V, V, V]],     # the last three: index == V, a negative index, (a, a, a)
                       dtype=np.int32)
    verts = np.concatenate([v, extra_v]).astype(np.float32)
    step = max(1, len(f) // (len(extra_f) + 1))
    faces = []
    for i, e in enumerate(extra_f):
        faces += [f[i * step:(i + 1) * step], e[None]]
    faces.append(f[len(extra_f) * step:])
    faces = np.concatenate(faces).astype(np.int32)
    assert len(faces) == len(f) + len(extra_f)
    return verts, faces, {"non_finite": 3, "guard_band": 1, "zero_area": 3, "bad_index": 2}


def near_plane_faces(size=64):
    """LIST pixel camera of `size`: a valid face, a face behind the camera (den < 0), a face straddling z_near = 0.25 (one
    vertex at den 0.1), a face with a vertex exactly at z_near -> (mesh, z_near, expected behind_near)."""
    t = [[(10, 10, 1), (50, 12, 1), (30, 50, 1)],
         [(10, 10, -2), (50, 12, -2), (30, 50, -2)],
         [(10, 10, 2), (5, 1.2, 0.1), (30, 50, 2)],
         [(2.5, 2.5, 0.25), (12, 3, 1), (3, 12, 1)]]
    return tri(t), 0.25, 3


# ---- marching-cubes meshes --------------------------------------------------------------------------------------------------
def sphere_field(n, r, c=(0.0, 0.0, 0.0)):
    a = np.linspace(-0.5, 0.5, n, dtype=np.float64)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


THREE_SPHERES = ((0.25, (-0.15, -0.12, -0.10)), (0.10, (0.30, 0.30, 0.25)), (0.04, (0.30, -0.30, 0.30)))


def three_spheres(n=48):
    """float32 [n,n,n], positive inside three well-separated spheres of very different sizes."""
    return np.maximum.reduce([sphere_field(n, r, c) for r, c in THREE_SPHERES])


# ---- the header on the host ---------------------------------------------------------------------------------------------
def build_host(directory):
    """Compiles tests/csrc/render_host.cpp for the host as the library is built (no contraction) -> the program's path."""
    exe = os.path.join(str(directory), "render_host")
    subprocess.run([host_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(ROOT, "tests", "csrc", "render_host.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_host(exe, directory, verts, faces, camera, H, W, z_near=1e-6, mode="lambert", background=None, alpha=1.0):
    """The header's rasteriser and shader on one mesh -> (face_id, depth, stats dict, rgb)."""
    R = _R()
    src, out = os.path.join(str(directory), "render_host.in"), os.path.join(str(directory), "render_host.out")
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    head = np.array([len(v), len(f), H, W, camera.mode, camera.map_size, R.SHADES[mode], R._alpha256(alpha),
                     background is not None], dtype=np.int64)
    with open(src, "wb") as fh:
        fh.write(head.tobytes() + camera.T.astype(np.float32).tobytes() + camera.eye.astype(np.float32).tobytes() +
                 np.float32(z_near).tobytes() + v.tobytes() + f.tobytes())
        if background is not None:
            fh.write(np.ascontiguousarray(background, dtype=np.uint8).tobytes())
    subprocess.run([exe, src, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    n = H * W
    face_id = np.frombuffer(raw, np.int32, n, 0).reshape(H, W)
    depth = np.frombuffer(raw, np.float32, n, 4 * n).reshape(H, W)
    stats = np.frombuffer(raw, np.int32, len(R.STATS), 8 * n)
    rgb = np.frombuffer(raw, np.uint8, 3 * n, 8 * n + 4 * len(R.STATS)).reshape(H, W, 3)
    return face_id, depth, dict(zip(R.STATS, stats.tolist())), rgb
