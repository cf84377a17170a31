"""CPU: the numpy restatement of the rasteriser (render.rasterize_cpu / shade_cpu) against facts worked out by hand, a
brute-force float64 point-in-triangle count, the analytic sphere and the oracle's projection; csrc/render_math.h compiled
for the host against the restatement, bit for bit; the C ABI of include/list_render.h; the parser's flags; Mesh.render
and the executor's pictures."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H        # noqa: E402
import _render_cases as RC       # noqa: E402


def _R():
    from list_amd import render
    return render


def covered(points, size, camera=None):
    """The set of (x, y) pixels the single triangle `points` [(x, y, z)] * 3 wins on a size x size image."""
    R = _R()
    v, f = RC.tri(points)
    face_id, depth, stats = R.rasterize_cpu(v, f, camera or RC.pixel_camera(), size, size)
    assert stats["small"] + stats["large"] == 1
    ys, xs = np.nonzero(face_id == 0)
    assert np.isinf(depth[face_id < 0]).all() and np.isfinite(depth[face_id == 0]).all()
    return set(zip(xs.tolist(), ys.tolist()))


# ---- the top-left rule, by hand ---------------------------------------------------------------------------------------------
# Pixel centres have integer coordinates and y grows downwards.  A centre on an edge belongs to the triangle iff the edge
# is a top edge (horizontal, the interior below it) or a left edge (the interior to its right).
HAND = {
    # legs on x = 0 (left edge: kept) and y = 0 (top edge: kept), hypotenuse x + y = 4 (interior to its left: dropped)
    "upper_left_half": ([(0, 0, 1), (4, 0, 1), (0, 4, 1)], {(x, y) for x in range(4) for y in range(4) if x + y <= 3}),
    # the other half of the square: x = 4 (right: dropped), y = 4 (bottom: dropped), x + y = 4 (interior to its right: kept)
    "lower_right_half": ([(4, 0, 1), (4, 4, 1), (0, 4, 1)], {(x, y) for x in range(4) for y in range(4) if x + y >= 4}),
    # the edge y = x / 2 runs through the centres (2, 1), (4, 2): for the triangle below it the interior is to its LEFT
    # (dropped); x = 0 is a left edge (kept), y = 3 a bottom edge (dropped)
    "below_the_slanted_edge": ([(0, 0, 1), (6, 3, 1), (0, 3, 1)], {(0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (3, 2)}),
    # ... and for the triangle above it the interior is to its RIGHT (kept); y = 0 is a top edge (kept), x = 6 a right
    # edge (dropped)
    "above_the_slanted_edge": ([(0, 0, 1), (6, 0, 1), (6, 3, 1)],
                               {(x, 0) for x in range(6)} | {(x, 1) for x in range(2, 6)} | {(4, 2), (5, 2)}),
}


@pytest.mark.parametrize("name", list(HAND))
@pytest.mark.parametrize("winding", ["as_given", "reversed"])
def test_top_left_rule_by_hand(name, winding):
    points, expected = HAND[name]
    if winding == "reversed":
        points = [points[0], points[2], points[1]]
    assert covered(points, 8) == expected


def test_hand_cases_tile_their_rectangles():
    """The two halves of each pair cover their rectangle exactly once -- the hand-made sets themselves agree with that."""
    a, b = HAND["upper_left_half"][1], HAND["lower_right_half"][1]
    assert not a & b and a | b == {(x, y) for x in range(4) for y in range(4)}
    a, b = HAND["below_the_slanted_edge"][1], HAND["above_the_slanted_edge"][1]
    assert not a & b and a | b == {(x, y) for x in range(6) for y in range(3)}


# ---- shared edges and a shared vertex: one winner per pixel, no holes -----------------------------------------------------
def brute_force_counts(points, size):
    """Per pixel, in float64 and without any fill rule: how many of the triangles hold the centre strictly inside
    (`inside`), and whether the centre lies on (within 1e-9 of) an edge line of any of them while not outside it
    (`on_edge`) -> (inside int [size,size], on_edge bool [size,size])."""
    ys, xs = np.mgrid[0:size, 0:size].astype(np.float64)
    inside, on_edge = np.zeros((size, size), dtype=np.int64), np.zeros((size, size), dtype=bool)
    for t in np.asarray(points, dtype=np.float64).reshape(-1, 3, 3):
        (x0, y0), (x1, y1), (x2, y2) = t[:, :2]
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        e = [((xb - xa) * (ys - ya) - (yb - ya) * (xs - xa)) * np.sign(area)
             for (xa, ya), (xb, yb) in (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1)))]
        e = np.stack(e)
        inside += (e > 1e-9).all(axis=0)
        on_edge |= (e >= -1e-9).all(axis=0) & (np.abs(e) <= 1e-9).any(axis=0)
    return inside, on_edge


# vertices on the 1/16 grid, so snapping moves nothing and the float64 check sees the triangles the rasteriser draws; both
# diagonals of the quad (slope 1 and -1 between integer points) and four spokes of the fan run through pixel centres
QUAD = [(2.0, 3.0), (41.0, 5.0), (44.0, 45.0), (5.0, 41.0)]
FAN_CENTRE = (20.0, 20.0)
FAN_RIM = [(38.5, 20.0), (33.0625, 33.0), (20.0, 39.25), (6.5, 30.75), (2.0, 20.0), (9.25, 5.5), (20.0, 1.125), (31.0, 7.0)]


def quad_faces(diagonal):
    a, b, c, d = [(x, y, 1.0) for x, y in QUAD]
    return [a, b, c, a, c, d] if diagonal == 0 else [a, b, d, b, c, d]


def fan_faces():
    c = FAN_CENTRE + (1.0,)
    rim = [p + (1.0,) for p in FAN_RIM]
    return [q for i in range(len(rim)) for q in (c, rim[i], rim[(i + 1) % len(rim)])]


@pytest.mark.parametrize("name,points", [("quad_diagonal_ac", quad_faces(0)), ("quad_diagonal_bd", quad_faces(1)),
                                         ("fan", fan_faces())])
def test_shared_edges_have_exactly_one_winner(name, points):
    R = _R()
    size, cam = 56, RC.pixel_camera()
    v, f = RC.tri(points)
    claims = np.zeros((size, size), dtype=np.int64)
    for k in range(len(f)):                                    # each face alone: which centres would it claim?
        claims += R.rasterize_cpu(v, f[k:k + 1], cam, size, size)[0] >= 0
    face_id = R.rasterize_cpu(v, f, cam, size, size)[0]
    inside, on_edge = brute_force_counts(points, size)
    assert claims.max() == 1, "a centre claimed by two faces"
    assert np.array_equal(face_id >= 0, claims == 1)
    interior = ~on_edge
    assert np.array_equal(claims[interior], inside[interior])       # away from the edges: the float64 count, 0 or 1
    # no holes: a centre strictly inside the union -- on an edge SHARED by two faces too -- has one winner.  The union is
    # star-shaped about `hub`; its own float64 test: inside a triangle of the hub's fan, or on a spoke but not on the outline
    outline = QUAD if name.startswith("quad") else FAN_RIM
    hub = tuple(np.mean(np.asarray(outline), axis=0)) if name.startswith("quad") else FAN_CENTRE
    shared = on_edge & ~outline_mask(outline, size)
    assert shared.sum() >= 10 and (claims[shared] == 1).all(), "centres on a shared edge: exactly one winner each"
    whole = [q + (1.0,) for i in range(len(outline)) for q in (hub, outline[i], outline[(i + 1) % len(outline)])]
    w_inside, w_edge = brute_force_counts(whole, size)
    strictly_inside_union = (w_inside == 1) | (w_edge & ~outline_mask(outline, size))
    assert (claims[strictly_inside_union] == 1).all(), "a hole inside the union"
    if name == "fan":
        assert face_id[int(FAN_CENTRE[1]), int(FAN_CENTRE[0])] >= 0    # the shared vertex on a centre: one winner


def outline_mask(outline, size):
    """Centres within 1e-9 of the outline polygon's own edges."""
    ys, xs = np.mgrid[0:size, 0:size].astype(np.float64)
    on = np.zeros((size, size), dtype=bool)
    n = len(outline)
    for i in range(n):
        (xa, ya), (xb, yb) = outline[i], outline[(i + 1) % n]
        e = (xb - xa) * (ys - ya) - (yb - ya) * (xs - xa)
        t = ((xs - xa) * (xb - xa) + (ys - ya) * (yb - ya)) / ((xb - xa) ** 2 + (yb - ya) ** 2)
        on |= (np.abs(e) <= 1e-9) & (t >= -1e-12) & (t <= 1 + 1e-12)
    return on


# ---- depth, ties, drop rules ------------------------------------------------------------------------------------------------
def test_nearer_triangle_wins_and_equal_depth_goes_to_the_lower_index():
    R = _R()
    cam = RC.pixel_camera()
    far, near = [(2, 2, 3.0), (30, 3, 3.0), (5, 28, 3.0)], [(4, 4, 2.0), (28, 6, 2.0), (8, 25, 2.0)]
    for order, winner in (([far, near], 1), ([near, far], 0)):
        v, f = RC.tri(order)
        face_id, depth, _ = R.rasterize_cpu(v, f, cam, 32, 32)
        alone = R.rasterize_cpu(*RC.tri([near]), cam, 32, 32)[0] >= 0
        assert alone.sum() > 100 and (face_id[alone] == winner).all() and (depth[alone] == 2.0).all()
        assert (depth[(face_id >= 0) & ~alone] == 3.0).all()
    v, f = RC.tri([near, near, near])
    face_id = R.rasterize_cpu(v, f[[2, 0, 1]], cam, 32, 32)[0]      # face k of the list is a copy whatever its vertices
    assert set(np.unique(face_id)) == {-1, 0}
    # LIST camera: the larger 1 / den is the nearer one, and depth comes back as den
    lcam = RC.list_pixel_camera(32)
    v, f = RC.tri([[(8, 8, 2.0), (56, 8, 2.0), (8, 56, 2.0)], [(4, 4, 1.0), (28, 4, 1.0), (4, 28, 1.0)]])
    face_id, depth, _ = R.rasterize_cpu(v, f, lcam, 32, 32)
    both = (R.rasterize_cpu(v, f[:1], lcam, 32, 32)[0] >= 0) & (R.rasterize_cpu(v, f[1:], lcam, 32, 32)[0] >= 0)
    assert both.sum() > 50 and (face_id[both] == 1).all() and (depth[both] == 1.0).all()
    assert (depth[face_id == 0] == 2.0).all()


def test_dropped_faces_leave_the_image_untouched_and_are_counted():
    R = _R()
    cam = RC.pixel_camera()
    valid = RC.small_triangles(60, 64, seed=5)
    ref_id, ref_depth, ref_stats = R.rasterize_cpu(*valid, cam, 64, 64)
    v, f, added = RC.with_dropped_faces(valid)
    face_id, depth, stats = R.rasterize_cpu(v, f, cam, 64, 64)
    kept = np.flatnonzero((f < len(valid[0])).all(axis=1) & (f >= 0).all(axis=1))       # the valid faces' new indices
    assert len(kept) == 60
    assert np.array_equal(face_id >= 0, ref_id >= 0) and depth.tobytes() == ref_depth.tobytes()
    assert np.array_equal(face_id[face_id >= 0], kept[ref_id[ref_id >= 0]])
    for name in R.STATS:
        assert stats[name] == ref_stats[name] + added.get(name, 0), name
    # each kind alone: nothing is drawn and exactly its counter is 1
    extras = f[np.setdiff1d(np.arange(len(f)), kept)]
    names = ["non_finite"] * 3 + ["guard_band"] + ["zero_area"] * 2 + ["bad_index"] * 2 + ["zero_area"]
    assert len(extras) == len(names)
    for extra, name in zip(extras, names):
        face_id, depth, stats = R.rasterize_cpu(v, extra[None], cam, 64, 64)
        assert (face_id == -1).all() and np.isinf(depth).all()
        assert stats == {n: int(n == name) for n in R.STATS}, (extra, name, stats)
    # the near plane of the LIST camera: behind it, straddling it (dropped whole) and exactly on it
    (v, f), z_near, n_behind = RC.near_plane_faces(64)
    lcam = RC.list_pixel_camera(64)
    face_id, depth, stats = R.rasterize_cpu(v, f, lcam, 64, 64, z_near=z_near)
    assert stats["behind_near"] == n_behind and stats["small"] + stats["large"] == 1
    assert set(np.unique(face_id)) == {-1, 0}
    assert R.rasterize_cpu(v, f, lcam, 64, 64, z_near=0.05)[2]["behind_near"] == 1       # only the one behind the camera


def test_empty_meshes_give_background():
    R = _R()
    cam = RC.pixel_camera()
    for v, f in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
                 (np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32)),
                 (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))):
        face_id, depth, stats = R.rasterize_cpu(v, f, cam, 7, 9)
        assert face_id.shape == (7, 9) and face_id.dtype == np.int32 and depth.dtype == np.float32
        assert (face_id == -1).all() and np.isposinf(depth).all()
        assert stats["bad_index"] == len(f) and sum(stats.values()) == len(f)
        rgb = R.shade_cpu(v, f, face_id, cam)
        assert rgb.shape == (7, 9, 3) and (rgb == 255).all()


# ---- a sphere from marching cubes against the analytic sphere ---------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_mesh():
    from list_amd import mesh
    v, f = mesh.marching_cubes_cpu(RC.sphere_field(32, 0.3))
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sphere_depth_and_silhouette(sphere_mesh, axis):
    """Radius r = 0.3 on a 32^3 grid of step h = 1/31, seen along `axis` at 64^2 (pixel pitch p = 1/63).

    Where the mesh lies.  The field is the exact signed distance f = r - |x|.  A mesh vertex is the root of the LINEAR
    interpolant of f along a grid edge; along that edge |f''| <= 1 / |x| <= 1 / (r - h), so the interpolant differs from f
    by at most h^2 / 8 / (r - h), and at the interpolant's root that difference IS the vertex's distance from the sphere:
    d1 = h^2 / (8 (r - h)).  A facet lies in one cell, so its vertices are at most L = sqrt(3) h apart.  A point q of the
    facet is a convex combination of vertices v_i with |v_i| in [r - d1, r + d1]: |q| <= r + d1 by convexity, and
    |q|^2 = sum l_i |v_i|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= (r - d1)^2 - L^2 / 3 = (r - d1)^2 - h^2.  So the surface
    lies in the shell r_in = sqrt((r - d1)^2 - h^2) <= |x| <= r_out = r + d1 (both O(h^2 / r) from r: the facet sagitta and
    the interpolation error).  The rasteriser moves a vertex sideways by at most s = p / 32 (snapping to 1/16 pixel) plus
    the float32 rounding of the projection (below 1e-4 p); that widens the shell to [r_in - s, r_out + s].

    Depth.  The mesh is closed and surrounds the inner ball, so the ray of a pixel at distance rho < r_in - s from the axis
    first meets it between the two spheres: -sqrt((r_out + s)^2 - rho^2) <= depth <= -sqrt((r_in - s)^2 - rho^2), and the
    analytic depth -sqrt(r^2 - rho^2) lies in the same interval: the bound on their difference is the interval's length,
    checked per pixel (plus 1e-6 for the float32 depth) for rho <= r_in - s - p, i.e. minus a one-pixel rim.

    Silhouette.  Every pixel with rho < r_in - s is covered and none with rho > r_out + s, so the count lies between those
    of the discs of radius r -+ (h^2 / r + p), which contain / are contained in those two (asserted)."""
    R = _R()
    v, f = sphere_mesh
    size, r, h = 64, 0.3, 1.0 / 31.0
    p = 1.0 / (size - 1)
    d1 = h * h / (8.0 * (r - h))
    s = p / 32.0 + 1e-4 * p
    r_in, r_out = np.sqrt((r - d1) ** 2 - h * h) - s, r + d1 + s
    assert r - (h * h / r + p) < r_in and r_out < r + (h * h / r + p)
    face_id, depth, stats = R.rasterize_cpu(v, f, R.Camera.orthographic(axis, size, size), size, size)
    # (a face seen edge-on has no area after snapping; one between two centres has none in its box)
    assert stats["small"] + stats["large"] + stats["offscreen"] + stats["zero_area"] == len(f) and stats["small"] > 2000
    c = -0.5 + np.arange(size) * p
    rho = np.sqrt(c[:, None] ** 2 + c[None, :] ** 2)
    hit = face_id >= 0
    assert hit[rho < r_in].all() and not hit[rho > r_out].any()
    assert (rho <= r - (h * h / r + p)).sum() <= hit.sum() <= (rho <= r + (h * h / r + p)).sum()
    core = rho <= r_in - p
    assert core.sum() > 800
    lo, hi = -np.sqrt(r_out ** 2 - rho[core] ** 2), -np.sqrt(r_in ** 2 - rho[core] ** 2)
    exact = -np.sqrt(r * r - rho[core] ** 2)
    got = depth[core].astype(np.float64)
    assert (got >= lo - 1e-6).all() and (got <= hi + 1e-6).all()
    assert (np.abs(got - exact) <= (hi - lo) + 1e-6).all()
    # the three views of a sphere centred in the box are the same picture up to the facets: same silhouette size +- rim
    assert abs(int(hit.sum()) - int((rho <= r).sum())) <= (rho <= r_out).sum() - (rho < r_in).sum()


# ---- the model's own projection -----------------------------------------------------------------------------------------------
def test_list_camera_is_the_query_paths_projection():
    """The unsnapped float32 (u, v) equal oracle.list_oracle.project_points bit for bit wherever the reference's clamp to
    [0, 136] is inactive: the picture shows where the network samples the image."""
    from list_amd import synthetic
    from oracle import list_oracle
    R = _R()
    T = synthetic.make_trans_mat(21, 3)
    rng = np.random.default_rng(3)
    n_checked = 0
    for b in range(3):
        v = rng.uniform(-0.5, 0.5, (500, 3)).astype(np.float32)
        cam = R.Camera.from_transmat(T[b])
        uv = R.project_uv(v, cam)
        pc = (v[:, ::-1] * np.float32(2)).astype(np.float32)              # models.py:91-92: query[:, :, [2,1,0]] * 2
        xy, _ = list_oracle.project_points(pc[None], T[b:b + 1])
        free = ((xy[0] > 0) & (xy[0] < 136)).all(axis=1)
        n_checked += int(free.sum())
        assert uv.dtype == np.float32 and uv[free].tobytes() == np.ascontiguousarray(xy[0][free]).tobytes()
    assert n_checked > 1000
    # ... and rasterize puts a small triangle around such a point onto the pixel u * (W-1)/136, v * (H-1)/136
    cam = R.Camera.from_transmat(T[0])
    centre = np.array([0.1, -0.2, 0.15], dtype=np.float32)
    u, w = R.project_uv(centre[None], cam)[0].astype(np.float64)
    e = 0.02
    tri_v = (centre[None] + np.array([[0, -e, -e], [0, e, -e], [0, 0, e]], dtype=np.float32)).astype(np.float32)
    face_id = R.rasterize_cpu(tri_v, np.array([[0, 1, 2]]), cam, 224, 224)[0]
    ys, xs = np.nonzero(face_id == 0)
    assert len(xs) > 3
    assert abs(xs.mean() - u * 223 / 136) < 1.5 and abs(ys.mean() - w * 223 / 136) < 1.5


# ---- shading ------------------------------------------------------------------------------------------------------------------
def test_shade_by_hand():
    """a = (z 1, y 0, x 0), b = (1, 0, 4), c = (1, 4, 0): n = (b - a) x (c - a) = (0, 0, 4) x (0, 4, 0) = (-16, 0, 0), the
    unit normal (-1, 0, 0) in mesh axis order, so the normal map is (round(0 * 255), round(127.5), round(127.5)) =
    (0, 128, 128) with halves rounded up.  Seen along axis 0 the head-light meets it squarely: grey 255."""
    R = _R()
    cam = RC.pixel_camera()
    v = np.array([[1, 0, 0], [1, 0, 4], [1, 4, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    face_id = R.rasterize_cpu(v, f, cam, 6, 6)[0]
    on = face_id == 0
    assert on.sum() == 10
    rgb = R.shade_cpu(v, f, face_id, cam, "normal")
    assert rgb.dtype == np.uint8 and (rgb[on] == (0, 128, 128)).all() and (rgb[~on] == 255).all()
    assert (R.shade_cpu(v, f[:, ::-1], face_id, cam, "normal")[on] == (255, 128, 128)).all()     # the other winding
    grey = R.shade_cpu(v, f, face_id, cam, "lambert")
    assert (grey[on] == 255).all() and (grey[~on] == 255).all()
    # tilted by 60 degrees about the y axis: n = (0, 0, 4) x ... -> |cos| = 0.5 -> round(127.5) = 128
    t = np.array([[0, 0, 0], [np.sqrt(3.0) * 2, 0, 2], [0, 4, 0]], dtype=np.float32)     # b - a = (2 sqrt 3, 0, 2)
    tilted = R.shade_cpu(t, f, np.zeros((1, 1), np.int32), cam, "lambert")
    assert abs(int(tilted[0, 0, 0]) - 128) <= 1 and len(set(tilted[0, 0].tolist())) == 1
    # over a background: alpha 0 gives it back byte for byte, alpha 1 the mesh's colour, 0.5 the rounded mean
    bg = np.random.default_rng(1).integers(0, 256, (6, 6, 3), dtype=np.uint8)
    assert R.shade_cpu(v, f, face_id, cam, "normal", bg, 0.0).tobytes() == bg.tobytes()
    full = R.shade_cpu(v, f, face_id, cam, "normal", bg, 1.0)
    assert (full[on] == (0, 128, 128)).all() and (full[~on] == bg[~on]).all()
    half = R.shade_cpu(v, f, face_id, cam, "normal", bg, 0.5)
    expect = (128 * np.array([0, 128, 128]) + 128 * bg[on].astype(np.int64) + 128) >> 8
    assert (half[on] == expect).all() and (half[~on] == bg[~on]).all()


# ---- the header on the host == the restatement ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return RC.build_host(tmp_path_factory.mktemp("render_host"))


def host_cases():
    valid = RC.small_triangles(300, 64, seed=5)
    dv, df, _ = RC.with_dropped_faces(valid)
    from list_amd import mesh
    sv, sf = mesh.marching_cubes_cpu(RC.three_spheres(24))
    near, z_near, _ = RC.near_plane_faces(64)
    return {
        "small": (RC.small_triangles(2000), RC.pixel_camera(), 64, 64, 1e-6),
        "large": (RC.large_triangles(40), RC.pixel_camera(), 64, 64, 1e-6),
        "both_paths_with_ties": (RC.interleave(RC.small_triangles(400, flat=True), RC.large_triangles(40, flat=True)),
                                 RC.pixel_camera(), 64, 64, 1e-6),
        "boundary": (RC.boundary_triangles()[0], RC.pixel_camera(), 64, 64, 1e-6),
        "copies": (RC.copies(500), RC.pixel_camera(), 64, 64, 1e-6),
        "coplanar": (RC.coplanar(), RC.pixel_camera(), 64, 64, 1e-6),
        "dropped": ((dv, df), RC.pixel_camera(), 64, 64, 1e-6),
        "near_plane": (near, RC.list_pixel_camera(64), 64, 64, z_near),
        "large_list_camera": (RC.large_triangles(40), RC.list_pixel_camera(64), 17, 33, 1e-6),
        "spheres_list_camera": ((sv, sf), RC.synthetic_list_camera(), 96, 80, 1e-6),
        "spheres_axis_1": ((sv, sf), _R().Camera.orthographic(1, 50, 70), 50, 70, 1e-6),
        "one_pixel": (RC.large_triangles(8), RC.pixel_camera(), 1, 1, 1e-6),
    }


@pytest.mark.parametrize("name", ["small", "large", "both_paths_with_ties", "boundary", "copies", "coplanar", "dropped",
                                  "near_plane", "large_list_camera", "spheres_list_camera", "spheres_axis_1", "one_pixel"])
def test_header_on_the_host_equals_the_restatement(host_exe, tmp_path, name):
    """csrc/render_math.h -- the code the kernels run -- as a sequential host program against render.py, bit for bit:
    face ids, depth bytes, every counter, and the shaded bytes in both modes over a background."""
    R = _R()
    (v, f), cam, Hh, Ww, z_near = host_cases()[name]
    bg = np.random.default_rng(2).integers(0, 256, (Hh, Ww, 3), dtype=np.uint8)
    face_id, depth, stats = R.rasterize_cpu(v, f, cam, Hh, Ww, z_near)
    for mode, alpha, back in (("lambert", 0.65, bg), ("normal", 1.0, None)):
        h_id, h_depth, h_stats, h_rgb = RC.run_host(host_exe, tmp_path, v, f, cam, Hh, Ww, z_near, mode, back, alpha)
        assert np.array_equal(h_id, face_id)
        assert h_depth.tobytes() == depth.tobytes()
        assert h_stats == stats
        assert h_rgb.tobytes() == R.shade_cpu(v, f, face_id, cam, mode, back, alpha).tobytes()
    if name not in ("dropped", "near_plane", "one_pixel"):
        assert (face_id >= 0).any()
    if name == "small":
        assert stats["large"] == 0 and stats["small"] > 1000
    if name == "large":
        assert stats == {**{n: 0 for n in R.STATS}, "large": 40}
    if name == "both_paths_with_ties":
        assert stats["small"] > 300 and stats["large"] == 40
    if name == "boundary":
        assert [R.STATS[o] for o in R.face_outcomes_cpu(v, f, cam, Hh, Ww)] == RC.boundary_triangles()[1]
    if name == "copies":
        assert set(np.unique(face_id)) == {-1, 0}


def test_coplanar_ties_go_to_the_lowest_index():
    """64 overlapping triangles in one plane: every pixel's winner is the lowest-numbered face that covers it alone."""
    R = _R()
    cam = RC.pixel_camera()
    v, f = RC.coplanar()
    face_id = R.rasterize_cpu(v, f, cam, 64, 64)[0]
    lowest = np.full((64, 64), -1, dtype=np.int64)
    for k in reversed(range(len(f))):
        lowest[R.rasterize_cpu(v, f[k:k + 1], cam, 64, 64)[0] >= 0] = k
    assert np.array_equal(face_id, lowest) and len(np.unique(face_id)) > 20


# ---- C ABI, parser, public interface ------------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    import __graft_entry__ as ge
    ge.build()
    from list_amd import hip
    R = _R()
    names, exported = H.declared("list_render.h"), H.exported(hip.LIB_PATH)
    assert names == sorted(R.RENDER_EXPORTS)
    assert {n for n in exported if n.startswith("list_render_")} == set(names)
    taken = tuple(p for _, _, prefixes in H.SECTIONS.values() if prefixes for p in prefixes) + ("list_cc_",)
    assert not any(n.startswith(taken) for n in names)
    assert not set(names) & set(hip.EXPORTS) and not any(n.startswith("list_render_") for n in hip.EXPORTS)
    raw, lib = ctypes.CDLL(hip.LIB_PATH), R.load()
    for name in names:
        assert hasattr(raw, name) and getattr(lib, name) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9
    text = open(os.path.join(H.ROOT, "include", "list_render.h")).read()
    for macro, value in (("LIST_RENDER_CAP", R.CAP), ("LIST_RENDER_LARGE_GROUPS", R.LARGE_GROUPS),
                         ("LIST_RENDER_N_STATS", len(R.STATS)), ("LIST_RENDER_N_STEPS", R.N_STEPS),
                         ("LIST_RENDER_MAX_SIDE", R.MAX_SIDE), ("LIST_RENDER_LIST", R.LIST), ("LIST_RENDER_ORTHO", R.ORTHO)):
        assert f"#define {macro} {value}\n" in text, macro
    assert "#define LIST_RENDER_MAX_PIXELS (1 << 26)" in text and R.MAX_PIXELS == 1 << 26
    assert ctypes.sizeof(R.ListRenderCamera) == 72


def test_refusals_without_gpu():
    """Argument checks come before any HIP call, each with its text in list_render_last_error; other sections' texts stay."""
    from list_amd import hip, mesh
    R = _R()
    lib = R.load()
    assert mesh.load().list_mc_workspace_bytes(1, 1, 1) == 0
    before = lib.list_mesh_last_error()
    assert lib.list_render_workspace_bytes(10, 64, 64) >= 8 * 64 * 64 + 4 * 10
    assert lib.list_render_workspace_bytes(0, 1, 1) > 0
    assert lib.list_render_workspace_bytes(10, 0, 64) == 0 and b"LIST_RENDER_MAX_SIDE" in lib.list_render_last_error()
    assert lib.list_render_workspace_bytes(10, R.MAX_SIDE + 1, 1) == 0
    assert lib.list_render_workspace_bytes(10, R.MAX_SIDE, R.MAX_SIDE) == 0           # H * W beyond MAX_PIXELS
    assert lib.list_render_workspace_bytes(2 ** 31, 64, 64) == 0 and b"INT32_MAX" in lib.list_render_last_error()
    buf = ctypes.create_string_buffer(256)                                      # never dereferenced: every call is refused
    p = ctypes.addressof(buf)
    cam = RC.pixel_camera().struct()
    args = lambda **k: [k.get("verts", p), k.get("V", 9), p, k.get("F", 3), k.get("cam", ctypes.byref(cam)),       # noqa: E731
                        k.get("H", 8), k.get("W", 8), k.get("z_near", 1e-6), k.get("ws", p), k.get("bytes", 1 << 20), p,
                        k.get("depth", p), p, k.get("b", 0), k.get("e", 4), None]
    assert lib.list_render_rasterize(*args(F=2 ** 31)) == hip.ERR_SHAPE
    assert lib.list_render_rasterize(*args(H=R.MAX_SIDE + 1)) == hip.ERR_SHAPE
    assert lib.list_render_rasterize(*args(cam=None)) == hip.ERR_ARG and b"camera is NULL" in lib.list_render_last_error()
    bad = RC.pixel_camera().struct()
    bad.mode = 2
    assert lib.list_render_rasterize(*args(cam=ctypes.byref(bad))) == hip.ERR_ARG
    bad.mode, bad.map_size = R.LIST, 1
    assert lib.list_render_rasterize(*args(cam=ctypes.byref(bad))) == hip.ERR_ARG and b"map_size" in lib.list_render_last_error()
    assert lib.list_render_rasterize(*args(z_near=-1.0)) == hip.ERR_ARG and b"z_near" in lib.list_render_last_error()
    assert lib.list_render_rasterize(*args(z_near=float("nan"))) == hip.ERR_ARG
    assert lib.list_render_rasterize(*args(verts=None)) == hip.ERR_ARG and b"NULL" in lib.list_render_last_error()
    assert lib.list_render_rasterize(*args(depth=None)) == hip.ERR_ARG
    assert lib.list_render_rasterize(*args(ws=p + 4)) == hip.ERR_ARG and b"aligned" in lib.list_render_last_error()
    assert lib.list_render_rasterize(*args(b=2, e=5)) == hip.ERR_ARG and b"steps" in lib.list_render_last_error()
    assert lib.list_render_rasterize(*args(bytes=64)) == hip.ERR_WORKSPACE
    assert b"list_render_workspace_bytes" in lib.list_render_last_error()
    shade = lambda **k: [p, 9, p, 3, k.get("ids", p), ctypes.byref(cam), 8, 8, k.get("shade", 1), None,        # noqa: E731
                         k.get("alpha", 256), k.get("rgb", p), None]
    assert lib.list_render_shade(*shade(shade=2)) == hip.ERR_ARG and b"shade" in lib.list_render_last_error()
    assert lib.list_render_shade(*shade(alpha=257)) == hip.ERR_ARG and b"alpha256" in lib.list_render_last_error()
    assert lib.list_render_shade(*shade(ids=None)) == hip.ERR_ARG
    assert lib.list_render_shade(*shade(rgb=None)) == hip.ERR_ARG
    assert lib.list_mesh_last_error() == before
    # the Python side refuses the same way, in the section's own error
    v, f = RC.tri([[(1, 1, 1), (5, 1, 1), (1, 5, 1)]])
    for bad_call in (lambda: R.rasterize_cpu(v, f, RC.pixel_camera(), 0, 8),
                     lambda: R.rasterize_cpu(v, f, RC.pixel_camera(), R.MAX_SIDE, R.MAX_SIDE),
                     lambda: R.rasterize_cpu(v, f, RC.pixel_camera(), 8, 8, z_near=-1),
                     lambda: R.shade_cpu(v, f, np.zeros((4, 4), np.int32), RC.pixel_camera(), "phong"),
                     lambda: R.shade_cpu(v, f, np.zeros((4, 4), np.int32), RC.pixel_camera(), alpha=1.5)):
        with pytest.raises(hip.ListError):
            bad_call()


def test_cameras():
    R = _R()
    # orthographic: the first of the two remaining axes runs down the rows, bb_min at pixel 0 and bb_max at size - 1
    for axis, (rows, cols) in enumerate([(1, 2), (0, 2), (0, 1)]):
        cam = R.Camera.orthographic(axis, 33, 65, -0.5, 0.5)
        assert cam.mode == R.ORTHO and cam.eye.tolist() == [float(axis == k) for k in range(3)] + [0.0]
        lo, hi = np.full(3, -0.5, np.float32), np.full(3, 0.5, np.float32)
        mid = np.zeros(3, np.float32)
        mid[axis] = 0.25
        X, Y, Z = (np.array(c) for c in R._chain(cam.T, np.stack([lo, hi, mid])))
        assert np.allclose(X, [0, 64, 32], atol=1e-4) and np.allclose(Y, [0, 32, 16], atol=1e-4)
        assert Z.tolist() == [-0.5, 0.5, 0.25]
        e = np.zeros(3, np.float32)
        e[rows] = 0.5
        assert np.allclose([c[0] for c in R._chain(cam.T, e[None])][:2], [32, 32], atol=1e-4)
    # the centre of a perspective camera: every vertex on a ray through it lands on one pixel
    from list_amd import synthetic
    T = synthetic.make_trans_mat(5, 1)[0].copy()
    T[2] = (3.0, -2.0, 0.4)                                     # a real perspective: den varies with p[2]
    cam = R.Camera.from_transmat(T)
    assert cam.mode == R.LIST and cam.map_size == 137 and abs(np.abs(cam.eye).max() - 1) < 1e-6 and cam.eye[3] != 0
    centre = cam.eye[:3].astype(np.float64) / cam.eye[3]
    a = np.array([0.1, -0.2, 0.3])
    ray = np.stack([a, a + 0.3 * (centre - a)]).astype(np.float32)
    uv = R.project_uv(ray, cam).astype(np.float64)
    assert np.allclose(uv[0], uv[1], rtol=0, atol=2e-3)
    with pytest.raises(ValueError):
        R.Camera.orthographic(3, 8, 8)
    with pytest.raises(ValueError):
        R.Camera.from_transmat(np.zeros((3, 3)))


def test_parser_defaults():
    from list_amd import arguments
    cfg = arguments.default_config()
    assert cfg.render_pred == "none" and cfg.render_size == 0
    cfg = arguments.get_args(["--render_pred", "both", "--render_size", "96"])
    assert cfg.render_pred == "both" and cfg.render_size == 96
    with pytest.raises(SystemExit):
        arguments.get_args(["--render_pred", "all"])


@pytest.fixture(scope="module")
def small_mesh():
    from list_amd import mesh
    return mesh.Mesh(*mesh.marching_cubes_cpu(RC.three_spheres(24)))


def test_mesh_render(small_mesh):
    R = _R()
    cam = R.Camera.orthographic(2, 40, 48)
    rgb = small_mesh.render(cam, 40, 48)
    assert rgb.shape == (40, 48, 3) and rgb.dtype == np.uint8
    face_id = R.rasterize_cpu(small_mesh.vertices, small_mesh.faces, cam, 40, 48)[0]
    assert rgb.tobytes() == R.shade_cpu(small_mesh.vertices, small_mesh.faces, face_id, cam, "lambert").tobytes()
    assert (rgb[face_id < 0] == 255).all() and (face_id >= 0).sum() > 100
    normal = small_mesh.render(cam, 40, 48, mode="normal")
    assert not np.array_equal(normal, rgb) and (normal[face_id < 0] == 255).all()
    from list_amd import mesh
    empty = mesh.Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)).render(cam, 40, 48)
    assert (empty == 255).all()


def _executor(**config):
    from list_amd import arguments
    from list_amd.network import executors
    cfg = arguments.default_config(**config)
    return executors.LIST(cfg, SimpleNamespace())              # render_views and save need no network


def test_executor_writes_pictures_only_when_asked(small_mesh, tmp_path):
    import torch
    from PIL import Image
    from list_amd import synthetic
    R = _R()
    batch = {"rgb_image": torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(1)),
             "transmat": torch.from_numpy(synthetic.make_trans_mat(3, 1))}
    pred = [small_mesh, None, None]
    os.makedirs(tmp_path / "plain")
    plain = _executor()                                                          # no flag at all
    assert plain.render_pred == "none" and plain.last_transmat is None
    plain.save(batch, pred, str(tmp_path / "plain" / "a"))
    assert sorted(os.listdir(tmp_path / "plain")) == ["a_pred.obj"]
    for which, names in (("none", []), ("view", ["view"]), ("canonical", ["x", "y", "z"]), ("both", ["view", "x", "y", "z"])):
        os.makedirs(tmp_path / which)
        ex = _executor(render_pred=which, render_size=48)
        ex.save(batch, pred, str(tmp_path / which / "a"))
        assert sorted(os.listdir(tmp_path / which)) == sorted(["a_pred.obj"] + [f"a_pred_{n}.png" for n in names])
        assert open(tmp_path / which / "a_pred.obj", "rb").read() == open(tmp_path / "plain" / "a_pred.obj", "rb").read()
        for n in names:
            img = np.asarray(Image.open(tmp_path / which / f"a_pred_{n}.png"))
            assert img.shape == (48, 48, 3) and img.dtype == np.uint8
            assert len(np.unique(img.reshape(-1, 3), axis=0)) > 10, n            # a picture, not a blank
    views = _executor(render_pred="both", render_size=48).render_views(batch, pred)
    assert list(views) == ["view", "x", "y", "z"]
    cam = R.Camera.orthographic(0, 48, 48)
    assert views["x"].tobytes() == small_mesh.render(cam, 48, 48).tobytes()
    # the view is the mesh from the batch's camera over the input image: where the mesh is not, the resized image shows
    cam = R.Camera.from_transmat(batch["transmat"][0])
    face_id = R.rasterize_cpu(small_mesh.vertices, small_mesh.faces, cam, 48, 48)[0]
    bg = plain._input_image(batch, 48)
    assert (face_id >= 0).sum() > 50 and (views["view"][face_id < 0] == bg[face_id < 0]).all()
    assert not (views["view"][face_id >= 0] == bg[face_id >= 0]).all()
    # the executor's own camera (what predict_grid used) takes precedence over the batch's
    ex = _executor(render_size=48)
    ex.last_transmat = torch.from_numpy(synthetic.make_trans_mat(4, 1))
    assert not np.array_equal(ex.render_views(batch, pred, "view")["view"], views["view"])
    # a mesh without a face: background-only pictures, no error
    from list_amd import mesh
    nothing = _executor(render_size=16).render_views(batch, mesh.Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32)))
    assert (nothing["x"] == 255).all() and nothing["view"].tobytes() == plain._input_image(batch, 16).tobytes()
    with pytest.raises(ValueError):
        _executor(render_pred="everything")
