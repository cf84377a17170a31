"""GPU: the rasteriser in HIP (include/list_render.h, render.rasterize / shade) against its numpy restatement
(rasterize_cpu / shade_cpu, themselves held to hand-made facts and to the header on the host in test_render_cpu.py).
Everything compared is an integer or the bits of a float32: exact equality, no tolerance."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_cases as RC   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def _R():
    from list_amd import render
    return render


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(mesh, camera, H, W, z_near=1e-6, shade=(("lambert", None, 1.0),)):
    """Device rasterize and shade of the mesh == the restatement's: face ids, depth as bytes, every counter, shaded bytes.
    Returns the restatement's (face_id, depth, stats)."""
    R = _R()
    v, f = mesh
    dv, df = dev(np.asarray(v, dtype=np.float32).reshape(-1, 3)), dev(np.asarray(f, dtype=np.int32).reshape(-1, 3))
    face_id, depth, stats = R.rasterize(dv, df, camera, H, W, z_near)
    ref_id, ref_depth, ref_stats = R.rasterize_cpu(v, f, camera, H, W, z_near)
    assert face_id.dtype == torch.int32 and depth.dtype == torch.float32 and face_id.is_cuda and depth.is_cuda
    assert tuple(face_id.shape) == (H, W) == tuple(depth.shape)
    assert stats == ref_stats, (stats, ref_stats)
    got_id = face_id.cpu().numpy()
    assert np.array_equal(got_id, ref_id), f"{int((got_id != ref_id).sum())} face ids differ"
    assert depth.cpu().numpy().tobytes() == ref_depth.tobytes(), "depth"
    for mode, background, alpha in shade:
        rgb = R.shade(dv, df, face_id, camera, mode, None if background is None else dev(background), alpha)
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and tuple(rgb.shape) == (H, W, 3)
        ref = R.shade_cpu(v, f, ref_id, camera, mode, background, alpha)
        assert rgb.cpu().numpy().tobytes() == ref.tobytes(), (mode, alpha)
    return ref_id, ref_depth, ref_stats


def test_small_path_only():
    """2 000 random triangles of 1 - 6 pixels on 64 x 64: every one stays in its thread."""
    _, _, stats = check(RC.small_triangles(2000), RC.pixel_camera(), 64, 64)
    assert stats["large"] == 0 and stats["small"] > 1000 and stats["offscreen"] > 0


def test_large_path_only():
    """40 triangles spanning up to the whole image, four of them mostly off-screen, one on each side."""
    R = _R()
    v, f = RC.large_triangles(40)
    ref_id, _, stats = check((v, f), RC.pixel_camera(), 64, 64)
    assert stats == {**{n: 0 for n in R.STATS}, "large": 40} and (ref_id >= 0).mean() > 0.5
    for k in range(4):                                                           # the mostly off-screen ones, each alone
        alone, _, _ = check((v, f[k:k + 1]), RC.pixel_camera(), 64, 64)
        assert 0 < (alone == 0).sum() < 64 * 64 // 2


def test_cap_boundary_and_both_paths_on_one_image():
    R = _R()
    cam = RC.pixel_camera()
    mesh, expected = RC.boundary_triangles()
    assert [R.STATS[o] for o in R.face_outcomes_cpu(*mesh, cam, 64, 64)] == expected
    _, _, stats = check(mesh, cam, 64, 64)
    assert stats["small"] == expected.count("small") and stats["large"] == expected.count("large")
    # small and large faces alternate in the face list and all lie in one plane: every overlap is a tie across the paths
    both = RC.interleave(RC.small_triangles(400, flat=True), RC.large_triangles(40, flat=True))
    ref_id, ref_depth, stats = check(both, cam, 64, 64)
    assert stats["small"] > 200 and stats["large"] == 40 and (ref_depth[ref_id >= 0] == 1.0).all()
    outcome = R.face_outcomes_cpu(*both, cam, 64, 64)
    winners = np.unique(ref_id[ref_id >= 0])
    assert (outcome[winners] == 6).any() and (outcome[winners] == 7).any()
    # the same with depths: nearest wins, across the paths too
    check(RC.interleave(RC.small_triangles(400), RC.large_triangles(40)), cam, 64, 64)


def test_atomic_ties_go_to_the_lowest_index():
    cam = RC.pixel_camera()
    ref_id, _, stats = check(RC.copies(5000), cam, 64, 64)
    assert stats["large"] == 5000 and set(np.unique(ref_id)) == {-1, 0} and (ref_id == 0).sum() > 800
    ref_id, _, _ = check(RC.coplanar(64), cam, 64, 64)
    assert len(np.unique(ref_id)) > 20


def test_drop_rules():
    R = _R()
    valid = RC.small_triangles(300, 64, seed=5)
    v, f, added = RC.with_dropped_faces(valid)
    _, _, stats = check((v, f), RC.pixel_camera(), 64, 64, shade=(("normal", None, 1.0),))
    for name, n in added.items():
        assert stats[name] >= n
    assert stats["non_finite"] == 3 and stats["guard_band"] == 1 and stats["bad_index"] == 2
    # LIST camera: behind the camera, straddling z_near (dropped whole), exactly on it; the dropped kinds again
    mesh, z_near, n_behind = RC.near_plane_faces(64)
    ref_id, _, stats = check(mesh, RC.list_pixel_camera(64), 64, 64, z_near)
    assert stats["behind_near"] == n_behind and set(np.unique(ref_id)) == {-1, 0}
    v = v.copy()
    v[:, 0] = np.where(np.isfinite(v[:, 0]), np.abs(v[:, 0]) + 0.5, v[:, 0])          # den > 0 where it is finite
    _, _, stats = check((v, f), RC.list_pixel_camera(64), 64, 64, shade=(("lambert", None, 1.0),))
    assert stats["non_finite"] == 3 and stats["bad_index"] == 2 and stats["small"] > 50 and stats["large"] > 50


@pytest.mark.parametrize("H,W", [(1, 1), (17, 33), (224, 224)])
def test_image_shapes(H, W):
    s = max(H, W, 64)                                                            # the cases are made at >= 64 pixels
    v, f = RC.join([RC.small_triangles(600, s, seed=3), RC.large_triangles(30, s, seed=4)])
    scale = np.array([1.0, H / s, W / s], dtype=np.float32)                      # (z, y, x): fill the H x W image
    ref_id, _, stats = check(((v * scale).astype(np.float32), f), RC.pixel_camera(), H, W)
    assert (ref_id >= 0).any() and stats["small"] + stats["large"] > 0
    check(((v * scale).astype(np.float32), f), RC.list_pixel_camera(max(s, 2)), H, W)


def test_face_counts_and_unused_vertices():
    R = _R()
    cam = RC.pixel_camera()
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    ref_id, ref_depth, stats = check(none, cam, 9, 7)                              # F = 0, V = 0
    assert (ref_id == -1).all() and np.isposinf(ref_depth).all() and sum(stats.values()) == 0
    check((np.zeros((5, 3), np.float32), none[1]), cam, 9, 7)                      # F = 0, V = 5
    check((none[0], np.array([[0, 1, 2]], np.int32)), cam, 9, 7)                   # V = 0: the face's indices are invalid
    one = RC.tri([[(1, 1, 2), (6, 2, 2), (2, 7, 2)]])
    ref_id, _, _ = check(one, cam, 9, 7)                                           # F = 1
    assert (ref_id == 0).sum() > 5
    # more large faces than persistent workgroups: the list loop wraps
    many = RC.large_triangles(R.LARGE_GROUPS + 44, 64, seed=8)
    _, _, stats = check(many, cam, 64, 64)
    assert stats["large"] == R.LARGE_GROUPS + 44
    # vertices no face uses, NaN among them, before, between and behind the used ones
    v, f = RC.small_triangles(200, 64, seed=9)
    pad = np.full((7, 3), np.nan, dtype=np.float32)
    v2 = np.concatenate([pad, v[:300], pad, v[300:], pad]).astype(np.float32)
    f2 = np.where(f < 300, f + 7, f + 14).astype(np.int32)
    a = check((v, f), cam, 64, 64)
    b = check((v2, f2), cam, 64, 64)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_list_camera_on_a_marching_cubes_mesh():
    """Three spheres -> mesh.marching_cubes at 48^3 -> keep_components(keep=1) -> rasterize from a synthetic trans_mat: the
    device's picture equals the restatement's, the kept sphere is there and the dropped ones leave no pixel."""
    from list_amd import components, mesh
    R = _R()
    cam = RC.synthetic_list_camera()
    vol = dev(RC.three_spheres(48))
    v_all, f_all = mesh.marching_cubes(vol)
    v, f, info = components.keep_components(v_all, f_all, keep=1)
    assert info["K"] == 3 and len(info["kept"]) == 1
    S = 137
    face_id, depth, stats = R.rasterize(v, f, cam, S, S)
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    ref_id, ref_depth, ref_stats = R.rasterize_cpu(hv, hf, cam, S, S)
    assert np.array_equal(face_id.cpu().numpy(), ref_id) and depth.cpu().numpy().tobytes() == ref_depth.tobytes()
    assert stats == ref_stats and stats["small"] > 1000 and stats["bad_index"] == 0
    hit = ref_id >= 0
    assert hit.sum() > 500
    # where each sphere's centre projects (S = map_size: pixel = (u, v)); radii through the camera's ~60 pixels per unit of p
    centres = np.array([c for _, c in RC.THREE_SPHERES], dtype=np.float32)
    uv = R.project_uv(centres, cam).astype(np.float64)
    ys, xs = np.nonzero(hit)
    d_big = np.hypot(xs - uv[0, 0], ys - uv[0, 1])
    assert d_big.max() < 0.25 * 2 * 60 * 1.25 and hit[int(round(uv[0, 1])), int(round(uv[0, 0]))]
    for k in (1, 2):                                                               # the dropped spheres: no pixel near them
        r_px = RC.THREE_SPHERES[k][0] * 2 * 60
        assert np.hypot(xs - uv[k, 0], ys - uv[k, 1]).min() > r_px
    full = R.rasterize(v_all, f_all, cam, S, S)[0].cpu().numpy()                   # ... which the unfiltered mesh does paint
    assert (full >= 0).sum() > hit.sum() + 50
    assert np.array_equal(full, R.rasterize_cpu(v_all.cpu().numpy(), f_all.cpu().numpy(), cam, S, S)[0])
    # Mesh.render and an orthographic view of the same device mesh
    m = mesh.Mesh(v, f)
    ocam = R.Camera.orthographic(1, 96, 80)
    assert m.render(ocam, 96, 80).tobytes() == mesh.Mesh(hv, hf).render(ocam, 96, 80).tobytes()


def test_shade_modes_backgrounds_and_alphas():
    from list_amd import mesh
    R = _R()
    v, f = mesh.marching_cubes_cpu(RC.three_spheres(24))
    bg = np.random.default_rng(6).integers(0, 256, (60, 52, 3), dtype=np.uint8)
    shades = [(mode, back, alpha) for mode in ("normal", "lambert") for back in (None, bg) for alpha in (0.0, 0.5, 1.0)]
    for cam in (R.Camera.orthographic(0, 60, 52), RC.synthetic_list_camera()):
        ref_id, _, _ = check((v, f), cam, 60, 52, shade=shades)
        assert (ref_id >= 0).sum() > 200
    # alpha 0 over a background is the background, byte for byte
    cam = R.Camera.orthographic(0, 60, 52)
    dv, df = dev(v), dev(f)
    face_id = R.rasterize(dv, df, cam, 60, 52)[0]
    assert R.shade(dv, df, face_id, cam, "lambert", dev(bg), 0.0).cpu().numpy().tobytes() == bg.tobytes()
    # a face id outside [0, F) is background, never an address
    wild = torch.tensor([[-1, len(f), 2 ** 31 - 1, -(2 ** 31)]], dtype=torch.int32, device=DEV)
    assert (R.shade(dv, df, wild, cam, "normal").cpu().numpy() == 255).all()


def test_refusals():
    from list_amd import hip
    R = _R()
    cam = RC.pixel_camera()
    v, f = (dev(a) for a in RC.small_triangles(50, 64))
    lib = R.load()
    for bad in (lambda: R.rasterize(v.double(), f, cam, 64, 64), lambda: R.rasterize(v, f.long(), cam, 64, 64),
                lambda: R.rasterize(v.half(), f, cam, 64, 64), lambda: R.rasterize(v.cpu(), f, cam, 64, 64),
                lambda: R.rasterize(v, f.t().contiguous().t(), cam, 64, 64),             # [F,3] with strides (1, F)
                lambda: R.rasterize(v[:, :2], f, cam, 64, 64),
                lambda: R.rasterize(v, f, cam, 64, 64, z_near=float("nan"))):
        with pytest.raises(hip.ListError):
            bad()
    # beyond the documented limits: the library's refusal, with its text
    for H, W in ((R.MAX_SIDE + 1, 4), (0, 4), (R.MAX_SIDE, R.MAX_SIDE)):
        with pytest.raises(hip.ListError, match="LIST_RENDER_MAX_SIDE"):
            R.rasterize(v, f, cam, H, W)
        assert b"LIST_RENDER_MAX_PIXELS" in lib.list_render_last_error()
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)
    out = torch.empty((64, 64), dtype=torch.int32, device=DEV)
    c = cam.struct()
    args = [v.data_ptr(), len(v), f.data_ptr(), 2 ** 31, ctypes.byref(c), 64, 64, 1e-6, ws.data_ptr(), ws.numel(),
            out.data_ptr(), out.data_ptr(), out.data_ptr(), 0, R.N_STEPS, None]
    assert lib.list_render_rasterize(*args) == hip.ERR_SHAPE and b"INT32_MAX" in lib.list_render_last_error()
    args[3], args[9] = len(f), 1024                                                  # a workspace too small
    assert lib.list_render_rasterize(*args) == hip.ERR_WORKSPACE
    assert b"list_render_workspace_bytes" in lib.list_render_last_error()
    face_id = R.rasterize(v, f, cam, 64, 64)[0]
    bg = torch.zeros((64, 64, 3), dtype=torch.uint8, device=DEV)
    for bad in (lambda: R.shade(v, f, face_id.long(), cam), lambda: R.shade(v, f, face_id.t(), cam),
                lambda: R.shade(v, f, face_id, cam, background=bg.float()),
                lambda: R.shade(v, f, face_id, cam, background=bg.permute(2, 0, 1).contiguous().permute(1, 2, 0)),
                lambda: R.shade(v, f, face_id, cam, background=bg[:32]), lambda: R.shade(v, f, face_id, cam, "phong"),
                lambda: R.shade(v, f, face_id, cam, alpha=-0.1)):
        with pytest.raises(hip.ListError):
            bad()
