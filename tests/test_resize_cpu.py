"""CPU: the resize (list_amd.resize) against Pillow, which is the judge: the numpy restatement resize_cpu and the library's
host compilation list_resize_host against Image.resize(..., BILINEAR) byte for byte, the plan against coeffs_cpu, the
stand-alone program under the sanitizers, apply_cpu against Pillow's whole pipeline, and the C ABI of
include/list_resize.h without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from list_amd import augment as A, hip, resize as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H  # noqa: E402
import _resize_case as RC  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return R.load()


def pil(image, out_h, out_w):
    return np.asarray(Image.fromarray(image).resize((out_w, out_h), Image.Resampling.BILINEAR))


def both_equal_pillow(image, out_h, out_w):
    want = pil(image, out_h, out_w)
    got, hst = R.resize_cpu(image, out_h, out_w), R.host(image, out_h, out_w)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), ("resize_cpu", image.shape, out_h, out_w)
    assert np.array_equal(hst, want), ("list_resize_host", image.shape, out_h, out_w)


# ---- the restatements against Pillow, no tolerance -------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", RC.PATTERNS)
def test_every_axis_pair_up_to_40_equals_pillow(lib, pattern):
    """n_in, n_out in 1 ... 40, as an n x 1 and as a 1 x n image: the vertical and the horizontal pass on their own."""
    for n_in in range(1, 41):
        column, row = RC.pixels(pattern, n_in, 1, 1), RC.pixels(pattern, 1, n_in, 2)
        for n_out in range(1, 41):
            both_equal_pillow(column, n_out, 1)
            both_equal_pillow(row, 1, n_out)


SHAPES = [(5, 7, 12, 16), (13, 13, 24, 24), (13, 17, 40, 31),                   # up-scaling
          (37, 53, 16, 12), (333, 500, 224, 224), (100, 77, 33, 50), (50, 31, 7, 9),      # non-integer reductions
          (64, 48, 16, 12), (90, 6, 30, 12),                                     # integer reduction; one axis up, one down
          (17, 3000, 8, 8), (2500, 30, 4, 24), (1, 1, 16, 12),                   # a reduction above 100 x
          (24, 24, 24, 24), (1, 1, 1, 1), (16, 12, 16, 12),                      # equal sizes
          (16, 29, 16, 12), (31, 12, 16, 12), (224, 50, 224, 224)]               # one axis equal


@pytest.mark.parametrize("pattern", RC.PATTERNS)
def test_2d_shapes_equal_pillow(lib, pattern):
    for h, w, out_h, out_w in SHAPES:
        both_equal_pillow(RC.pixels(pattern, h, w, 3), out_h, out_w)


@pytest.mark.parametrize("pattern", RC.PATTERNS)
def test_the_tall_rule_on_both_sides_of_its_borders(lib, pattern):
    """H = 100 W against 100 W + 1 (the order changes there), and out_h = H - 1 against out_h = H; 3000 x 17 -> 8 x 8 is the
    case that equals Pillow only with the vertical pass first."""
    for W in (1, 2, 3):
        for h in (100 * W, 100 * W + 1):
            assert R.stages_cpu(h, W, 8, 12)[0] == ((R.VERTICAL, R.HORIZONTAL) if h > 100 * W else (R.HORIZONTAL, R.VERTICAL))
            both_equal_pillow(RC.pixels(pattern, h, W, 4), 8, 12)
            both_equal_pillow(RC.pixels(pattern, h, W, 4), h - 1, 12)
            both_equal_pillow(RC.pixels(pattern, h, W, 4), h, 12)
            both_equal_pillow(RC.pixels(pattern, h, W, 4), h + 7, 12)
    assert R.stages_cpu(301, 3, 300, 12)[0] == (R.VERTICAL, R.HORIZONTAL)
    assert R.stages_cpu(301, 3, 301, 12)[0] == (R.HORIZONTAL, R.COPY) and R.stages_cpu(301, 3, 302, 12)[0] == (R.HORIZONTAL, R.VERTICAL)
    both_equal_pillow(RC.pixels(pattern, 3000, 17, 4), 8, 8)


def test_the_order_matters_where_the_rule_applies():
    image = RC.pixels("random", 3000, 17, 4)
    other = R._pass_cpu(R._pass_cpu(image, 8, 1), 8, 0)              # horizontal first: not Pillow's bytes
    assert not np.array_equal(other, pil(image, 8, 8))


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_the_plan_holds_coeffs_cpu(lib):
    out_h, out_w = 16, 12
    images, _ = RC.branch_batch(A, out_h, out_w)
    ragged = R.RaggedImages.pack(images)
    buf = R.plan(ragged, out_h, out_w)
    head, records, tables = R.parse_plan(buf)
    rec = ragged.records()
    assert int(head["plan_bytes"]) == buf.size == lib.list_resize_plan_bytes(rec.ctypes.data, 9, out_h, out_w)
    assert int(head["workspace_bytes"]) == lib.list_resize_workspace_bytes(rec.ctypes.data, 9, out_h, out_w)
    assert (int(head["B"]), int(head["out_h"]), int(head["out_w"]), int(head["src_bytes"])) == (9, out_h, out_w, ragged.data.numel())
    mid, used = 0, R.PLAN_HEADER.itemsize + 9 * R.PLAN_IMAGE.itemsize
    for i, (h, w) in enumerate(ragged.sizes.tolist()):
        stages, (mid_h, mid_w) = R.stages_cpu(h, w, out_h, out_w)
        r = records[i]
        assert (int(r["src_offset"]), int(r["H"]), int(r["W"])) == (int(ragged.offsets[i]), h, w)
        assert tuple(r["stage"]) == stages and (int(r["mid_h"]), int(r["mid_w"]), int(r["mid_offset"])) == (mid_h, mid_w, mid)
        mid += 3 * mid_h * mid_w
        for s, stage in enumerate(stages):
            if stage == R.COPY:
                assert tables(i, s) is None and int(r["ksize"][s]) == 0
                continue
            n_in, n_out = (w, out_w) if stage == R.HORIZONTAL else (h, out_h)
            bounds, K = R.coeffs_cpu(n_in, n_out)
            got_bounds, got_K = tables(i, s)
            assert int(r["ksize"][s]) == K.shape[1] and int(r["bounds"][s]) == used
            assert np.array_equal(got_bounds, bounds) and np.array_equal(got_K, K)
            assert (K.sum(1) > (1 << 22) - K.shape[1]).all() and (K.sum(1) < (1 << 22) + K.shape[1]).all() and (K >= 0).all()
            used += 4 * n_out * (2 + K.shape[1])
    assert used == buf.size and mid == int(head["workspace_bytes"])
    for n_in, n_out in ((700, 8), (13, 24), (1, 1), (4000, 224), (16384, 1)):
        bounds, K = R.coeffs_cpu(n_in, n_out)
        assert K.shape[1] == 2 * max(-(-n_in // n_out), 1) + 1 and (bounds[:, 0] + bounds[:, 1] <= n_in).all()


# ---- the stand-alone program under the sanitizers -------------------------------------------------------------------------
def test_host_program_is_clean_under_asan_and_ubsan(lib, tmp_path):
    exe = RC.build_host(tmp_path)
    for h, w, out_h, out_w in ((700, 3, 8, 8), (37, 53, 16, 12), (1, 1, 1, 1), (5, 7, 12, 16), (303, 3, 320, 8), (24, 24, 24, 24)):
        image = RC.pixels("random", h, w, 9)
        got, plan = RC.run_host(exe, image, out_h, out_w, tmp_path)
        assert np.array_equal(got, pil(image, out_h, out_w))
        assert np.array_equal(plan, R.plan(R.RaggedImages.pack([image]), out_h, out_w))


# ---- apply_cpu against Pillow's pipeline ----------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_apply_cpu_is_flip_jitter_resize_totensor_in_that_order():
    images, params = RC.branch_batch(A, 16, 12)
    ragged = R.RaggedImages.pack(images)
    assert len(ragged) == 9 and ragged.sizes.shape == (9, 2) and ragged.sizes.dtype == torch.int64
    got = R.apply_cpu(ragged, 16, 12, params)
    assert got.shape == (9, 3, 16, 12) and got.dtype == np.float32
    for i, image in enumerate(images):
        want = A.to_tensor(R.resize_pil(A.jitter_pil(image, params[i:i + 1]), (12, 16))).numpy()
        assert np.array_equal(bits(got[i]), bits(want)), i
    # the order is part of the definition: resizing first and jittering after gives other bytes
    late = A.to_tensor(A.jitter_pil(R.resize_pil(images[5], (12, 16)), params[5:6])).numpy()
    assert not np.array_equal(bits(got[5]), bits(late))
    plain = R.apply_cpu(ragged, 16, 12)
    assert np.array_equal(bits(plain[3]), bits((images[3].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)))      # the copy
    for cl in (False, True):
        t = R.apply(ragged, 16, 12, params, channels_last=cl)             # CPU tensors take apply_cpu
        assert t.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        assert np.array_equal(bits(t.numpy()), bits(got))
    with pytest.raises(ValueError, match="record"):
        R.apply_cpu(ragged, 16, 12, params[:2])
    with pytest.raises(ValueError):
        R.apply_cpu(ragged, 0, 12)
    with pytest.raises(ValueError):
        R.apply(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), 4, 4)


def test_ragged_images_pack_and_move():
    images = [RC.pixels("random", 3, 5), RC.pixels("checker", 1, 1), RC.pixels("random", 4, 2)]
    ragged = R.RaggedImages.pack([images[0], torch.from_numpy(images[1]), images[2]])
    assert len(ragged) == 3 and ragged.data.dtype == torch.uint8 and ragged.data.numel() == 45 + 3 + 24
    assert ragged.sizes.tolist() == [[3, 5], [1, 1], [4, 2]] and ragged.offsets.tolist() == [0, 45, 48]
    for i, image in enumerate(images):
        assert np.array_equal(ragged.image(i).numpy(), image)
    moved = ragged.to("cpu")
    assert isinstance(moved, R.RaggedImages) and torch.equal(moved.data, ragged.data) and moved.device.type == "cpu"
    for bad in ([], [images[0].astype(np.float32)], [images[0][..., :2]], [images[0][0]]):
        with pytest.raises(ValueError):
            R.RaggedImages.pack(bad)
    with pytest.raises(ValueError, match="offsets"):
        R.RaggedImages(ragged.data, ragged.sizes, [0, 45, 49])


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree(lib):
    names = H.declared("list_resize.h")
    assert names == sorted(R.RESIZE_EXPORTS) == ["list_resize_fwd", "list_resize_host", "list_resize_last_error",
                                                 "list_resize_plan", "list_resize_plan_bytes", "list_resize_workspace_bytes"]
    exported = H.exported(hip.LIB_PATH)
    assert {n for n in exported if n.startswith("list_resize_")} == set(names)
    assert not set(names) & set(hip.EXPORTS)
    for header, (_, _, prefixes) in H.SECTIONS.items():                 # no other section owns the prefix
        assert not prefixes or not any(n.startswith(prefixes) for n in names), header
    for n in names:
        assert getattr(lib, n) is not None
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9
    build = __import__("list_amd.build", fromlist=["x"])
    assert "list_resize.h" in build.PUBLIC_HEADERS and "resize_kernels.hip" in build.SOURCES
    assert "resize_math.h" in build.HEADERS and "augment_check.h" in build.HEADERS
    text = open(os.path.join(H.ROOT, "include", "list_resize.h")).read()                  # the records the binding mirrors
    assert "int64_t offset;" in text and "LIST_RESIZE_MAX_SIDE 16384" in text
    assert [R.IMAGE.fields[k][1] for k in ("offset", "H", "W")] == [0, 8, 12]
    assert [R.PLAN_HEADER.fields[k][1] for k in ("plan_bytes", "workspace_bytes", "src_bytes", "magic", "B", "out_h", "out_w")] \
        == [0, 8, 16, 24, 28, 32, 36]
    assert [R.PLAN_IMAGE.fields[k][1] for k in ("src_offset", "mid_offset", "H", "W", "mid_h", "mid_w", "stage", "ksize", "bounds",
                                                "weights")] == [0, 8, 16, 20, 24, 28, 32, 40, 48, 64]
    # the one copy of the parameter checks: both units refuse a record in the same words
    bad = A.make_params(16)
    assert A.load().list_augment_pixel(np.zeros(3, np.uint8).ctypes.data, bad.ctypes.data, None, None) == hip.ERR_ARG
    assert b"params[0].ops = 16" in lib.list_augment_last_error()


def test_refusals_come_before_any_hip_call(lib):
    fake = 4096                                   # never dereferenced: every refusal below is a host check
    err = lambda: lib.list_resize_last_error().decode()
    images = [RC.pixels("random", 5, 7), RC.pixels("random", 16, 12), RC.pixels("random", 40, 3)]
    ragged = R.RaggedImages.pack(images)
    rec, n = ragged.records(), ragged.data.numel()
    buf = R.plan(ragged, 16, 12)
    ws_need = lib.list_resize_workspace_bytes(rec.ctypes.data, 3, 16, 12)
    good = A.draw_params(3, True, True, torch.Generator().manual_seed(0))

    # sizing and planning
    for fn in (lib.list_resize_plan_bytes, lib.list_resize_workspace_bytes):
        assert fn(None, 3, 16, 12) == 0 and "images is NULL" in err()
        for B, oh, ow in ((0, 16, 12), (-1, 16, 12), (65536, 16, 12), (3, 0, 12), (3, 16, 0), (3, 16385, 12), (3, 16, 16385)):
            assert fn(rec.ctypes.data, B, oh, ow) == 0 and "need 1 <= B" in err()
        for field, v in (("H", 0), ("W", 0), ("H", 16385), ("W", -3)):
            r = rec.copy()
            r[field][1] = v
            assert fn(r.ctypes.data, 3, 16, 12) == 0 and "images[1]" in err()
    out = R._aligned_bytes(buf.size)

    def make(r=rec, B=3, src_bytes=n, plan=out.ctypes.data, plan_bytes=buf.size):
        return lib.list_resize_plan(r.ctypes.data if r is not None else None, B, src_bytes, 16, 12, plan, plan_bytes)

    assert make() == 0 and np.array_equal(out, buf)
    assert make(plan=None) == hip.ERR_ARG and "plan is NULL" in err()
    assert make(r=None) == hip.ERR_ARG and "images is NULL" in err()
    assert make(B=0) == hip.ERR_SHAPE
    assert make(plan=out.ctypes.data + 4) == hip.ERR_ARG and "aligned" in err()
    assert make(plan_bytes=buf.size - 1) == hip.ERR_WORKSPACE and "list_resize_plan_bytes" in err()
    assert make(src_bytes=n - 1) == hip.ERR_ARG and "images[2]" in err() and "outside src_bytes" in err()
    for offset in (-1, n, int(rec["offset"][1]) + 1 + int(rec["offset"][2])):
        r = rec.copy()
        r["offset"][2 if offset != -1 else 0] = offset
        assert make(r=r) == hip.ERR_ARG and "outside src_bytes" in err(), offset

    # the launch call
    def fwd(plan=buf, plan_bytes=None, src_bytes=n, cl=0, p=good, ws_bytes=ws_need, **ptr):
        a = dict(src=fake, plan_host=plan.ctypes.data, plan_device=fake, dst=fake, workspace=fake,
                 params_host=None if p is None else p.ctypes.data, params_device=None if p is None else fake)
        a.update(ptr)
        return lib.list_resize_fwd(a["src"], src_bytes, a["plan_host"], a["plan_device"], plan.size if plan_bytes is None else plan_bytes,
                                   a["params_host"], a["params_device"], a["dst"], cl, a["workspace"], ws_bytes, None)

    for name in ("src", "plan_host", "plan_device", "dst", "workspace", "params_host", "params_device"):
        assert fwd(**{name: None}) == hip.ERR_ARG and f"{name} is NULL" in err()
    assert fwd(plan_device=fake + 4) == hip.ERR_ARG and "aligned" in err()
    assert fwd(dst=fake + 2) == hip.ERR_ARG and "aligned" in err()
    for cl in (2, -1):
        assert fwd(cl=cl) == hip.ERR_SHAPE and f"channels_last = {cl}" in err()
    assert fwd(plan_bytes=buf.size - 1) == hip.ERR_WORKSPACE and "list_resize_plan_bytes" in err()
    assert fwd(plan_bytes=8) == hip.ERR_WORKSPACE
    assert fwd(ws_bytes=ws_need - 1) == hip.ERR_WORKSPACE and "list_resize_workspace_bytes" in err()
    assert fwd(src_bytes=n - 1) == hip.ERR_ARG and "src_bytes" in err()

    def spoiled(change):
        b = buf.copy()
        head, records, tables = R.parse_plan(b)
        change(b, b[:R.PLAN_HEADER.itemsize].view(R.PLAN_HEADER), records, tables)
        return fwd(plan=b)

    assert spoiled(lambda b, h, r, t: h["magic"].__setitem__(0, 7)) == hip.ERR_ARG and "not a plan" in err()
    assert spoiled(lambda b, h, r, t: h["B"].__setitem__(0, 0)) == hip.ERR_ARG and "not a plan" in err()
    assert spoiled(lambda b, h, r, t: h["out_h"].__setitem__(0, 16385)) == hip.ERR_ARG
    assert spoiled(lambda b, h, r, t: r["H"].__setitem__(0, 0)) == hip.ERR_SHAPE and "plan image 0" in err()
    assert spoiled(lambda b, h, r, t: r["src_offset"].__setitem__(2, n)) == hip.ERR_ARG and "outside src_bytes" in err()
    for field, v in (("mid_offset", 1), ("mid_h", 6), ("W", 40), ("stage", (2, 1)), ("ksize", (3, 9)), ("bounds", (0, 0)),
                     ("weights", (8, 8))):
        assert spoiled(lambda b, h, r, t: r[field].__setitem__(0, v)) == hip.ERR_ARG and "plan image 0" in err(), field
    assert spoiled(lambda b, h, r, t: t(0, 0)[0].__setitem__((3, 0), 7)) == hip.ERR_ARG and "plan image 0" in err()      # xmin + xmax > W
    assert spoiled(lambda b, h, r, t: t(2, 1)[0].__setitem__((1, 1), -1)) == hip.ERR_ARG and "plan image 2" in err()

    # list_augment_fwd's parameter checks, in its words
    def bad(field, value, ops=A.JITTER):
        p = good.copy()
        p["ops"][1] = ops
        p[field][1] = value
        return fwd(p=p)

    assert bad("ops", 16, 16) == hip.ERR_ARG and "params[1].ops = 16" in err()
    assert bad("order", (0, 1, 2, 2)) == hip.ERR_ARG and "not a permutation" in err()
    for field, v in (("brightness", 1.31), ("saturation", np.nan), ("hue_shift", 256)):
        assert bad(field, v) == hip.ERR_ARG and f"params[1].{field}" in err()

    # list_resize_host
    a, o = images[0], np.empty((16, 12, 3), np.uint8)
    assert lib.list_resize_host(None, 5, 7, o.ctypes.data, 16, 12) == hip.ERR_ARG and "src is NULL" in err()
    assert lib.list_resize_host(a.ctypes.data, 5, 7, None, 16, 12) == hip.ERR_ARG and "dst is NULL" in err()
    for dims in ((0, 7, 16, 12), (5, 16385, 16, 12), (5, 7, 0, 12), (5, 7, 16, 16385)):
        assert lib.list_resize_host(a.ctypes.data, dims[0], dims[1], o.ctypes.data, dims[2], dims[3]) == hip.ERR_SHAPE


def test_a_refused_call_leaves_the_other_sections_text_alone(lib):
    assert A.load().list_augment_pixel(None, None, None, None) == hip.ERR_ARG
    before = lib.list_augment_last_error()
    assert lib.list_resize_host(None, 1, 1, None, 1, 1) == hip.ERR_ARG and b"src is NULL" in lib.list_resize_last_error()
    assert lib.list_augment_last_error() == before and b"rgb_in" in before
