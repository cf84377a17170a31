"""GPU: the .obj text composed on the device (objtext.obj_text, include/list_objtext.h) against objtext.obj_text_cpu, which
test_objtext_cpu.py holds to the file utils.write_obj writes.  Every comparison is byte for byte; nothing is left out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _objtext_cases as OC  # noqa: E402

pytestmark = pytest.mark.gpu

LINES = 256                      # lines per workgroup of k_objtext_emit (kLines)
GUARD = 0xAA
NO_V, NO_F = np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)


def _O():
    import __graft_entry__ as ge
    ge.build()
    from list_amd import objtext
    return objtext


def _dev(v, f):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda()


def _device_text(v, f):
    return _O().obj_text(*_dev(v, f)).cpu().numpy().tobytes()


def _check(v, f):
    want = _O().obj_text_cpu(v, f)
    got = _device_text(v, f)
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"first difference at byte {i}: device {got[max(i - 40, 0):i + 40]!r}, oracle {want[max(i - 40, 0):i + 40]!r}")
    return want


def _emit_at(v, f, offset=0, short=0, band=96):
    """list_objtext_count and list_objtext_emit through the C ABI, the output at `offset` bytes past a 16-byte aligned
    address inside a buffer of GUARD bytes, n_out_bytes `short` below the file's length ->
    (the buffer on the host, where the output starts in it, the file's length)."""
    import torch
    from list_amd import hip
    O = _O()
    lib = O.load()
    tv, tf = _dev(v, f)
    V, F = len(tv), len(tf)
    need = lib.list_objtext_workspace_bytes(V, F)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    totals = torch.zeros((2,), dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr() if t.numel() else None
    O._check(lib.list_objtext_count(p(tv), p(tf), V, F, ws.data_ptr(), need, totals.data_ptr(), hip._stream()), "count")
    n, n_verts = (int(x) for x in totals.tolist())
    assert n_verts == len(O.obj_text_cpu(v, NO_F))
    buf = torch.full((band + 16 + n + band,), GUARD, dtype=torch.uint8, device="cuda")
    start = band + (-(buf.data_ptr() + band)) % 16 + offset
    assert (buf.data_ptr() + start) % 16 == offset
    O._check(lib.list_objtext_emit(p(tv), p(tf), V, F, ws.data_ptr(), need, buf.data_ptr() + start, n - short, hip._stream()),
             "emit")
    torch.cuda.synchronize()
    return buf.cpu().numpy(), start, n


def _mixed_mesh(V, F, seed):
    bits = OC.signed(OC.structured_bits())
    rng = np.random.default_rng(seed)
    v = OC.as_vertices(rng.choice(bits, 3 * V)) if V else NO_V
    f = rng.integers(-20, 3000, (F, 3)).astype(np.int32) if F else NO_F
    return v, f


# ---- values ---------------------------------------------------------------------------------------------------------
def test_structured_and_random_values():
    """The structured list of test_objtext_cpu.py in both signs plus 2^18 random bit patterns, packed as vertices."""
    bits = np.concatenate([OC.signed(OC.structured_bits()), OC.random_bits(1 << 18, seed=30)])
    _check(OC.as_vertices(bits), NO_F)


def test_face_index_borders():
    f = np.concatenate([OC.border_indices(), np.array([[OC.INT32_MAX, OC.INT32_MIN, 0]], dtype=np.int32)])
    want = _check(NO_V, f)
    assert want.endswith(b"f 2147483648 -2147483647 1\n")
    _check(OC.as_vertices(OC.structured_bits()[:30]), f)


# ---- line lengths and the span's staging ------------------------------------------------------------------------------
SHORT_NAN, SHORT_ZERO = [0x7FC00000] * 3, [0] * 3                 # "v nan nan nan", "v 0.0 0.0 0.0": 14 bytes
LONG = [0x80800000, 0xFF7FFFFF, 0x80800000]                       # three 23-byte tokens: a 74-byte line


def _rows(n, *forms):
    return np.array([forms[i % len(forms)] for i in range(n)], dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("n", [257, 513])
@pytest.mark.parametrize("form", ["nan", "zero", "long", "alternating"])
def test_shortest_and_longest_lines(n, form):
    v = {"nan": _rows(n, SHORT_NAN), "zero": _rows(n, SHORT_ZERO), "long": _rows(n, LONG),
         "alternating": _rows(n, SHORT_NAN, LONG, SHORT_ZERO, LONG)}[form]
    want = _check(v, NO_F)
    lens = {len(l) + 1 for l in want.split(b"\n")[:-1]}
    assert lens == {"nan": {14}, "zero": {14}, "long": {_O().MAX_VERTEX_LINE}, "alternating": {14, 74}}[form]


@pytest.mark.parametrize("total", [LINES - 1, LINES, LINES + 1, 2 * LINES - 1, 2 * LINES, 2 * LINES + 1])
def test_line_counts_around_a_workgroup(total):
    """V + F one below, at and one above a multiple of the workgroup's line count; the vertex / face border inside a
    workgroup and on its edge."""
    for V in (total // 3, min(LINES, total), total - 1):
        _check(*_mixed_mesh(V, total - V, seed=total + V))


@pytest.mark.parametrize("V,F", [(700, 0), (0, 700), (1, 0), (0, 1), (1, 1), (0, 0)])
def test_vertex_only_face_only_single_line_and_empty(V, F):
    want = _check(*_mixed_mesh(V, F, seed=7))
    assert (len(want) == 0) == (V + F == 0)
    if V + F == 0:
        assert _O().obj_text(_dev(NO_V, NO_F)[0]).numel() == 0


# ---- where the output lies --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", range(16))
def test_every_alignment_between_guard_bands(offset):
    v, f = _mixed_mesh(300, 301, seed=40)
    want = _O().obj_text_cpu(v, f)
    buf, start, n = _emit_at(v, f, offset=offset)
    assert n == len(want) and buf[start:start + n].tobytes() == want
    assert (buf[:start] == GUARD).all() and (buf[start + n:] == GUARD).all()


@pytest.mark.parametrize("short", ["one", "half", "all but one"])
def test_short_output_writes_the_prefix_and_nothing_past_it(short):
    v, f = _mixed_mesh(400, 333, seed=41)
    want = _O().obj_text_cpu(v, f)
    cut = {"one": 1, "half": len(want) // 2, "all but one": len(want) - 1}[short]
    buf, start, n = _emit_at(v, f, offset=5, short=cut)
    keep = n - cut
    assert n == len(want) and buf[start:start + keep].tobytes() == want[:keep]
    assert (buf[:start] == GUARD).all() and (buf[start + keep:] == GUARD).all()


# ---- the interface ------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from list_amd import hip
    O = _O()
    v, f = _dev(*_mixed_mesh(5, 4, seed=1))
    with pytest.raises(RuntimeError):
        O.obj_text(v.double(), f)
    with pytest.raises(RuntimeError):
        O.obj_text(v, f.long())
    with pytest.raises(RuntimeError):
        O.obj_text(v.cpu(), f)
    with pytest.raises(RuntimeError):
        O.obj_text(torch.zeros((3, 5), device="cuda").t(), f)          # [5,3] but not contiguous
    with pytest.raises(hip.ListError):
        O.obj_text(v.reshape(-1), f)
    lib = O.load()
    assert lib.list_objtext_count(v.data_ptr(), f.data_ptr(), 5, 4, v.data_ptr(), 8, v.data_ptr(), None) == hip.ERR_WORKSPACE
    assert b"list_objtext_workspace_bytes" in lib.list_objtext_last_error()


def test_end_to_end_export(tmp_path):
    """marching_cubes -> keep_components -> simplify on the device, Mesh.export through the device path: the file
    utils.write_obj writes of the host arrays, and evaluate.load_mesh reads the same float32 vertices and faces back."""
    import torch
    from list_amd import components, evaluate, mesh, simplify
    O = _O()
    ax = np.linspace(-0.5, 0.5, 32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.from_numpy((0.3 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)).cuda()
    v, f = mesh.marching_cubes(vol)
    v, f, _ = components.keep_components(v, f, keep=1)
    v, f, _ = simplify.simplify(v, f, 16)
    m = mesh.Mesh(v, f)
    assert m._device is not None and len(m.faces) > 500
    path = m.export(str(tmp_path / "device.obj"))
    data = open(path, "rb").read()
    assert data == OC.loop_file(tmp_path, m.vertices, m.faces) == O.obj_text_cpu(m.vertices, m.faces)
    assert O.write_obj(str(tmp_path / "again.obj"), v, f) == len(data)
    back = evaluate.load_mesh(path)
    assert back.vertices.tobytes() == m.vertices.tobytes() and np.array_equal(back.faces, m.faces)
    cloud = str(tmp_path / "cloud.obj")
    assert O.write_obj(cloud, v) == len(O.obj_text_cpu(m.vertices)) and open(cloud, "rb").read() == O.obj_text_cpu(m.vertices)
