"""CPU: the .obj text rule of objtext.py / csrc/objtext_math.h, token by token against the f-string of utils.write_obj and
file by file against the file utils.write_obj writes; the header compiled for the host under the sanitizers; the table
generator; the C ABI of include/list_objtext.h.  Every comparison is of bytes.

What the f-string prints.  utils.write_obj writes f"{v[0]}" of a numpy.float32.  format(numpy.float32, "") does not go
through str(numpy.float32): numpy hands the value to Python's float, so the token is repr(float(x)) -- the shortest digits
of the value widened to float64, 0.10000000149011612 for 0.1f, not float32's own shortest digits 0.1.  The file is the
oracle, so the rule here is the float64 one (Ryu's double tables cut to float32's exponents); test_tokens_are_not_
str_float32 pins the difference, so that a change of numpy's formatting shows up here and not as a silent change of files."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_headers as H  # noqa: E402
import _objtext_cases as OC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _O():
    from list_amd import objtext
    return objtext


def _tokens(bits):
    return [t.decode("ascii") for t in _O().format_f32_cpu(bits)]


# ---- tokens ---------------------------------------------------------------------------------------------------------
def test_structured_tokens_equal_the_f_string():
    """Every power of two 2^-149 .. 2^127 with +-2 ulps, the float nearest every 10^k with +-1 ulp, the neighbours of
    1e-4, 1e16 and 2^24, zeros, infinities, NaNs of both signs and several payloads, the subnormal extremes, FLT_MAX and
    the interval-end class, in both signs."""
    bits = OC.signed(OC.structured_bits())
    got, want = _tokens(bits), OC.oracle_tokens(bits)
    bad = [(hex(b), g, w) for b, g, w in zip(bits, got, want) if g != w]
    assert not bad, bad[:10]
    assert max(len(t) for t in got) == _O().MAX_TOKEN == 23            # -1.1754943508222875e-38
    for b, text in ((0x7FC00000, "nan"), (0xFFC00001, "nan"), (0xFF800000, "-inf"), (0x80000000, "-0.0"), (1, "1.401298464324817e-45"),
                    (0x3DCCCCCD, "0.10000000149011612"), (0x4B800000, "16777216.0"), (0x4C01AE8C, "33995312.0"),
                    (0x5A0E1BCA, "1.0000000272564224e+16"), (0x5A0E1BC9, "9999999198822400.0"),
                    (0x38D1B717, "9.999999747378752e-05"), (0x38D1B718, "0.00010000000474974513"), (0x3F000000, "0.5")):
        assert _tokens([b]) == [text]


def test_interval_end_class_needs_included_ends():
    """The members of the class really have their text ON an end of the float64's rounding interval (exact, Fractions):
    a rule with excluded ends prints them a digit longer."""
    cls = OC.interval_end_class()
    assert len(cls) >= 88
    assert all(OC.on_interval_end(b) for b in cls[:: max(len(cls) // 300, 1)])
    assert _tokens(cls) == OC.oracle_tokens(cls)


def test_random_tokens_equal_the_f_string():
    bits = OC.random_bits(1 << 20, seed=20)
    got, want = _O().format_f32_cpu(bits), np.array(OC.oracle_tokens(bits)).astype("S23")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(bits[i]), got[i], want[i]) for i in bad[:10]]


def test_sphere_vertex_tokens_equal_the_f_string():
    v, _ = OC.sphere_mesh()
    bits = v.view(np.uint32).reshape(-1)
    assert len(bits) > 3000 and _tokens(bits) == OC.oracle_tokens(bits)


def test_tokens_are_not_str_float32():
    """The f-string and str() of a numpy.float32 differ (module docstring): the file holds the former."""
    x = np.float32(0.1)
    assert f"{x}" == repr(float(x)) == "0.10000000149011612" and str(x) == "0.1"
    assert _tokens([OC.f32_bits(0.1)]) == [f"{x}"]


# ---- files ----------------------------------------------------------------------------------------------------------
def _mesh_cases():
    sv, sf = OC.sphere_mesh()
    one = np.array([[0.25, -1.5, 3.0]], dtype=np.float32)
    none_v, none_f = np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)
    return {"sphere": (sv, sf), "V=0": (none_v, OC.border_indices()), "F=0": (sv[:77], none_f), "empty": (none_v, none_f),
            "one vertex": (one, none_f), "borders": (OC.as_vertices(OC.signed(OC.structured_bits())[:999]), OC.border_indices())}


@pytest.mark.parametrize("name", ["sphere", "V=0", "F=0", "empty", "one vertex", "borders"])
def test_file_equals_the_python_loop(tmp_path, name):
    v, f = _mesh_cases()[name]
    O = _O()
    text = O.obj_text_cpu(v, f)
    assert text == OC.loop_file(tmp_path, v, f)
    assert text == O.obj_text_cpu(v, f if len(f) else None)
    if name == "borders":
        lines = text.decode("ascii").splitlines()
        tokens = {t for l in lines if l[0] == "f" for t in l.split()[1:]}
        assert {str(10 ** k + d) for k in range(1, 10) for d in (-1, 0, 1)} <= tokens
        assert {"0", "1", "-1", "-2", "-9", "-10", "-11", "-2147483647", "2147483647"} <= tokens
        assert max(len(l) for l in lines if l[0] == "f") + 1 <= O.MAX_FACE_LINE


def test_int32_max_prints_in_int64():
    """The one index the loop cannot print (its int32 sum overflows): the rule states 2147483648."""
    f = np.array([[OC.INT32_MAX, OC.INT32_MIN, 0]], dtype=np.int32)
    assert _O().obj_text_cpu(np.zeros((0, 3), dtype=np.float32), f) == b"f 2147483648 -2147483647 1\n"
    assert len(b"f -2147483647 -2147483647 -2147483647\n") == _O().MAX_FACE_LINE


def test_refusals():
    O = _O()
    with pytest.raises(ValueError):
        O.obj_text_cpu(np.zeros((2, 3), dtype=np.float64))
    with pytest.raises(ValueError):
        O.obj_text_cpu(np.zeros((2, 2), dtype=np.float32))
    with pytest.raises(ValueError):
        O.obj_text_cpu(np.zeros((2, 3), dtype=np.float32), np.zeros((1, 3), dtype=np.int64))


def test_host_mesh_export_is_untouched(tmp_path):
    from list_amd import mesh
    v, f = OC.sphere_mesh(16)
    path = mesh.Mesh(v, f).export(str(tmp_path / "m.obj"))
    assert open(path, "rb").read() == OC.loop_file(tmp_path, v, f) == _O().obj_text_cpu(v, f)


# ---- the shared header on the host ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return OC.build_host(tmp_path_factory.mktemp("objtext_host"))


def test_header_on_the_host_equals_the_numpy_rule(host_exe, tmp_path):
    """csrc/objtext_math.h -- the code the kernels run -- as a stand-alone program under AddressSanitizer and
    UndefinedBehaviorSanitizer, its output buffer exactly `cap` bytes: the whole file, one byte short, far short, nothing."""
    O = _O()
    bits = np.concatenate([OC.signed(OC.structured_bits()), OC.random_bits(1 << 16, seed=21)])
    sv, sf = OC.sphere_mesh(16)
    v = np.concatenate([OC.as_vertices(bits), sv])
    f = np.concatenate([OC.border_indices(), sf, np.array([[OC.INT32_MAX, 0, -1]], dtype=np.int32)])
    want = O.obj_text_cpu(v, f)
    for cap in (len(want), len(want) - 1, 97, 0):
        total, got = OC.run_host(host_exe, tmp_path, v, f, cap)
        assert total == len(want) and got == want[:cap]
    assert OC.run_host(host_exe, tmp_path, v[:0], f[:0], 16) == (0, b"")


def test_library_host_entry_equals_the_numpy_rule():
    import __graft_entry__ as ge
    ge.build()
    O = _O()
    v, f = OC.as_vertices(OC.signed(OC.structured_bits())[:3000]), OC.border_indices()
    want = O.obj_text_cpu(v, f)
    assert O.obj_text_host(v, f) == want and O.obj_text_host(v[:0], None) == b""
    lib = O.load()
    short = np.full(64, 0xAA, dtype=np.uint8)
    assert lib.list_objtext_host(v.ctypes.data, f.ctypes.data, len(v), len(f), short.ctypes.data, 40) == len(want)
    assert short[:40].tobytes() == want[:40] and (short[40:] == 0xAA).all()
    assert lib.list_objtext_host(None, None, 3, 0, None, 0) < 0 and b"NULL" in lib.list_objtext_last_error()
    assert lib.list_objtext_workspace_bytes(-1, 0) == 0 and b"V = -1" in lib.list_objtext_last_error()
    assert lib.list_objtext_workspace_bytes(2 ** 31 - 2, 1) == 0


# ---- tables and bindings ----------------------------------------------------------------------------------------------
def test_generator_reproduces_the_committed_tables():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_objtext_tables.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    inv, pw = _O().tables()
    word = lambda t, i: int(t[i, 0]) | (int(t[i, 1]) << 64)
    assert word(inv, 0) == 2 ** 125 + 1 and word(pw, 0) == 2 ** 124
    assert all(word(pw, i) == 5 ** i << (125 - (5 ** i).bit_length()) for i in range(1, 54))
    assert all(word(inv, q) == 2 ** ((5 ** q).bit_length() - 1 + 125) // 5 ** q + 1 for q in range(1, len(inv)))


def test_header_table_and_library_agree():
    """What include/list_objtext.h declares == OBJTEXT_EXPORTS == what the library exports under list_objtext_."""
    import __graft_entry__ as ge
    ge.build()
    from list_amd import hip
    O = _O()
    names, exported = H.declared("list_objtext.h"), H.exported(hip.LIB_PATH)
    assert names == sorted(O.OBJTEXT_EXPORTS)
    raw, lib = ctypes.CDLL(hip.LIB_PATH), O.load()
    for name in names:
        assert hasattr(raw, name), f"{name} declared in list_objtext.h but not exported"
        assert getattr(lib, name) is not None
    assert {n for n in exported if n.startswith("list_objtext_")} == set(names)
    assert not set(names) & set(hip.EXPORTS) and not any(n.startswith("list_objtext_") for n in hip.EXPORTS)
    assert hip.ABI_VERSION == 9 and lib.list_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "list_objtext.h")).read()
    for name, value in (("MAX_TOKEN", O.MAX_TOKEN), ("MAX_VERTEX_LINE", O.MAX_VERTEX_LINE), ("MAX_FACE_LINE", O.MAX_FACE_LINE)):
        assert f"#define LIST_OBJTEXT_{name} {value}\n" in text
