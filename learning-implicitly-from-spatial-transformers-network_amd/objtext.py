"""The text of a Wavefront .obj file, composed on the device: the bytes utils.write_obj writes, without its Python loop.

`obj_text` runs on the tensors' device through liblist_hip.so (include/list_objtext.h) and `write_obj` puts its bytes into
a file; `obj_text_cpu` is the same rule in numpy -- the test oracle, itself held to utils.write_obj.  All give, exactly:

  * all vertex lines, then all face lines: "v " s(x) " " s(y) " " s(z) "\\n" and "f " d(a+1) " " d(b+1) " " d(c+1) "\\n";
  * d: the decimal of the int32 index plus one computed in int64, '-' in front when negative; no index is validated.
    (utils.write_obj adds the one in int32, which overflows for INT32_MAX alone; here that index prints 2147483648);
  * s: what the f-string makes of a numpy.float32 -- format(x, "") hands the value to Python's float, so the text is
    repr(float(x)), the shortest digits of the value WIDENED to float64 (0.1f prints 0.10000000149011612) -- from the bit
    pattern alone in integer arithmetic: "nan" for a NaN of either sign and any payload, "inf", "-inf", "0.0", "-0.0";
    else the shortest digits d1..dn (1 <= n <= 17) and exponent inside the float64's rounding interval -- it ends at the
    midpoints to the neighbouring float64s (the lower half is half as wide when x is a power of two), ends included, as
    the widened significand is always even -- and among the shortest the closest to the value (Ryu's float64 rule; its
    two multiplier tables, cut to the exponents a float32 reaches, are csrc/objtext_tables.h, written by
    tools/gen_objtext_tables.py);
  * layout, on the digits: with x = d1.d2..dn * 10^e, -4 <= e < 16 is positional with at least one digit on each side of
    the point, zeros up to the point and then ".0"; else d1[.d2..dn]e+XX / e-XX with two exponent digits;
  * a token is at most 23 bytes, a vertex line at most 74, a face line at most 38.

The numpy restatement shares no code with numpy's own float formatting: it works on uint32 bit patterns with integer
operations (128-bit products from 32-bit halves of uint64 words, as csrc/objtext_math.h takes them)."""
import ctypes as C
import os
import re

import numpy as np

from . import hip

_TABLES_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "objtext_tables.h")
INT32_MAX = 2 ** 31 - 1
MAX_TOKEN, MAX_VERTEX_LINE, MAX_FACE_LINE = 23, 74, 38      # LIST_OBJTEXT_MAX_*
MAX_INDEX_TOKEN = 11                                        # -2147483647
MAX_DIGITS = 17
POW5_BITS = 125

OBJTEXT_EXPORTS = {
    "list_objtext_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "list_objtext_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p]),
    "list_objtext_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_int64, C.c_void_p]),
    "list_objtext_host": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]),
    "list_objtext_last_error": (C.c_char_p, []),
}

_section = hip.Section(OBJTEXT_EXPORTS, "list_objtext_last_error")    # include/list_objtext.h on hip.load()'s handle
load, _check = _section.load, _section.check


# ---- device ---------------------------------------------------------------------------------------------------------
def _dev_inputs(verts, faces):
    import torch
    hip._f32_cuda(verts, "verts")
    if faces is None:
        faces = torch.empty((0, 3), dtype=torch.int32, device=verts.device)
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or not faces.is_cuda:
        raise RuntimeError(f"faces must be an int32 CUDA/HIP tensor (got {type(faces).__name__} "
                           f"{getattr(faces, 'dtype', None)} {getattr(faces, 'device', None)})")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise hip.ListError("obj_text", hip.ERR_SHAPE, f"verts of shape {tuple(verts.shape)}: need [V,3]")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise hip.ListError("obj_text", hip.ERR_SHAPE, f"faces of shape {tuple(faces.shape)}: need [F,3]")
    if faces.device != verts.device:
        raise RuntimeError(f"verts on {verts.device}, faces on {faces.device}")
    if not (verts.is_contiguous() and faces.is_contiguous()):
        raise RuntimeError("verts and faces must be contiguous")
    if len(verts) + len(faces) >= INT32_MAX:
        raise hip.ListError("obj_text", hip.ERR_SHAPE, f"V = {len(verts)}, F = {len(faces)}: V + F must be below INT32_MAX")
    return verts, faces


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def obj_text(verts, faces=None):
    """The .obj text of a mesh on the device -> uint8 CUDA tensor [bytes], on the tensors' device and current stream.
    verts: float32 [V,3], faces: int32 [F,3] (None: a point cloud), contiguous CUDA tensors; anything else is refused
    (RuntimeError for a type, dtype, device or stride, hip.ListError / ERR_SHAPE for a shape).  The one host
    synchronisation reads the two totals (bytes, bytes of the vertex lines) back between the two calls."""
    import torch
    verts, faces = _dev_inputs(verts, faces)
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), verts.device
    lib = load()
    with torch.cuda.device(dev):
        ws = _section.workspace(dev, lib.list_objtext_workspace_bytes(V, F), "list_objtext_workspace_bytes")
        totals = torch.empty((2,), dtype=torch.int64, device=dev)
        stream = hip._stream()
        _check(lib.list_objtext_count(_ptr(verts), _ptr(faces), V, F, ws.data_ptr(), ws.numel(), totals.data_ptr(),
                                      stream), "list_objtext_count")
        n = int(totals.tolist()[0])                             # the read-back
        out = torch.empty((n,), dtype=torch.uint8, device=dev)
        _check(lib.list_objtext_emit(_ptr(verts), _ptr(faces), V, F, ws.data_ptr(), ws.numel(), _ptr(out), n, stream),
               "list_objtext_emit")
    return out


def write_obj(path, verts, faces=None):
    """utils.write_obj's file from CUDA tensors: obj_text, one device-to-host copy, one write -> the byte count."""
    data = obj_text(verts, faces).cpu().numpy()
    with open(path, "wb") as f:
        f.write(memoryview(data))
    return int(data.size)


def obj_text_host(verts, faces=None):
    """The same bytes from the library's host-only entry (list_objtext_host: csrc/objtext_math.h compiled for the CPU, no
    device used) -> bytes.  verts: array-like [V,3] float32, faces: array-like [F,3] int32."""
    v, f = _host_inputs(verts, faces)
    lib = load()
    p = lambda a: a.ctypes.data if a.size else None
    n = lib.list_objtext_host(p(v), p(f), len(v), len(f), None, 0)
    if n < 0:
        _check(int(n), "list_objtext_host")
    out = np.empty(n, dtype=np.uint8)
    _check(min(int(lib.list_objtext_host(p(v), p(f), len(v), len(f), p(out), n)), 0), "list_objtext_host")
    return out.tobytes()


# ---- host: the rule in numpy ----------------------------------------------------------------------------------------
_tables = None


def tables():
    """(pow5_inv uint64 [21,2], pow5 uint64 [64,2]) parsed from csrc/objtext_tables.h: 128-bit entries as (low, high)."""
    global _tables
    if _tables is None:
        text = open(_TABLES_H).read()

        def body(name):
            m = re.search(name + r"\[\w+\]\[2\]\s*=\s*\{(.*?)\n\};", text, flags=re.S)
            return np.array([int(x) for x in re.findall(r"(\d+)ull", m.group(1))], dtype=np.uint64).reshape(-1, 2)

        inv, pw = body("kObjtextPow5Inv"), body("kObjtextPow5")
        assert len(inv) == int(re.search(r"OBJTEXT_N_POW5_INV (\d+)", text).group(1))
        assert len(pw) == int(re.search(r"OBJTEXT_N_POW5 (\d+)", text).group(1))
        _tables = inv, pw
    return _tables


_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _pow5bits(e):
    return ((e * 1217359) >> 19) + 1


def _mul64(a, b):
    """a * b of uint64 arrays -> (high, low) uint64 words, from 32-bit halves (no partial sum passes 2^64)."""
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    return p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32), (p00 & _M32) | ((mid & _M32) << _S32)


def _mulshift(m, f, shift):
    """floor(m * f / 2^shift): m uint64 [T], f uint64 [T,2] = (low, high) words, 64 < shift < 128 (int64 [T])."""
    h0, _ = _mul64(m, f[:, 0])
    h1, l1 = _mul64(m, f[:, 1])
    total = h0 + l1                                            # wraps like the header's uint64
    h1 = h1 + (total < h0)
    d = (shift - 64).astype(np.uint64)
    return (h1 << (np.uint64(64) - d)) | (total >> d)


def _multiple_of_pow5(v, p):
    """5^p divides v, element-wise (int64 v > 0 below 2^57: at most 24 factors)."""
    c, v = np.zeros_like(v), v.copy()
    for _ in range(25):
        act = v % 5 == 0
        if not act.any():
            break
        v = np.where(act, v // 5, v)
        c += act
    return c >= p


def shortest_cpu(bits):
    """uint32 bit patterns of finite non-zero float32 (the sign is ignored) -> (digits int64, exp10 int64, n int64): the
    shortest decimal of the same value as a float64, value = digits * 10^exp10, digits with n decimal digits --
    objtext_shortest of csrc/objtext_math.h, element-wise."""
    inv_t, pow_t = tables()
    b = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    mant, expo = b & 0x7FFFFF, (b >> 23) & 0xFF
    sub = expo == 0
    top = np.zeros_like(mant)                                   # a subnormal's highest set bit
    for k in range(1, 23):
        top += sub & (mant >= (1 << k))
    mant = np.where(sub, (mant << (23 - top)) & 0x7FFFFF, mant)
    expo = np.where(sub, top - 22, expo)
    field = mant << 29
    e2 = expo + 896 - 1023 - 52 - 2
    m2 = field | (1 << 52)
    mm_shift = (field != 0).astype(np.int64)
    mv, mp, mm = 4 * m2, 4 * m2 + 2, 4 * m2 - 1 - mm_shift
    big = e2 >= 0

    # e2 >= 0: divide by 10^q with the reciprocal table
    ea = np.where(big, e2, 0)
    qa = ((ea * 78913) >> 18) - (ea > 3)
    sa = -ea + qa + POW5_BITS + _pow5bits(qa) - 1
    fa = inv_t[qa]
    # e2 < 0: multiply by 5^(-e2 - q)
    eb = np.where(big, 1, -e2)
    qb = ((eb * 732923) >> 20) - (eb > 1)
    ib = eb - qb
    sb = qb - (_pow5bits(ib) - POW5_BITS)
    fb = pow_t[ib]
    f, shift = np.where(big[:, None], fa, fb), np.where(big, sa, sb)
    assert ((shift > 64) & (shift < 128)).all()
    vr, vp, vm = (_mulshift(x.astype(np.uint64), f, shift).astype(np.int64) for x in (mv, mp, mm))
    assert (vr >= 0).all() and (vp >= 0).all() and (vm >= 0).all()

    mv5 = mv % 5 == 0
    vr0a = mv5 & _multiple_of_pow5(mv, qa)
    vm0a = ~mv5 & _multiple_of_pow5(mm, qa)
    q01 = qb <= 1
    vr0b = q01 | ((qb < 63) & ((mv & ((np.int64(1) << np.clip(qb, 0, 62)) - 1)) == 0))
    vm0b = q01 & (mm_shift == 1)
    vr0, vm0 = np.where(big, vr0a, vr0b), np.where(big, vm0a, vm0b)
    last, removed = np.zeros_like(vr), np.zeros_like(vr)
    e10 = np.where(big, qa, qb + e2)

    def drop(act):
        nonlocal vr, vp, vm, last, vr0, removed
        vr0 = np.where(act, vr0 & (last == 0), vr0)
        last = np.where(act, vr % 10, last)
        vr, vp, vm = np.where(act, vr // 10, vr), np.where(act, vp // 10, vp), np.where(act, vm // 10, vm)
        removed = removed + act

    for _ in range(20):
        act = vp // 10 > vm // 10
        if not act.any():
            break
        vm0 = np.where(act, vm0 & (vm % 10 == 0), vm0)
        drop(act)
    for _ in range(20):
        act = vm0 & (vm % 10 == 0)
        if not act.any():
            break
        drop(act)
    last = np.where(vr0 & (last == 5) & (vr % 2 == 0), 4, last)
    digits = vr + (((vr == vm) & ~vm0) | (last >= 5))
    n = np.ones_like(digits)
    for k in range(1, 19):
        n += digits >= 10 ** k
    return digits, e10 + removed, n


def _digit_matrix(value, n, width):
    """The n decimal digits of value, left-aligned in `width` columns (zeros behind)."""
    i = np.arange(width, dtype=np.int64)[None, :]
    p = 10 ** np.clip(n[:, None] - 1 - i, 0, 18)
    return np.where(i < n[:, None], (value[:, None] // p) % 10, 0)


def _pick(dg, k):
    return np.take_along_axis(dg, np.clip(k, 0, dg.shape[1] - 1), axis=1)


def _f32_tokens(bits):
    """uint32 [T] -> (chars uint8 [T,23], zeros behind each token, lens int64 [T])."""
    b = np.asarray(bits, dtype=np.uint32).reshape(-1).astype(np.int64)
    T = len(b)
    a, neg = b & 0x7FFFFFFF, (b >> 31) == 1
    nan, inf, zero = a > 0x7F800000, a == 0x7F800000, a == 0
    special = nan | inf | zero
    D, e, n = shortest_cpu(np.where(special, 0x3F800000, a))
    positional = (e + n - 1 >= -4) & (e + n - 1 < 16)
    dg = _digit_matrix(D, n, MAX_DIGITS) + ord("0")
    p = np.broadcast_to(np.arange(MAX_TOKEN, dtype=np.int64)[None, :], (T, MAX_TOKEN))
    nn, ee = n[:, None], e[:, None]
    Z, DOT = ord("0"), ord(".")

    # positional: an integer | the point inside the digits | "0." zeros digits
    c_int = np.where(p < nn, _pick(dg, p), np.where(p == nn + ee, DOT, Z))
    ip = nn + ee
    c_mid = np.where(p < ip, _pick(dg, p), np.where(p == ip, DOT, _pick(dg, p - 1)))
    z = -ee - nn
    c_low = np.where(p == 1, DOT, np.where(p < 2 + z, Z, _pick(dg, p - 2 - z)))
    pos = np.where(ee >= 0, c_int, np.where(ee > -nn, c_mid, c_low))
    pos_len = np.where(e >= 0, n + e + 2, np.where(e > -n, n + 1, 2 - e))

    # scientific: d1[.d2..dn]e+XX
    sci_e = e + n - 1
    epos = np.where(n > 1, n + 1, 1)[:, None]
    mant = np.where(p == 0, _pick(dg, p), np.where(p == 1, DOT, _pick(dg, p - 1)))
    ae = np.abs(sci_e)[:, None]
    tail = np.where(p == epos, ord("e"), np.where(p == epos + 1, np.where(sci_e[:, None] < 0, ord("-"), ord("+")),
                                                   np.where(p == epos + 2, Z + ae // 10, Z + ae % 10)))
    sci = np.where(p < epos, mant, tail)
    sci_len = epos[:, 0] + 4

    body = np.where(positional[:, None], pos, sci)
    blen = np.where(positional, pos_len, sci_len)
    for mask, word in ((nan, b"nan"), (inf, b"inf"), (zero, b"0.0")):
        body = np.where(mask[:, None] & (p < 3), np.frombuffer(word + bytes(MAX_TOKEN - 3), dtype=np.uint8)[None, :], body)
        blen = np.where(mask, 3, blen)
    minus = neg & ~nan
    shifted = np.concatenate([np.full((T, 1), ord("-"), dtype=np.int64), body[:, :-1]], axis=1)
    chars = np.where(minus[:, None], shifted, body)
    lens = blen + minus
    assert T == 0 or (lens.max() <= MAX_TOKEN and lens.min() >= 1)
    return np.where(p < lens[:, None], chars, 0).astype(np.uint8), lens


def _index_tokens(idx):
    """int32 [T] -> (chars uint8 [T,11] of the decimal of idx + 1 in int64, lens int64 [T])."""
    v = np.asarray(idx, dtype=np.int32).reshape(-1).astype(np.int64) + 1
    T = len(v)
    neg, u = v < 0, np.abs(v)
    n = np.ones_like(u)
    for k in range(1, 10):
        n += u >= 10 ** k
    body = _digit_matrix(u, n, MAX_INDEX_TOKEN) + ord("0")
    shifted = np.concatenate([np.full((T, 1), ord("-"), dtype=np.int64), body[:, :-1]], axis=1)
    chars, lens = np.where(neg[:, None], shifted, body), n + neg
    p = np.arange(MAX_INDEX_TOKEN, dtype=np.int64)[None, :]
    return np.where(p < lens[:, None], chars, 0).astype(np.uint8), lens


def _lines(first, chars, lens, width):
    """L lines `first` " " t0 " " t1 " " t2 "\\n" from 3L tokens (chars [3L,w], lens [3L]) -> uint8 [total bytes]."""
    L, w = len(lens) // 3, chars.shape[1]
    chars, lens = chars.reshape(L, 3, w), lens.reshape(L, 3)
    M = np.zeros((L, width), dtype=np.uint8)
    M[:, 0] = ord(first)
    rows = np.arange(L)
    col = np.full(L, 1, dtype=np.int64)                         # where the next separator goes
    j = np.arange(w, dtype=np.int64)[None, :]
    for k in range(3):
        M[rows, col] = ord(" ")
        live = j < lens[:, k, None]
        r, c = np.nonzero(live)
        M[r, col[r] + 1 + c] = chars[:, k, :][live]
        col = col + 1 + lens[:, k]
    M[rows, col] = ord("\n")
    return M[np.arange(width, dtype=np.int64)[None, :] <= col[:, None]]


_CHUNK = 1 << 16


def format_f32_cpu(bits):
    """f"{numpy.float32}" of uint32 bit patterns (any shape, taken flat) by this module's integer rule -> numpy array of
    byte strings (dtype S23)."""
    b = np.asarray(bits, dtype=np.uint32).reshape(-1)
    out = np.empty(len(b), dtype=f"S{MAX_TOKEN}")
    for s in range(0, len(b), _CHUNK):
        chars, _ = _f32_tokens(b[s:s + _CHUNK])
        out[s:s + _CHUNK] = np.ascontiguousarray(chars).view(f"S{MAX_TOKEN}")[:, 0]
    return out


def _host_inputs(verts, faces):
    if hasattr(verts, "detach"):
        verts = verts.detach().cpu().numpy()
    if hasattr(faces, "detach"):
        faces = faces.detach().cpu().numpy()
    v = np.asarray(verts)
    if v.size == 0:
        v = np.zeros((0, 3), dtype=np.float32)
    f = np.zeros((0, 3), dtype=np.int32) if faces is None or np.asarray(faces).size == 0 else np.asarray(faces)
    if v.dtype != np.float32 or v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"verts of dtype {v.dtype} and shape {v.shape}: need float32 [V,3]")
    if f.dtype != np.int32 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces of dtype {f.dtype} and shape {f.shape}: need int32 [F,3]")
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


def obj_text_cpu(verts, faces=None):
    """obj_text restated in numpy -> bytes.  verts: float32 [V,3], faces: int32 [F,3] or None (arrays; tensors are
    copied to the host); another dtype or shape is refused (ValueError)."""
    v, f = _host_inputs(verts, faces)
    parts = []
    vb = v.view(np.uint32).reshape(-1, 3)
    for s in range(0, len(vb), _CHUNK):
        chars, lens = _f32_tokens(vb[s:s + _CHUNK].reshape(-1))
        parts.append(_lines("v", chars, lens, MAX_VERTEX_LINE))
    for s in range(0, len(f), _CHUNK):
        chars, lens = _index_tokens(f[s:s + _CHUNK].reshape(-1))
        parts.append(_lines("f", chars, lens, MAX_FACE_LINE))
    return b"".join(p.tobytes() for p in parts)
