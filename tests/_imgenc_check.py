"""The per-launch, per-element check of the HIP image encoder (list_amd.imgenc), shared by test_imgenc_cpu.py (which shows
on deliberately wrong layers that the check rejects them) and test_imgenc_gpu.py (which applies it to every launch of
the device).  Plain numpy float64; no GPU here.

A launch is one convolution with its epilogue, the max-pool, or the head.  It is judged on its own: the reference is
computed from the launch's OWN inputs as the device held them (bit-exact copies), so nothing compounds from layer to
layer, and every output element has its own bound (`reference`).  The derivation follows tests/_voxenc_check.py."""
import os
import sys

import numpy as np

from list_amd import imgenc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxenc_check as vc  # noqa: E402

U24 = vc.U24                        # unit roundoff of fp32
ratios = vc.ratios                  # error / bound per element; NaN and the infinities compared by class
half_bound = vc.half_bound          # the bound of an fp16 output: plus the storage rounding


class Launch:
    """One launch as the device runs it.  step: its imgenc.Step; w: float64 [Cout,Cin,k,k], the weights as the device holds
    them (fp32 for the stem, fp32 rounded to nearest even to fp16 for the matrix-core layers); w32: before any rounding;
    s, t: the fp32 BN scale and shift as float64.  The head: w [128,512] and t [128], the composed matrix and bias as
    the device holds them."""

    def __init__(self, step, w=None, s=None, t=None, w32=None):
        self.step, self.name, self.kind, self.w, self.s, self.t, self.w32 = step, step.name, step.kind, w, s, t, w32

    @property
    def mfma(self):
        return self.kind == "conv"


def launches(params, head=None):
    """The 22 launches of params_of(module), in imgenc.step_names() order.  head: (W [128,512], bias [128]) as the
    device holds them (Packed.head()); None: composed here."""
    st, eps, f64 = params["state"], params["eps"], np.float64
    out = []
    for step in imgenc.STEPS:
        if step.kind == "pool":
            out.append(Launch(step))
        elif step.kind == "head":
            w, b = head if head is not None else imgenc.compose_head(st)
            out.append(Launch(step, np.asarray(w, f64), None, np.asarray(b, f64)))
        else:
            w32 = np.asarray(st[step.key + ".weight"]).astype(np.float32)
            w = w32.astype(np.float16) if step.kind == "conv" else w32
            s, t = imgenc.bn_affine(st, eps[step.bn], step.bn)
            out.append(Launch(step, w.astype(f64), s.astype(f64), t.astype(f64), w32.astype(f64)))
    return out


def reference(L, x, idt=None, pad=None):
    """(y, bound) of launch L on the input x, float64 channels-last [B,H,W,Cin] holding the device's values exactly (idt:
    the identity [B,h,w,Cout], likewise).  y is the float64 value of every output element BEFORE the storage rounding;
    the device's fp32 level must lie within `bound` of it and its fp16 activation within `half_bound(y, bound)`.

    Convolutions.  With z = sum x w over the K = k k Cin products, A the same convolution of the absolute values and
    u = 2^-24, the bound is the sum of
      accumulation  e_acc = (K + 2) c u A, times |s| through the scale.  The products are exact in fp32 on the matrix
                    cores (fp16 x fp16 has 22 significant bits) and rounded inside an fma in the stem; the recursive-
                    summation bound of K roundings is below (K + 2) u for every K here and holds for ANY order.  c = 1
                    for the stem's fmaf chain, c = 2 for the matrix cores: the allowance _voxenc_check states for their
                    undocumented internal order and rounding -- fixed beforehand, not fitted.
      epilogue      one rounding per operation: the multiply by s and the add of t, 2 u (|s| (|z| + e_acc) + |t|); the
                    add of the identity (an exact fp16 value), u (|v| + |idt| + everything above).  ReLU is 1-Lipschitz
                    and exact.
      storage       (half_bound) half an fp16 ulp of the value that is rounded, 2^-11 (|y| + bound), or half a subnormal
                    step, 2^-25.
    Max-pool: exact, the bound is 0.  Head: mean = (sum of hw values, hw - 1 roundings, then one division):
    e_mean = (hw + 1) u mean|x|; vec = sum_k mean_k W_k + b in an fmaf chain of 512 roundings and the bias add:
    sum_k |W_k| e_mean_k + 514 u (sum_k |mean_k| |W_k| + |b|).
    Non-finite inputs: where A is not finite the accumulation term is dropped; such an element is non-finite in y (and
    compared by class) or exactly relu(-inf) = 0."""
    step = L.step
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if L.kind == "pool":
            y = imgenc._pool(x)
            return y, np.zeros_like(y)
        if L.kind == "head":
            hw = x.shape[1] * x.shape[2]
            flat = x.reshape(x.shape[0], hw, -1)
            mean, amean = flat.sum(axis=1) / hw, np.abs(flat).sum(axis=1) / hw
            e_mean = (hw + 1) * U24 * amean
            y = mean @ L.w.T + L.t
            bound = e_mean @ np.abs(L.w).T + 514 * U24 * ((np.abs(mean) + e_mean) @ np.abs(L.w).T + np.abs(L.t))
            return y, bound
        p = step.ks // 2 if pad is None else pad
        z = imgenc._conv2(x, L.w, step.stride, p)
        A = imgenc._conv2(np.abs(x), np.abs(L.w), step.stride, p)
        K = step.ks * step.ks * step.cin
        e_acc = (K + 2) * (2 if L.mfma else 1) * U24 * A
        e_acc = np.where(np.isfinite(A), e_acc, 0.0)
        fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)
        y = z * L.s + L.t
        bound = np.abs(L.s) * e_acc + 2 * U24 * (np.abs(L.s) * (fin(z) + e_acc) + np.abs(L.t))
        if idt is not None:
            idt = np.asarray(idt, dtype=np.float64)
            bound = bound + U24 * (fin(y) + fin(idt) + bound)
            y = y + idt
        if step.relu:
            y = np.where(y < 0, 0.0, y)                          # (a NaN stays a NaN)
    return y, bound


def check(L, x, idt=None, act=None, level=None):
    """The largest error / bound of launch L's outputs given its inputs: `act` its fp16 activation (vec for the head), `level`
    its fp32 level, both channels-last; None: not judged."""
    y, bound = reference(L, x, idt)
    worst = 0.0
    if act is not None:
        half = L.kind in ("stem", "conv")
        q = ratios(act, y, half_bound(y, bound) if half else bound, bound, half)
        worst = max(worst, float(q.max()))
    if level is not None:
        worst = max(worst, float(ratios(level, y, bound, bound, False).max()))
    return worst


# ---- the device's arithmetic, restated launch by launch (for the CPU tests) --------------------------------------------
def emulate(L, x, idt=None, pad=None):
    """Launch L in the device's own precisions (imgenc.encode_cpu's "device" arithmetic for one launch) -> (act, level):
    the sum in float64 rounded once to fp32, the epilogue in fp32; act is rounded to fp16 where the device stores fp16,
    level is the fp32 value (None for launches that write no level)."""
    f32, step = np.float32, L.step
    with np.errstate(over="ignore", invalid="ignore"):
        if L.kind == "pool":
            return imgenc._pool(np.asarray(x)), None
        if L.kind == "head":
            f4 = np.asarray(x, np.float64)
            hw = f4.shape[1] * f4.shape[2]
            mean = f4.reshape(f4.shape[0], hw, -1).sum(axis=1).astype(f32) / f32(hw)
            return (mean.astype(np.float64) @ L.w.T).astype(f32) + L.t.astype(f32), None
        p = step.ks // 2 if pad is None else pad
        z = imgenc._conv2(np.asarray(x, np.float64), L.w, step.stride, p).astype(f32)
        v = z * L.s.astype(f32) + L.t.astype(f32)
        if idt is not None:
            v = v + np.asarray(idt).astype(f32)
        if step.relu:
            v = np.where(v < 0, f32(0), v)
        return v.astype(np.float16), (v if step.level is not None else None)


def run_emulated(Ls, img):
    """Every launch on the outputs of those before, as the device chains them -> [(x, idt, act, level)] per launch,
    channels-last.  The head's x is the fp32 level 4."""
    x0 = np.moveaxis(np.asarray(img, np.float32), 1, 3)
    acts, out, f4 = [], [], None
    for L in Ls:
        s = L.step
        x = x0 if L.kind == "stem" else f4 if L.kind == "head" else acts[s.src]
        idt = acts[s.idt] if s.idt is not None else None
        act, level = emulate(L, x, idt)
        if s.level == 4:
            f4 = level
        acts.append(act)
        out.append((x, idt, act, level))
    return out


# ---- the fp32 graph against the exact one: a forward error bound -----------------------------------------------------
def fp32_graph_bound(params, img):
    """Per tensor, a bound on |encode_cpu("device", storage="fp32") - encode_cpu("exact")|, propagated through the exact
    graph: the same per-launch terms as `reference` with c = 1 (any fp32 summation), plus what an input error E does --
    conv(E, |w|) through a convolution, unchanged through ReLU, the identity add and the max-pool (all 1-Lipschitz) --
    and the rounding of the fp32 BN constants (s: an add, a square root and a division, 4 u |s|; t: 8 u (|b| + |m s|))
    and of the composed head (u |W|).  Second-order terms are covered by the factor 1.001.
    Returns {step name: bound [B,h,w,C]}, the head under "vec"."""
    st, eps, f64 = params["state"], params["eps"], np.float64
    ex = imgenc.encode_cpu(params, img, arithmetic="exact")
    x0 = np.moveaxis(np.asarray(img, f64), 1, 3)
    E, out = [], {}
    for k, step in enumerate(imgenc.STEPS):
        if step.kind == "pool":
            e = imgenc._pool(E[step.src])
        elif step.kind == "head":
            f4, e4 = ex["layer4_1_conv2"], E[k - 1]
            hw = f4.shape[1] * f4.shape[2]
            mean = np.abs(f4).reshape(f4.shape[0], hw, -1).sum(axis=1) / hw
            e_mean = e4.reshape(f4.shape[0], hw, -1).sum(axis=1) / hw + (hw + 1) * U24 * mean
            wc, bc = imgenc.compose_head(st, f64)
            e = (e_mean @ np.abs(wc).T + 516 * U24 * ((mean + e_mean) @ np.abs(wc).T + np.abs(bc))) * 1.001
            out["vec"] = e
            break
        else:
            x = x0 if step.kind == "stem" else ex[imgenc.STEPS[step.src].name]
            e_in = np.zeros_like(x) if step.kind == "stem" else E[step.src]
            w = np.asarray(st[step.key + ".weight"]).astype(f64)
            p = step.ks // 2
            K = step.ks * step.ks * step.cin
            z = imgenc._conv2(x, w, step.stride, p)
            e_z = imgenc._conv2(e_in, np.abs(w), step.stride, p) \
                + (K + 2) * U24 * imgenc._conv2(np.abs(x) + e_in, np.abs(w), step.stride, p)
            s, t = imgenc.bn_affine(st, eps[step.bn], step.bn, exact=True)
            ms = np.abs(np.asarray(st[step.bn + ".running_mean"]).astype(f64) * s)
            ds, dt = 4 * U24 * np.abs(s), 8 * U24 * (np.abs(np.asarray(st[step.bn + ".bias"]).astype(f64)) + ms)
            e = np.abs(s) * e_z + ds * (np.abs(z) + e_z) + dt + 2 * U24 * (np.abs(s) * (np.abs(z) + e_z) + np.abs(t))
            if step.idt is not None:
                v = z * s + t
                idt = ex[imgenc.STEPS[step.idt].name]
                e = e + E[step.idt] + U24 * (np.abs(v) + np.abs(idt) + e + E[step.idt])
            e = e * 1.001
        E.append(e)
        out[step.name] = e
    return out
