"""The per-launch, per-element check of the HIP occupancy encoder (list_amd.voxenc), shared by test_voxenc_cpu.py
(which shows on deliberately wrong layers that the check rejects them) and test_voxenc_gpu.py (which applies it to
every launch of the device).  Plain numpy float64; no GPU here.

A launch is one 3x3x3 convolution with its epilogue.  It is judged on its own: the reference is computed from the
launch's OWN input as the device held it (a bit-exact copy), so nothing compounds from layer to layer, and every
output element has its own bound (`reference`)."""
import numpy as np

from list_amd import stage, voxenc

U24 = 2.0 ** -24                    # unit roundoff of fp32
F16_OVERFLOW = 65520.0              # round-to-nearest-even gives an infinity from here on (65504 + half an ulp)
LIST_A = [1, 1, 1, 1, 64, 16, 128, 16, 64]
LIST_B = [1, 1, 1, 1, 128, 128, 32, 16, 16]


class Launch:
    """One launch as the device runs it.  w: float64 [Cout,Cin,3,3,3], the weights as the device holds them (fp32, or
    fp32 rounded to nearest even to fp16 for the matrix-core layers); b, s, t: the fp32 bias and BN scale / shift as
    float64 (s, t None without BN); kind: "relu_bn", "relu" or "sigmoid"; mfma: accumulated on the matrix cores;
    half: the output is stored as fp16; stage, second: where it sits; D(R): side of its volume; w32: the module's
    fp32 weights before any rounding."""

    def __init__(self, name, stage, second, w, b, s, t, kind, mfma, half, w32=None):
        self.name, self.stage, self.second, self.w32 = name, stage, second, w32
        self.w, self.b, self.s, self.t, self.kind, self.mfma, self.half = w, b, s, t, kind, mfma, half
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])

    def D(self, R):
        return R if self.stage < 3 else R >> (self.stage - 3)

    def template(self):
        """What the launch instantiates: the fp32 kernels by name, voxenc_conv_kernel as <CC,NT>."""
        if not self.mfma:
            return "stencil" if self.cout == 1 else f"expand C={self.cout}"
        return f"<{16 if self.cin == 16 else 32},{self.cout // 16}>"


def bn_affine(state, eps, l):
    """s, t of stage l in fp32, operation for operation as the device's prep computes them (stage.bn_affine)."""
    return stage.bn_affine(state[f"bn.{l}.weight"], state[f"bn.{l}.bias"], state[f"bn.{l}.running_mean"],
                           state[f"bn.{l}.running_var"], eps)


def launches(params):
    """The 13 launches of params_of(module), in voxenc.step_names() order."""
    layers, eps, st = params["layers"], params["eps"], params["state"]
    f64 = np.float64

    def weights(name, half):
        w = np.asarray(st[f"conv.{name}.weight"]).astype(np.float32)
        b = np.asarray(st[f"conv.{name}.bias"]).astype(np.float32).astype(f64)
        return (w.astype(np.float16) if half else w).astype(f64), b, w.astype(f64)

    out = []
    for l in range(3):
        w, b, w32 = weights(f"conv_{l}", False)
        s, t = bn_affine(st, eps[l], l) if l < 2 else (None, None)
        out.append(Launch(f"conv_{l}", l, False, w, b, None if s is None else s.astype(f64),
                          None if t is None else t.astype(f64), "relu_bn" if l < 2 else "sigmoid", False, False, w32))
    for l in range(3, voxenc.N_STAGES):
        w, b, w32 = weights(f"conv_{l}", layers[l] != 1)
        out.append(Launch(f"conv_{l}", l, False, w, b, None, None, "relu", layers[l] != 1, True, w32))
        w, b, w32 = weights(f"conv_{l}_0", True)
        s, t = bn_affine(st, eps[l], l)
        out.append(Launch(f"conv_{l}_0", l, True, w, b, s.astype(f64), t.astype(f64), "relu_bn", True, True, w32))
    return out


def half_bound(y, head):
    """`head` plus the storage term of an fp16 output: half an ulp of the value that is rounded, 2^-11 (|y| + head), or
    half a subnormal step, 2^-25."""
    ya = np.where(np.isfinite(y), np.abs(y), 0.0)
    return head + 2.0 ** -11 * (ya + head) + 2.0 ** -25


def reference(x, L):
    """(y, bound, headroom) of launch L on the input x, float64 [B,Dz,Dy,Dx,Cin] holding the device's values exactly.
    y is the float64 value of every output element; the device's element must lie within `bound` of it.  `headroom`
    is the part of the bound before the storage rounding (used to judge an fp16 overflow, see `ratios`).

    With z = sum x w over the K = 27 Cin products, A = sum |x| |w| the same convolution of the absolute values,
    r = relu(z + b) and u = 2^-24 (fp32's unit roundoff), the bound is the sum of

      accumulation  e_acc = (K + 2) c u (A + |b|), times |s| under BN (ReLU is 1-Lipschitz).  The products are exact
                    in fp32 on the matrix cores (fp16 x fp16 has 22 significant bits) and rounded inside an fma in
                    the fp32 kernels; each of the at most K additions and the bias add rounds once, and the classical
                    recursive-summation bound gamma_n = n u / (1 - n u) of n = K + 1 roundings is below (K + 2) u for
                    every K here (K u <= 2.1e-4).  It holds for ANY order of summation.  c = 1 for the fp32 kernels
                    (fmaf chains) and c = 2 for the matrix cores: the stated allowance for their undocumented internal
                    summation order and rounding -- fixed beforehand, not fitted.
      epilogue      three fp32 roundings under BN (bias add, scale, shift; a contracted fma has fewer):
                    3 u (|s| (r + e_acc) + |t|).  ReLU alone: the bias add is the (K + 2)nd rounding of e_acc.
      storage       fp16 outputs: half an ulp of the value that is rounded, 2^-11 (|y| + everything above), or half a
                    subnormal step, 2^-25.  Nothing for fp32 outputs.
      sigmoid       y = 1 / (1 + expf(-(z + b))): e_acc passes through the sigmoid with its slope, and
                    |sigma'(xi)| <= min(1/4, y (1 - y) exp(|xi - z|)) because |d ln sigma' / dz| = |1 - 2 sigma| <= 1;
                    then 4 u |y| for expf, the add and the division.  This one constant is an ALLOWANCE: the ROCm
                    install carries no document of expf's accuracy (nothing under its doc or share trees names it),
                    so it assumes the 1 ulp (<= 2 u relative) that the OpenCL specification gives for exp, plus one
                    rounding each (u) for the add and the correctly rounded division.

    The second-order terms (a rounding of an already perturbed value) are kept so that the bound is a bound, not an
    estimate; they change it by parts in 10^4.

    Non-finite inputs: where A is not finite the accumulation term is dropped; such an element is either non-finite
    in y (and compared by class) or exactly relu(-inf) = 0 before the affine."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        z = voxenc._conv3(x, L.w)
        A = voxenc._conv3(np.abs(x), np.abs(L.w))
        K = 27 * L.cin
        e_acc = (K + 2) * (2 if L.mfma else 1) * U24 * (A + np.abs(L.b))
        e_acc = np.where(np.isfinite(A), e_acc, 0.0)
        pre = z + L.b
        if L.kind == "sigmoid":
            y = 1.0 / (1.0 + np.exp(-pre))
            slope = np.minimum(0.25, y * (1.0 - y) * np.exp(e_acc))
            head = e_acc * slope + 4 * U24 * np.abs(y)
        else:
            r = np.where(pre < 0, 0.0, pre)                     # (a NaN stays a NaN)
            if L.kind == "relu_bn":
                y = r * L.s + L.t
                rr = np.where(np.isfinite(r), r, 0.0)
                head = np.abs(L.s) * e_acc + 3 * U24 * (np.abs(L.s) * (rr + e_acc) + np.abs(L.t))
            else:
                y, head = r, e_acc
        bound = half_bound(y, head) if L.half else head
    return y, bound, head


def ratios(got, y, bound, head, half):
    """error / bound of every element (float64 array): inf where the classes differ.  NaN must meet NaN and an
    infinity the same infinity.  A finite y may meet an infinity of its sign in an fp16 output when |y| + headroom
    reaches the overflow threshold of round-to-nearest-even (65520): that IS y rounded to fp16 (not saturated)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == y.shape, (got.shape, y.shape)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        err = np.abs(got - y)
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        fin_y, fin_g = np.isfinite(y), np.isfinite(got)
        q = np.where(fin_y & fin_g, q, np.inf)
        q = np.where(np.isnan(y) & np.isnan(got), 0.0, q)
        q = np.where(np.isinf(y) & (got == y), 0.0, q)
        if half:
            over = fin_y & np.isinf(got) & (np.sign(got) == np.sign(y)) & (np.abs(y) + head >= F16_OVERFLOW)
            q = np.where(over, 0.0, q)
    return q


def check(got, x, L, inner=None):
    """The largest error / bound of launch L's output `got` given its input x (both [B,Dz,Dy,Dx,C]; x may be a crop
    that carries a halo, then inner = the three slices of got's block inside x)."""
    y, bound, head = reference(x, L)
    if inner is not None:
        sl = (slice(None),) + tuple(inner)
        y, bound, head = y[sl], bound[sl], head[sl]
    q = ratios(got, y, bound, head, L.half)
    return float(q.max()) if q.size else 0.0


def crop_range(lo, hi, D):
    """A block [lo, hi) of an axis of side D -> (a, b, slice): the input range [a, b) with one voxel of halo where the
    volume has one (at a face of the volume the zero padding of `reference` is the real one), and where the block
    lies inside it."""
    a, b = max(lo - 1, 0), min(hi + 1, D)
    return a, b, slice(lo - a, hi - a)


# ---- the device's arithmetic, restated launch by launch (for the CPU tests) --------------------------------------------
def emulate(x, L):
    """Launch L in the device's own precisions (voxenc.encode_cpu's storage="fp16" arithmetic for one layer): the sum
    in float64 rounded once to fp32, the epilogue in fp32, the output rounded to fp16 where the device stores fp16."""
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        z = voxenc._conv3(np.asarray(x, dtype=np.float64), L.w)
        if L.kind == "sigmoid":
            z = (z.astype(f32) + L.b.astype(f32)).astype(np.float64)
            return (1.0 / (1.0 + np.exp(-z))).astype(f32)
        r = z.astype(f32) + L.b.astype(f32)
        r = np.where(r < 0, f32(0), r)
        if L.kind == "relu_bn":
            r = r * L.s.astype(f32) + L.t.astype(f32)
        return r.astype(np.float16) if L.half else r


def run_emulated(occ, Ls, layer=emulate):
    """Every launch on the output of the one before, as the device chains them -> [(x, y)] per launch, channels-last."""
    net = np.asarray(occ, dtype=np.float32)[..., None]
    out = []
    for L in Ls:
        y = layer(net, L)
        out.append((net, y))
        net = y
        if L.second and L.stage < voxenc.N_STAGES - 1:
            net = voxenc._pool(net)
    return out
