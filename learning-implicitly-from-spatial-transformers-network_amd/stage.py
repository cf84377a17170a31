"""What the wrappers of the opt-in HIP stages (voxenc.py, imgenc.py, coarse.py) share above hip.Section: the weight
cache on the module, the refusals of `forward`, the per-launch timing loop and the one statement of the eval-mode BN
fold.  Plain functions; nothing of a stage's own network is here."""
import numpy as np
import torch


def align256(n):
    """Every array of a packed blob or a workspace starts on a 256-byte boundary."""
    return (n + 255) // 256 * 256


# ---- parameters ------------------------------------------------------------------------------------------------------
def state_numpy(module):
    """state_dict as numpy arrays."""
    return {k: v.detach().cpu().numpy() for k, v in module.state_dict().items()}


def bn_affine(g, b, m, v, eps, exact=False):
    """Eval-mode BN as y * s + t: s = g / sqrt(v + eps), t = b - m * s.  In fp32 every operation is rounded, in that
    order -- operation for operation as the device's prep computes them (fp32 add, correctly rounded sqrt and division,
    fp32 multiply and subtract); exact: float64."""
    ty = np.float64 if exact else np.float32
    g, b, m, v = (np.asarray(a).astype(ty) for a in (g, b, m, v))
    s = (g / np.sqrt(v + ty(eps), dtype=ty)).astype(ty)
    return s, (b - (m * s).astype(ty)).astype(ty)


def pack_cached(owner, slot, tensors, prep):
    """prep() cached in owner.__dict__[slot].  The cache holds for the SAME tensors with unchanged version counters,
    storage addresses, devices and dtypes: an optimizer step, load_state_dict (an in-place copy: the versions move),
    module.to() or .half() all rebuild.  The slot is None while prep runs: a prep that raises leaves no stale entry."""
    key = tuple((id(t), t._version, t.data_ptr(), str(t.device), t.dtype) for t in tensors)
    cached = owner.__dict__.get(slot)
    if cached is not None and cached[0] == key and all(a is b for a, b in zip(cached[1], tensors)):
        return cached[2]
    owner.__dict__[slot] = None
    packed = prep()
    owner.__dict__[slot] = (key, tensors, packed)
    return packed


def require_hip_module(where, device):
    if device.type != "cuda":
        raise RuntimeError(f"{where}: the module is on {device}; the HIP forward needs it on a HIP device")


def new_blob(device, nbytes):
    """A zeroed packed blob on `device`."""
    with torch.cuda.device(device):
        return torch.zeros((nbytes,), dtype=torch.uint8, device=device)


def f32_pointers(device=None):
    """-> (ptr, keep): ptr(x) is the address of x (a tensor where it lies, or a numpy array copied to `device`) as
    contiguous float32; `keep` holds those tensors until the caller drops it."""
    keep = []

    def ptr(x):
        if isinstance(x, torch.Tensor):
            t = x.detach().to(torch.float32).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
        keep.append(t)
        return t.data_ptr()
    return ptr, keep


# ---- forward ---------------------------------------------------------------------------------------------------------
def refuse_training_and_grad(flag, what, modules, inputs):
    """The two refusals of a stage's forward(): `flag` the model option (e.g. "vox_encoder"), `what` the noun
    ("encoder", "stage"), `modules` those the call runs, `inputs` its tensors (None entries are skipped)."""
    if any(m.training for m in modules):
        raise RuntimeError(f"{flag}='hip' is the inference forward only: the module is in training mode "
                           "(batch-statistics BatchNorm and the backward are not implemented in HIP).  Call .eval(), "
                           f"or train with --{flag} torch")
    if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in inputs)
                                    or any(p.requires_grad for m in modules for p in m.parameters())):
        raise RuntimeError(f"{flag}='hip' has no backward: gradients are required here (grad mode is on and the "
                           f"{what}'s inputs or parameters require them).  Wrap the call in torch.no_grad(), or use "
                           f"--{flag} torch")


def time_launches(run, n_steps, reps):
    """Milliseconds per launch (median over reps): run(0, n_steps) once -- a whole forward fills the buffers -- then
    each run(s, s + 1) alone between two events.  The caller selects the device."""
    out = []
    run(0, n_steps)
    for s in range(n_steps):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(s, s + 1)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        out.append(float(np.median(ts)))
    return out
