"""Connected components of a triangle mesh: drop the floating fragments an implicit network leaves around the object.

`label` and `keep_components` run on the tensors' device through liblist_hip.so (include/list_components.h) when they
are given CUDA tensors; `label_cpu` / `keep_components_cpu` are the same rules in numpy (no scipy) -- the CPU fallback
and the test oracle.  Both give, exactly:

  * the vertices are the nodes and a face links its three vertices: two faces that share ONE vertex are connected;
  * a face with an index outside [0, V) is invalid: it links nothing, is in no component and never in the output;
    degenerate (a,a,b / a,a,a) and duplicate faces are ordinary faces;
  * a vertex's label is the smallest vertex index of its component; a vertex no valid face uses is in no component
    (id -1) and never in the output;
  * components are numbered 0 .. K-1 in increasing order of label, each with its face count, vertex count and root;
  * `select_components` (one function, used by both paths) picks the kept ones from the K face counts;
  * kept vertices keep their order and their bits, kept faces keep their order with indices remapped.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np

from . import hip

INT32_MAX = 2 ** 31 - 1
MAX_ROUNDS = 64                 # LIST_CC_MAX_ROUNDS
# hook + compress rounds enqueued per read-back of their changed words.  A round after the fixpoint is two launches that
# return at once (4-5 microseconds each); a read-back is a stream synchronisation.  Counting the round that sees no
# change, 256^3 marching_cubes meshes took 3 and 5 rounds and strips with permuted ids up to 7:
# 8 is one read-back for all of them.
ROUNDS_PER_READBACK = 8

COMPONENTS_EXPORTS = {
    "list_cc_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "list_cc_begin": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "list_cc_rounds": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p]),
    "list_cc_finish": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "list_cc_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "list_cc_last_error": (C.c_char_p, []),
}

_section = hip.Section(COMPONENTS_EXPORTS, "list_cc_last_error")    # include/list_components.h on hip.load()'s handle
load, _check = _section.load, _section.check


class Labels(NamedTuple):
    """ids [V] (component of each vertex, -1 for none), then per component roots, n_faces, n_verts [K]; the number of
    invalid faces; and the hook + compress rounds that changed something plus the one that saw no change."""
    ids: object
    roots: object
    n_faces: object
    n_verts: object
    invalid_faces: int
    rounds: int


# ---- selection (host, both paths) -----------------------------------------------------------------------------------
def select_components(n_faces, keep="all", min_faces=0):
    """Which of the K components stay -> bool [K].  First the components with fewer than min_faces faces are dropped;
    then, for an integer keep = k > 0, the k with the most faces stay (ties go to the lower component id); keep = "all"
    keeps what min_faces left."""
    n = np.asarray(n_faces, dtype=np.int64).reshape(-1)
    if isinstance(min_faces, bool) or int(min_faces) != min_faces or min_faces < 0:
        raise ValueError(f"min_faces must be an integer >= 0 (got {min_faces!r})")
    ok = n >= int(min_faces)
    if isinstance(keep, str):
        if keep != "all":
            raise ValueError(f"keep must be 'all' or a positive integer (got {keep!r})")
        return ok
    if isinstance(keep, bool) or int(keep) != keep or keep < 1:
        raise ValueError(f"keep must be 'all' or a positive integer (got {keep!r})")
    order = np.lexsort((np.arange(n.size), -n))               # most faces first, the lower id first among equals
    order = order[ok[order]][:int(keep)]
    mask = np.zeros(n.size, dtype=bool)
    mask[order] = True
    return mask


def _info(K, mask, n_faces, n_verts, V, invalid, rounds):
    nf, nv = np.asarray(n_faces, dtype=np.int64), np.asarray(n_verts, dtype=np.int64)
    return {"K": int(K), "kept": np.flatnonzero(mask).astype(np.int32),
            "kept_faces": int(nf[mask].sum()), "kept_verts": int(nv[mask].sum()),
            "dropped_faces": int(nf[~mask].sum()), "dropped_verts": int(nv[~mask].sum()),
            "unused_verts": int(V - nv.sum()), "invalid_faces": int(invalid), "rounds": int(rounds)}


# ---- device ---------------------------------------------------------------------------------------------------------
def _is_cuda(x):
    return hasattr(x, "is_cuda") and x.is_cuda


def _faces_cuda(faces):
    import torch
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or not faces.is_cuda:
        raise RuntimeError(f"faces must be an int32 CUDA/HIP tensor (got {type(faces).__name__} "
                           f"{getattr(faces, 'dtype', None)} {getattr(faces, 'device', None)})")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise hip.ListError("components", hip.ERR_SHAPE, f"faces of shape {tuple(faces.shape)}: need [F,3]")
    return faces.contiguous()


def _check_count(V, F):
    if not 0 <= V <= INT32_MAX or F > INT32_MAX:
        raise hip.ListError("components", hip.ERR_SHAPE, f"V = {V}, F = {F}: both must be in [0, INT32_MAX]")


def _label_device(faces, V):
    """faces: contiguous int32 [F,3] on the device, F > 0, V > 0 -> (ids [V] on the device, table int32 [3,V] on the
    device whose rows hold roots / face counts / vertex counts in their first K entries, K, invalid faces, rounds,
    workspace)."""
    import torch
    lib = load()
    dev, F = faces.device, int(faces.shape[0])
    ws = _section.workspace(dev, lib.list_cc_workspace_bytes(V, F), "list_cc_workspace_bytes")
    stream = hip._stream()
    fp, wp, wn = faces.data_ptr(), ws.data_ptr(), ws.numel()
    _check(lib.list_cc_begin(fp, V, F, wp, wn, stream), "list_cc_begin")
    changed = torch.empty((ROUNDS_PER_READBACK,), dtype=torch.int32, device=dev)
    rounds = 0
    while True:
        # past the cap the library refuses, with its text: the loop ends in an error, never in a spin
        _check(lib.list_cc_rounds(fp, V, F, wp, wn, rounds, ROUNDS_PER_READBACK, changed.data_ptr(), stream),
               "list_cc_rounds")
        flags = changed.tolist()                               # the read-back
        if 0 in flags:
            rounds += flags.index(0) + 1
            break
        rounds += ROUNDS_PER_READBACK
    ids = torch.empty((V,), dtype=torch.int32, device=dev)
    table = torch.empty((3, V), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    _check(lib.list_cc_finish(fp, V, F, wp, wn, ids.data_ptr(), table[0].data_ptr(), table[1].data_ptr(),
                              table[2].data_ptr(), totals.data_ptr(), stream), "list_cc_finish")
    K, invalid = (int(x) for x in totals.tolist())
    return ids, table, K, invalid, rounds, ws


def label(faces, n_verts):
    """Components of the mesh with faces [F,3] over n_verts vertices -> Labels(ids, roots, n_faces, n_verts,
    invalid_faces, rounds).

    An int32 CUDA tensor takes the HIP path on its device and current stream and gets int32 tensors on that device; a
    tensor of another dtype is refused (RuntimeError), a shape other than [F,3] is refused (hip.ListError, ERR_SHAPE),
    a non-contiguous one is copied.  A CPU tensor or an array-like of any integer dtype goes to label_cpu and gets
    numpy arrays.  F = 0 or n_verts = 0 gives K = 0 and ids of -1 without a launch."""
    if not _is_cuda(faces):
        return label_cpu(faces, n_verts)
    import torch
    faces, V = _faces_cuda(faces), int(n_verts)
    F = int(faces.shape[0])
    _check_count(V, F)
    dev = faces.device
    if V == 0 or F == 0:
        e = torch.empty((0,), dtype=torch.int32, device=dev)
        return Labels(torch.full((V,), -1, dtype=torch.int32, device=dev), e, e.clone(), e.clone(), F if V == 0 else 0, 0)
    with torch.cuda.device(dev):
        ids, table, K, invalid, rounds, _ = _label_device(faces, V)
    return Labels(ids, table[0, :K], table[1, :K], table[2, :K], invalid, rounds)


def keep_components(verts, faces, keep="all", min_faces=0):
    """The mesh without the components select_components(face counts, keep, min_faces) drops ->
    (verts' float32 [V',3], faces' int32 [F',3], info).  info: K (components found), kept (their ids), kept_faces /
    kept_verts, dropped_faces / dropped_verts (of the dropped components), unused_verts (in no component),
    invalid_faces, rounds.

    CUDA tensors (verts float32 [V,3], faces int32 [F,3], one device) take the HIP path and get tensors on that device;
    another dtype is refused (RuntimeError), another shape is refused (hip.ListError, ERR_SHAPE), non-contiguous
    tensors are copied.  CPU tensors and array-likes go to keep_components_cpu, which converts them (float32 / any
    integer dtype) and gives numpy arrays.  V = 0 or F = 0 gives empty outputs without a launch."""
    if not (_is_cuda(verts) and _is_cuda(faces)):
        if _is_cuda(verts) or _is_cuda(faces):
            raise RuntimeError("verts and faces must both be CUDA/HIP tensors, or neither")
        return keep_components_cpu(verts, faces, keep, min_faces)
    import torch
    select_components(np.zeros(0, dtype=np.int64), keep, min_faces)            # a bad keep / min_faces: refused first
    hip._f32_cuda(verts, "verts")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise hip.ListError("components", hip.ERR_SHAPE, f"verts of shape {tuple(verts.shape)}: need [V,3]")
    faces = _faces_cuda(faces)
    if faces.device != verts.device:
        raise RuntimeError(f"verts on {verts.device}, faces on {faces.device}")
    verts = verts.contiguous()
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), verts.device
    _check_count(V, F)
    if V == 0 or F == 0:
        info = _info(0, np.zeros(0, dtype=bool), [], [], V, F if V == 0 else 0, 0)
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                info)
    lib = load()
    with torch.cuda.device(dev):
        ids, table, K, invalid, rounds, ws = _label_device(faces, V)
        counts = table[1:, :K].cpu().numpy()                   # face counts, vertex counts: K integers each
        mask = select_components(counts[0], keep, min_faces)
        info = _info(K, mask, counts[0], counts[1], V, invalid, rounds)
        Vk, Fk = info["kept_verts"], info["kept_faces"]
        out_v = torch.empty((Vk, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((Fk, 3), dtype=torch.int32, device=dev)
        if Vk:
            keep_dev = torch.from_numpy(mask.astype(np.uint8)).to(dev)
            _check(lib.list_cc_compact(verts.data_ptr(), faces.data_ptr(), V, F, ids.data_ptr(), keep_dev.data_ptr(), K,
                                       ws.data_ptr(), ws.numel(), out_v.data_ptr(), Vk,
                                       out_f.data_ptr() if Fk else None, Fk, hip._stream()), "list_cc_compact")
    return out_v, out_f, info


# ---- host -----------------------------------------------------------------------------------------------------------
def _faces_host(faces):
    if hasattr(faces, "detach"):
        faces = faces.detach().cpu().numpy()
    f = np.asarray(faces)
    if f.size == 0:
        f = f.reshape(-1, 3).astype(np.int64)
    if f.dtype.kind not in "iu":
        raise TypeError(f"faces must hold integers (got {f.dtype})")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces of shape {f.shape}: need [F,3]")
    return f.astype(np.int64)


def _label_host(f, V):
    """f int64 [F,3] -> (parent int64 [V] with parent[v] = v's label, used bool [V], valid bool [F], rounds): the
    device's rounds in numpy -- hook every root above a face's smallest root onto it (minimum), then point every
    vertex at its root -- until a round sees no face with two roots."""
    valid = ((f >= 0) & (f < V)).all(axis=1)
    g = f[valid]
    used = np.zeros(V, dtype=bool)
    used[g.ravel()] = True
    parent = np.arange(V, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        r = parent[g]                                          # the forest is flat: parent is the root
        m = r.min(axis=1, keepdims=True)
        hi = r != m
        if not hi.any():
            break
        np.minimum.at(parent, r[hi], np.broadcast_to(m, r.shape)[hi])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent, used, valid, rounds


def label_cpu(faces, n_verts):
    """label restated in numpy: faces array-like [F,3] of any integer dtype (a tensor is copied to the host) ->
    Labels of int32 numpy arrays."""
    f, V = _faces_host(faces), int(n_verts)
    _check_count(V, len(f))
    parent, used, valid, rounds = _label_host(f, V)
    is_root = used & (parent == np.arange(V))
    roots = np.flatnonzero(is_root)
    number = np.cumsum(is_root) - 1                           # at a root: its component id
    ids = np.where(used, number[parent], -1).astype(np.int32)
    K = roots.size
    n_faces = np.bincount(ids[f[valid, 0]], minlength=K).astype(np.int32)
    n_verts_ = np.bincount(ids[used], minlength=K).astype(np.int32)
    if V == 0 or len(f) == 0:
        rounds = 0
    return Labels(ids, roots.astype(np.int32), n_faces, n_verts_, int((~valid).sum()), rounds)


def keep_components_cpu(verts, faces, keep="all", min_faces=0):
    """keep_components restated in numpy -> (verts' float32 [V',3], faces' int32 [F',3], info), all on the host."""
    if hasattr(verts, "detach"):
        verts = verts.detach().cpu().numpy()
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    f = _faces_host(faces)
    V = len(v)
    lab = label_cpu(f, V)
    mask = select_components(lab.n_faces, keep, min_faces)
    info = _info(len(lab.roots), mask, lab.n_faces, lab.n_verts, V, lab.invalid_faces, lab.rounds)
    vkeep = np.zeros(V, dtype=bool)
    in_comp = lab.ids >= 0
    vkeep[in_comp] = mask[lab.ids[in_comp]]
    valid = ((f >= 0) & (f < V)).all(axis=1)
    fkeep = valid.copy()
    fkeep[valid] = vkeep[f[valid, 0]]
    vmap = np.cumsum(vkeep) - 1
    return v[vkeep].copy(), vmap[f[fkeep]].astype(np.int32).reshape(-1, 3), info
