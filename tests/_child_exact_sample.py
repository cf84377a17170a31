"""The grid-aligned exact checks on the GPU (tests/_exact_sample_case.py): shared by tests/test_exact_vox_gather_gpu.py and
tests/test_exact_vox_adjoint_gpu.py, which import it, and run as a script for the sides the library chooses by an environment
switch it reads once per process (LIST_GATHER_BOX, LIST_TAIL_RIDE, LIST_SCATTER_BOX, LIST_SCATTER_F32):

    python _child_exact_sample.py gather|adjoint SPEC ...      SPEC = pyramid:N-per-image:j_star[:precision:mode:overlap]

Every comparison is np.array_equal against float64; the script prints each mismatch and exits 1 when there is one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _exact_case as E                      # noqa: E402
import _exact_sample_case as S               # noqa: E402

C4 = (1, 4, 32, 64, 128, 128)
ODD = (6, 10, 14)
# name -> (sizes, channels, the call's form, the aligned size or None for level 1's)
PYRAMIDS = {
    "p8": (S.cubic(8), S.VOX_CHANNELS, "model", None),
    "p16": (S.cubic(16), S.VOX_CHANNELS, "plain", None),
    "p32": (S.cubic(32), S.VOX_CHANNELS, "model", None),
    "c4": (S.cubic(8), C4, "model", None),                                  # level 1 with 4 channels: every later column offset moves by 4 mod 8
    "nc8": (tuple(ODD if l == 2 else (8, 8, 8) for l in range(6)), S.VOX_CHANNELS, "plain", (8, 8, 8)),
    "nc": (tuple(ODD if l == 2 else (8, 8, 8) for l in range(6)), S.VOX_CHANNELS, "plain", ODD),      # the non-cubic level alone
}
# (precision, voxel maps as fp16)
GATHER_CONFIGS = (("fp16", True), ("fp16", False), ("bf16x3", False))


def case(pyramid, n, j_star, pile=0):
    sizes, channels, variant, align = PYRAMIDS[pyramid]
    B = 2 if n <= 1024 else 1                                           # 600 points, or 4 096 of one image
    return S.vox_case(sizes, channels, j_star, variant, B, n, align, pile)


def layout(channels, img_C=S.IMG_C):
    """make_layout (csrc/list_common.h): the first column of every level in gather order."""
    off, col = [0] * 6, img_C
    for l, c in enumerate(channels):
        if c != 1:
            off[l], col = col, col + 7 * c
    for l, c in enumerate(channels):
        if c == 1:
            off[l], col = col, col + 7
    return off


def rows_of(c):
    return (c["B"] * c["N"] + 255) // 256 * 256


def fwd_plan_words(c, precision, vox16, box=1, ride=1, gather_only=0):
    """The call as tests/csrc/query_fwd_plan_host.cpp reads it."""
    w = [f"prec={precision}", "img=pfeat", f"vox16={int(vox16)}", f"rows={rows_of(c)}", f"box={box}", f"ride={ride}",
         f"gather_only={gather_only}"]
    for l in range(6):
        w += [f"l{l}.C={c['channels'][l]}", "l%d.dims=%d,%d,%d" % ((l,) + c["sizes"][l])]
    return " ".join(w)


def adjoint_plan_case(VP, c, precision, mode, overlap, box_mode=-1, f32=False):
    """The call as tests/csrc/vox_adjoint_plan_host.cpp reads it."""
    off = layout(c["channels"])
    edits = []
    for l in range(6):
        edits += [f"l{l}.C={c['channels'][l]}", "l%d.dims=%d,%d,%d" % ((l,) + c["sizes"][l]), f"l{l}.off={off[l]}"]
    return VP.case(B=c["B"], N=c["N"], fp16=precision == "fp16", forked=overlap, mode={"auto": 0, "scatter": 1, "gather": 2}[mode],
                   box_mode=box_mode, f32=f32, edits=edits)


# ------------------------------------------------------------------------------------------ on the GPU
def load_hip():
    import torch
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date
    from list_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def prepare(hip, c, precision, vox16):
    vox = hip.prep_vox_maps([dev(m) for m in c["vox_maps"]], dtype="f16" if vox16 else "f32")
    params = {k: dev(v) for k, v in c["weights"].items()}
    packed = hip.prep_mlp_weights(params, vox.channels, S.IMG_C, precision)
    return vox, packed, params


def mismatch(got, want, what):
    """'' or one line that says where `got` (a tensor) leaves the float64 `want`."""
    got = got.detach().cpu().numpy()
    want = np.asarray(want, np.float64).reshape(got.shape)
    if np.array_equal(got.astype(np.float64), want):
        return ""
    return f"{what}: {E.first_mismatch(got.reshape(got.shape[0], -1), want.reshape(got.shape[0], -1))}"


def check_gather(hip, c, precision, vox16, want_box_levels=None):
    """gather_features on the aligned and perceptual columns, and sdf_query sorted and unsorted -> list of mismatches."""
    import torch
    vox, packed, _ = prepare(hip, c, precision, vox16)
    q, pf = dev(c["query"]), dev(c["percep_feat"])
    what = f"j*={c['j_star']} {precision} vox16={int(vox16)}"
    bad = []
    X = hip.gather_features(q, None, None, vox, packed, perm=c["perm"], scale=c["scale"], percep_feat=pf)
    assert tuple(X.shape) == (c["B"], c["F"], c["N"])
    Xc = X[:, torch.from_numpy(c["cols"]).to(X.device), :]
    bad.append(mismatch(Xc.reshape(-1, c["N"]), c["X_cols"].reshape(-1, c["N"]), f"gather_features {what} (row = b * columns + aligned column)"))
    for sort in (True, False):
        plan = {}
        sdf = hip.sdf_query(q, None, None, vox, packed, perm=c["perm"], scale=c["scale"], precision=precision, percep_feat=pf,
                            sort_points=sort, plan=plan)
        bad.append(mismatch(sdf, c["sdf"], f"sdf {what} sort_points={sort}"))
        if want_box_levels is not None:
            assert plan["box_levels"] == want_box_levels and plan["chunks"] == 1, (what, plan)
    return [b for b in bad if b]


def check_adjoint(hip, c, precision, mode, overlap):
    """sdf_query_backward(want_vox=True, want_mlp=False) on the aligned levels -> list of mismatches."""
    import torch
    vox, packed, params = prepare(hip, c, precision, precision == "fp16")
    packed_b = hip.prep_mlp_weights_bwd(params, vox.channels, S.IMG_C, precision)
    sdf, ctx = hip.sdf_query(dev(c["query"]), None, None, vox, packed, perm=c["perm"], scale=c["scale"], precision=precision,
                             percep_feat=dev(c["percep_feat"]), save_for_backward=True)
    out = hip.sdf_query_backward(ctx, dev(c["grad_sdf"]), packed_b, want_mlp=False, want_img=False, want_vox=True,
                                 vox_adjoint=mode, overlap=overlap)
    torch.cuda.synchronize()
    what = f"j*={c['j_star']} {precision} {mode} overlap={overlap}"
    bad = [mismatch(sdf, c["sdf"], f"sdf {what}")]
    for l in c["aligned"]:              # (the gradient of a level that is not aligned in this run is not compared)
        g = out["vox"][l]
        assert tuple(g.shape) == (c["B"],) + c["sizes"][l] + (c["channels"][l],)
        bad.append(mismatch(g.reshape(-1, c["channels"][l]), c["d_vox"][l].reshape(-1, c["channels"][l]),
                            f"d_vox[{l}] {what} (row = voxel, column = channel)"))
    return [b for b in bad if b]


def main(argv):
    kind, specs = argv[0], argv[1:]
    hip = load_hip()
    bad = []
    for spec in specs:
        f = spec.split(":")
        c = case(f[0], int(f[1]), int(f[2]), int(f[6]) if len(f) > 6 else 0)
        if kind == "gather":
            for precision, vox16 in GATHER_CONFIGS:
                bad += [f"{spec}: {b}" for b in check_gather(hip, c, precision, vox16)]
        else:
            bad += [f"{spec}: {b}" for b in check_adjoint(hip, c, f[3], f[4], bool(int(f[5])))]
        print(f"{spec}: done", flush=True)
    for b in bad:
        print("MISMATCH", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
