"""CPU: the byte counts of the stage units' workspaces and packed blobs, pinned as literals.

Every sizing function below is host arithmetic over a carved layout ("region a | region b | ...", each region on a
256-byte boundary): a slip in a layout moves its total at some shape.  Three shapes each: the smallest the function
accepts, an odd one at which no region is a multiple of 256 bytes (where the shape rules allow one: the encoders'
channel counts and the decoder's input widths are multiples of 16), and the workload's own.

The literals were recorded from the library as it was BEFORE the layouts were rewritten on csrc/list_host.h's Carver
(commit 56df71b), by running this file as a script in a checkout of that commit with its library built:

    PYTHONPATH=. python tests/test_stage_layouts_cpu.py

which prints the EXPECTED table.  They are not computed from the code under test.  The sections that size a hipCUB
scratch region (mesh, refine, components, eval) ask the device and are not pinned here."""
import pytest

from list_amd import chamfer, coarse, imgenc, prepare, render, s2loss, voxenc

VOX_DEFAULT = [1, 1, 1, 1, 16, 32, 64, 128, 128]
VOX_NARROW = [1, 1, 1, 1, 16, 16, 16, 16, 16]
VOX_MIXED = [1, 1, 1, 1, 64, 32, 128, 16, 64]
COARSE_DEFAULT = ([128, 128, 256, 256, 256, 128, 128, 3], [2, 2, 2, 2, 2, 2, 64], {})
COARSE_SMALLEST = ([16, 3], [1], {"has_mlp": False, "has_camera": False})
COARSE_ODD = ([16, 48, 3], [5, 9], {"g2": 1001, "hidden": 99})


def _vox_weights(layers):
    return voxenc.weight_bytes(layers)


def _vox_workspace(B, R, layers):
    return voxenc.workspace_bytes(B, R, layers)


def _coarse_weights(shape):
    f, d, kw = shape
    return coarse.weight_bytes(coarse.shape_of(f, d, **kw))


def _coarse_workspace(shape, B):
    f, d, kw = shape
    return coarse.workspace_bytes(coarse.shape_of(f, d, **kw), B)


# name -> (function, [argument tuples: smallest, odd, the workload's])
CASES = {
    "list_chamfer_workspace_bytes": (lambda *a: chamfer.load().list_chamfer_workspace_bytes(*a),
                                     [(1, 1, 1), (3, 5, 7), (12, 4096, 10000)]),
    "list_s2loss_workspace_bytes": (lambda *a: s2loss.load().list_s2loss_workspace_bytes(*a),
                                    [(1, 1, 1), (7, 3, 5), (8 * 128 ** 3, 8, 20000)]),
    "list_render_workspace_bytes": (lambda *a: render.load().list_render_workspace_bytes(*a),
                                    [(0, 1, 1), (1, 3, 5), (500000, 224, 224)]),
    "list_data_signed_distance_workspace_bytes":
        (lambda *a: prepare.load().list_data_signed_distance_workspace_bytes(*a), [(1,), (7,), (100000,)]),
    "list_voxenc_weight_bytes": (_vox_weights, [(VOX_NARROW,), (VOX_MIXED,), (VOX_DEFAULT,)]),
    "list_voxenc_workspace_bytes": (_vox_workspace, [(1, 16, VOX_NARROW), (3, 48, VOX_MIXED), (8, 128, VOX_DEFAULT)]),
    "list_imgenc_weight_bytes": (imgenc.weight_bytes, [()]),
    "list_imgenc_workspace_bytes": (imgenc.workspace_bytes, [(1, 32, 32), (3, 48, 80), (8, 224, 224)]),
    "list_coarse_weight_bytes": (_coarse_weights, [(COARSE_SMALLEST,), (COARSE_ODD,), (COARSE_DEFAULT,)]),
    "list_coarse_workspace_bytes": (_coarse_workspace, [(COARSE_SMALLEST, 1), (COARSE_ODD, 3), (COARSE_DEFAULT, 8)]),
}

EXPECTED = {
    'list_chamfer_workspace_bytes': [2048, 2304, 3383296],
    'list_s2loss_workspace_bytes': [17920, 17920, 17920],
    'list_render_workspace_bytes': [768, 768, 2401792],
    'list_data_signed_distance_workspace_bytes': [80, 560, 8000000],
    'list_voxenc_weight_bytes': [138496, 1912064, 3538176],
    'list_voxenc_workspace_bytes': [182784, 50930432, 760217600],
    'list_imgenc_weight_bytes': [22653696],
    'list_imgenc_workspace_bytes': [438272, 4930560, 171802624],
    'list_coarse_weight_bytes': [512, 1256448, 4699392],
    'list_coarse_workspace_bytes': [256, 9216, 1679360],
}


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


@pytest.mark.parametrize("name", sorted(CASES))
def test_byte_counts_are_the_recorded_ones(name):
    fn, shapes = CASES[name]
    assert len(EXPECTED[name]) == len(shapes)
    for args, want in zip(shapes, EXPECTED[name]):
        got = fn(*args)
        print(f"{name}{args}: {got} bytes, recorded {want}")
        assert got == want > 0, (name, args)


def test_an_odd_shape_has_no_region_of_a_multiple_of_256_bytes():
    """The odd shapes are odd: Chamfer's regions at B, N, M = 3, 5, 7 and the renderer's at F, H, W = 1, 3, 5, by the
    layouts' comments in csrc/loss_kernels.hip and csrc/render_kernels.hip."""
    B, N, M = CASES["list_chamfer_workspace_bytes"][1][1]
    for region in (8 * B * (N + M), 8 * 2 * B, 4 * B * N, 4 * B * M):
        assert region % 256 != 0
    F, H, W = CASES["list_render_workspace_bytes"][1][1]
    for region in (8 * H * W, 4 * F, 4 * 9):
        assert region % 256 != 0


if __name__ == "__main__":
    print("EXPECTED = {")
    for name in CASES:
        fn, shapes = CASES[name]
        print(f"    {name!r}: {[fn(*a) for a in shapes]!r},")
    print("}")
