"""GPU: the per-launch timing loop the three opt-in HIP stages share (list_amd.stage.time_launches), through each stage's
time_steps at its smallest accepted shape: one finite positive time per launch, and the stage computes the same bits
right after it as before."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fill, synth
from list_amd import coarse, imgenc, voxenc
from list_amd.network.modules import PointMLP, ResEncoder, TreeGraphDecoder, VoxelEncoder2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coarse_check as cc  # noqa: E402
import _voxenc_check as vc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPS = 2


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as ge
    ge.build()                      # no-op when csrc/liblist_hip.so is up to date


def check_times(ms, n_steps):
    assert len(ms) == n_steps and n_steps > 0
    assert all(isinstance(t, float) and math.isfinite(t) and t > 0 for t in ms), ms


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        assert x is None or (x.data_ptr() != y.data_ptr() and torch.equal(x, y))


def test_voxenc_time_steps():
    m = fill.fill_state(VoxelEncoder2(vc.LIST_A), seed=2).eval().to(DEV)
    occ = torch.from_numpy((np.random.default_rng(11).random((1, 16, 16, 16)) < 0.03).astype(np.float32)).to(DEV)
    with torch.no_grad():
        packed = voxenc.pack(m)
        before = voxenc.encode(occ, packed)
        ms = voxenc.time_steps(occ, packed, reps=REPS)
        after = voxenc.encode(occ, packed)
    check_times(ms, len(voxenc.step_names(vc.LIST_A)))
    same(after, before)


def test_imgenc_time_steps():
    m = fill.fill_state(ResEncoder(), seed=3).eval().to(DEV)
    img = torch.from_numpy(synth.uniform(7, (1, 3, 32, 32)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        packed = imgenc.pack(m)
        vec0, lv0 = imgenc.encode(packed, img)
        ms = imgenc.time_steps(packed, img, reps=REPS)
        vec1, lv1 = imgenc.encode(packed, img)
    check_times(ms, imgenc.n_steps())
    same([vec1] + lv1, [vec0] + lv0)


class _Holder(torch.nn.Module):
    def __init__(self, g2=24, hidden=40):
        super().__init__()
        nn = torch.nn
        self.point_decoder = TreeGraphDecoder(1, cc.SMALL["features"], cc.SMALL["degrees"], 10)
        self.point_mlp_coarse = PointMLP()
        self.spatial_transformer = nn.Sequential(
            nn.Linear(512 + g2, hidden), nn.LeakyReLU(0.2), nn.BatchNorm1d(hidden),
            nn.Linear(hidden, hidden), nn.LeakyReLU(0.2), nn.BatchNorm1d(hidden), nn.Linear(hidden, 12))


def test_coarse_time_steps():
    m = fill.fill_state(_Holder(), seed=8).eval().to(DEV)
    feat_g = torch.from_numpy(synth.uniform(21, (1, cc.SMALL["features"][0])).astype(np.float32)).to(DEV)
    feat_g2 = torch.from_numpy(synth.uniform(22, (1, 24)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        packed = coarse.pack(m)
        before = coarse.decode(packed, feat_g, feat_g2, vox_res=16)
        ms = coarse.time_steps(packed, feat_g, feat_g2, vox_res=16, reps=REPS)
        after = coarse.decode(packed, feat_g, feat_g2, vox_res=16)
    check_times(ms, len(coarse.step_names(packed.shape)))
    assert all(t is not None for t in before)
    same(after, before)
