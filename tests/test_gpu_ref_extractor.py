"""The HIP extractor against the REFERENCE's own ORBextractor.cc -- directly, not through the oracle's restatement of it.

Two sources of the reference's results: tests/golden/ref_orb_mini.npz (recorded from the reference library, always there) and
oracle/_ref/libivf_ref_orb.so (tests/ref_lib.py: the reference's file compiled unmodified against oracle/cvshim/), which is
built where the reference tree exists and travels with the working tree.  Nothing here reads the reference tree.  The OpenCV
primitives under the reference's logic are the oracle's, so this pins the kernels to the reference's extractor logic; the
primitives stay pinned to the oracle by tests/test_gpu_parity.py.  Small shapes only: 1242x375 is covered there."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R
from iv_slam_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ref_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not R.available(), reason=R.SKIP_REASON)
BF = 386.1448
B = BF / 718.856


@pytest.fixture(scope="module")
def iv():
    import iv_slam_amd
    lib = iv_slam_amd.load()
    assert lib.ivf_device_count() >= 1, "no HIP device: libivfront has no CPU fallback"
    return iv_slam_amd


class Device:
    """iv.ORBextractor behind the surface oracle_lib.Extractor / ref_lib.Extractor have"""

    def __init__(self, iv, n, sf, nlevels, ini, mn, introspection=False):
        self.e = iv.ORBextractor(n, sf, nlevels, ini, mn, introspection)

    def __call__(self, img, cost=None):
        return self.e(img, cost)

    def pyramid(self, l):
        return self.e._level(self.e._lib.ivf_extractor_pyramid_level, l)

    def quality_pyramid(self, l):
        return self.e._level(self.e._lib.ivf_extractor_quality_level, l)

    def level_counts(self):
        return self.e.level_counts()

    def tables(self):
        nf, um = self.e.feature_tables()            # ivf_extractor_get_feature_tables
        return dict(scale=self.e.GetScaleFactors(), inv_scale=self.e.GetInverseScaleFactors(), sigma2=self.e.GetScaleSigmaSquares(),
                    inv_sigma2=self.e.GetInverseScaleSigmaSquares(), features_per_level=nf, umax=um)


def assert_bytes_equal(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s%r vs %s%r" % (what, a.dtype, a.shape, b.dtype, b.shape)
    if a.tobytes() != b.tobytes():
        if a.dtype.names:
            for f in a.dtype.names:
                bad = np.flatnonzero(a[f].view(np.uint32) != b[f].view(np.uint32))
                assert bad.size == 0, "%s: field %s differs at %d places, first %d: device %r, reference %r" % (
                    what, f, bad.size, bad[0], a[bad[0]], b[bad[0]])
        raise AssertionError("%s differs at %d of %d elements" % (what, int((a != b).sum()), a.size))


@pytest.mark.parametrize("case", ["plain", "intro"])
def test_device_equals_recorded_reference(iv, case):
    mini = np.load(os.path.join(GOLDEN, "mini_320x200.npz")); ref = np.load(os.path.join(GOLDEN, "ref_orb_mini.npz"))
    got = G.record(lambda *a: Device(iv, *a), mini["left"], mini["cost"] if case == "intro" else None)
    keys = sorted(k[len(case) + 1:] for k in ref.files if k.startswith(case + "_"))
    assert keys == sorted(got)
    for k in keys:
        assert_bytes_equal(np.asarray(got[k]), ref[case + "_" + k], case + "_" + k)


N = 1000      # at these sizes the upper levels find fewer corners than their quota: redistribution and both retainBest calls run


@needs_ref
@pytest.mark.parametrize("mode", ["plain", "cost", "zero"])
@pytest.mark.parametrize("size", [(320, 200), (333, 207)], ids=lambda s: "%dx%d" % s)
def test_device_equals_reference_library(iv, size, mode):
    """keypoints, descriptors, level counts, every pyramid and quality plane and the tables, byte for byte.  `zero`: introspection
    on with an all-zero cost map, which leaves weights, quotas and responses alone and isolates the stale hY of the cell rows."""
    w, h = size
    img, _ = synth.make_pair(w, h, seed=7, idx=0)
    cost = {"plain": None, "cost": synth.make_cost_map(w, h, seed=7, idx=0), "zero": np.zeros_like(img)}[mode]
    d = Device(iv, N, 1.2, 8, 20, 7, mode != "plain")
    r = R.Extractor(N, 1.2, 8, 20, 7, mode != "plain")
    dk, dd = d(img, cost)
    rk, rd = r(img, cost)
    assert len(rk) > 0
    assert_bytes_equal(dk, rk, "keypoints")
    assert_bytes_equal(dd, rd, "descriptors")
    assert d.level_counts() == r.level_counts()
    for l in range(8):
        assert_bytes_equal(d.pyramid(l), r.pyramid(l), "pyramid level %d" % l)
        if mode != "plain":
            assert_bytes_equal(d.quality_pyramid(l), r.quality_pyramid(l), "quality level %d" % l)
    td, tr = d.tables(), r.tables()
    for k in tr:
        assert_bytes_equal(td[k], tr[k], "table " + k)


@needs_ref
def test_batched_frontend_equals_reference_library(iv):
    """one ivf_frontend_run of 3 pairs with cost maps: left images against the reference with introspection on and the pair's map,
    right images against the reference with introspection off (the right extractor is built without it and ignores the map)"""
    import torch
    w, h, n, pairs = 320, 200, 500, 3
    stream = synth.make_stream(pairs, w, h, seed=43)
    cost = np.stack([synth.make_cost_map(w, h, seed=43, idx=i) for i in range(pairs)])
    dev = torch.device("cuda:0")
    fe = iv.StereoFrontend(w, h, pairs, nfeatures=n, enableIntrospection=True, bf=BF, b=B)
    fe.run(torch.from_numpy(stream[:, 0].copy()).to(dev), torch.from_numpy(stream[:, 1].copy()).to(dev), torch.from_numpy(cost).to(dev))
    fe.sync()
    for p in range(pairs):
        rkL, rdL = R.Extractor(n, 1.2, 8, 20, 7, True)(stream[p, 0], cost[p])
        rkR, rdR = R.Extractor(n, 1.2, 8, 20, 7, False)(stream[p, 1], cost[p])
        gl = fe.fetch(p, 0); gr = fe.fetch(p, 1)
        assert len(rkL) > 0 and len(rkR) > 0
        assert_bytes_equal(gl["kps"], rkL, "pair %d left keypoints" % p)
        assert_bytes_equal(gr["kps"], rkR, "pair %d right keypoints" % p)
        assert_bytes_equal(np.ascontiguousarray(gl["desc"]), rdL, "pair %d left descriptors" % p)
        assert_bytes_equal(np.ascontiguousarray(gr["desc"]), rdR, "pair %d right descriptors" % p)
