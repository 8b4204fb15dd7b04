"""The oracle's extractor against the REFERENCE's own ORBextractor.cc (compiled unmodified against oracle/cvshim/, loaded by
tests/ref_lib.py): constructor tables, keypoint records, descriptors, per-level counts and every pyramid / quality-pyramid
plane, compared as raw bytes -- no tolerances.  Both sides share the OpenCV primitives (the shim delegates them to the
oracle's orc_*), so what is pinned here is the extractor's own logic: the tables, the pyramids and their borders, the
ComputeKeyPointsOld cell grid with its float-to-int conversions, stale hY and quality-weighted quotas, the response scaling,
IC_Angle, the descriptor, and the level order and coordinate scaling of operator().

The fixture tests (tests/golden/ref_orb_mini.npz: results recorded from the reference library) need no library and always
run; the others skip only where neither the library nor the reference tree to build it from exists."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R
from iv_slam_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ref_golden as G  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not R.available(), reason=R.SKIP_REASON)
NLEVELS = 8


def compare(img, cost, n, ini, mn, introspection):
    """one extraction on both sides; returns the oracle's keypoints for input-sanity checks by the caller"""
    o = O.Extractor(n, 1.2, NLEVELS, ini, mn, introspection)
    r = R.Extractor(n, 1.2, NLEVELS, ini, mn, introspection)
    ko, do = o(img, cost)
    kr, dr = r(img, cost)            # a ShimAssertion here is a finding: the reference asked OpenCV for something out of range
    assert len(ko) == len(kr), "keypoint count: oracle %d, reference %d" % (len(ko), len(kr))
    assert o.level_counts() == r.level_counts()
    for f in O.KP_DTYPE.names:
        bad = np.flatnonzero(ko[f].view(np.uint32) != kr[f].view(np.uint32))
        assert bad.size == 0, "keypoint field %s differs first at %d: oracle %r, reference %r" % (f, bad[0], ko[bad[0]], kr[bad[0]])
    assert ko.tobytes() == kr.tobytes()
    assert do.tobytes() == dr.tobytes(), "descriptors differ at rows %r" % np.flatnonzero((do != dr).any(axis=1))[:8]
    quality = introspection and cost is not None
    for l in range(NLEVELS):
        po, pr = o.pyramid(l), r.pyramid(l)
        assert po.shape == pr.shape and po.tobytes() == pr.tobytes(), "pyramid level %d" % l
        # the 19-pixel border ComputePyramid puts round each level (the oracle stores none): reflect-101 of the level itself,
        # also for levels > 0 whose storage sits inside the bordered plane (BORDER_ISOLATED)
        assert np.array_equal(r.pyramid(l, 19), np.pad(po, 19, mode="reflect")), "pyramid border, level %d" % l
        qo, qr = o.quality_pyramid(l), r.quality_pyramid(l)
        if quality:
            assert qo.shape == qr.shape and qo.tobytes() == qr.tobytes(), "quality pyramid level %d" % l
            assert np.array_equal(r.quality_pyramid(l, 19), np.pad(qo, 19, mode="reflect")), "quality border, level %d" % l
        else:
            assert qr is None          # built only with introspection on AND a mask (ORBextractor.cc operator())
    return ko


# ---- constructor tables ----
@needs_ref
@pytest.mark.parametrize("nlevels", [4, 8])
@pytest.mark.parametrize("scale_factor", [1.2, 1.5])
@pytest.mark.parametrize("nfeatures", [300, 500, 1000, 2000, 4000])
def test_constructor_tables(nfeatures, scale_factor, nlevels):
    a = O.Extractor(nfeatures, scale_factor, nlevels).tables()
    b = R.Extractor(nfeatures, scale_factor, nlevels).tables()
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), "%s: oracle %r, reference %r" % (k, a[k], b[k])
    assert int(a["features_per_level"].sum()) == nfeatures


# ---- full extraction ----
# nfeatures per size: large enough that the upper levels find fewer corners than their quota at the small sizes, so the
# redistribution of unused quota (nToDistribute) and the final per-level retainBest both run
SIZES = [(320, 200, 1000), (333, 207, 1000), (640, 240, 2000), (1242, 375, 2000)]
MODES = ["plain", "cost", "zero", "full"]
_inputs = {}


def inputs(w, h):
    if (w, h) not in _inputs:
        L, _ = synth.make_pair(w, h, seed=7, idx=0)
        cost = synth.make_cost_map(w, h, seed=7, idx=0)
        for a in (L, cost):
            a.setflags(write=False)
        _inputs[(w, h)] = (L, cost)
    return _inputs[(w, h)]


def mode_cost(mode, img, cost):
    return {"plain": None, "cost": cost, "zero": np.zeros_like(img), "full": np.full_like(img, 255)}[mode]


@needs_ref
@pytest.mark.parametrize("thresholds", [(20, 7), (12, 7)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[:2])
def test_extraction(size, mode, thresholds):
    """introspection off; on with a cost map; on with an all-zero cost map (weights, quotas and responses untouched, which
    isolates the stale hY of the cell rows); on with an all-255 cost map (every weight 0, so the quota is ceil(0/0) under max)"""
    w, h, n = size
    img, cost = inputs(w, h)
    k = compare(img, mode_cost(mode, img, cost), n, thresholds[0], thresholds[1], mode != "plain")
    assert len(k) > 0 and k["octave"].max() == NLEVELS - 1


@needs_ref
def test_introspection_without_mask_and_mask_without_introspection():
    img, cost = inputs(320, 200)
    compare(img, None, 1000, 20, 7, True)
    compare(img, cost, 1000, 20, 7, False)


def flat_band_image(w=320, h=200):
    """mid-grey with corners of contrast 14 (below iniThFAST 20, above minThFAST 7) everywhere, and strong corners in the left
    third only: the cells right of it find <= 3 corners at 20 and are re-run at 7"""
    r = np.random.Generator(np.random.PCG64(1234))
    img = np.full((h, w), 128, np.int32)
    for _ in range(260):
        x = int(r.integers(2, w - 5)); y = int(r.integers(2, h - 5))
        img[y:y + 3, x:x + 3] += int(r.choice([-14, 14]))
    for _ in range(40):
        x = int(r.integers(2, w // 3)); y = int(r.integers(2, h - 5))
        img[y:y + 3, x:x + 3] = int(r.choice([20, 235]))
    return np.clip(img, 0, 255).astype(np.uint8)


@needs_ref
@pytest.mark.parametrize("introspection", [False, True])
def test_min_threshold_fallback(introspection):
    img = flat_band_image()
    cost = synth.make_cost_map(320, 200, seed=9, idx=0) if introspection else None
    k = compare(img, cost, 500, 20, 7, introspection)
    # the input does what it is for: without the re-run at minThFAST the result is another one, and it is not simply the 7/7 one
    k20, _ = O.Extractor(500, 1.2, NLEVELS, 20, 20, introspection)(img, cost)
    k7, _ = O.Extractor(500, 1.2, NLEVELS, 7, 7, introspection)(img, cost)
    assert len(k) > len(k20) and k.tobytes() != k7.tobytes()


@needs_ref
@pytest.mark.parametrize("introspection", [False, True])
def test_response_ties(introspection):
    """four-valued noise: corner scores fall on a handful of values, so nth_element / retainBest cut through long runs of equal
    responses in every cell and at every level; the survivors' order is then decided by the selection's own moves"""
    r = np.random.Generator(np.random.PCG64(77))
    img = (30 + 60 * r.integers(0, 4, size=(207, 333))).astype(np.uint8)
    cost = np.zeros_like(img) if introspection else None         # zero cost: responses stay integers, ties stay ties
    k = compare(img, cost, 500, 20, 7, introspection)
    lvl0 = k[k["octave"] == 0]["response"]
    assert len(np.unique(lvl0)) * 8 < len(lvl0)


# ---- the OpenCV-version switches reach both sides ----
@needs_ref
@pytest.mark.parametrize("variant", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
def test_variant_switches(variant):
    img, cost = inputs(320, 200)
    base_k, base_d = R.Extractor(1000, 1.2, NLEVELS, 20, 7, True)(img, cost)
    try:
        O.set_opencv_variant(*variant)
        compare(img, cost, 1000, 20, 7, True)
        k, d = R.Extractor(1000, 1.2, NLEVELS, 20, 7, True)(img, cost)
        assert k.tobytes() != base_k.tobytes() or d.tobytes() != base_d.tobytes(), "the switch did not reach the reference build"
    finally:
        O.set_opencv_variant()
    k, d = R.Extractor(1000, 1.2, NLEVELS, 20, 7, True)(img, cost)
    assert k.tobytes() == base_k.tobytes() and d.tobytes() == base_d.tobytes()


# ---- the shim refuses what OpenCV would refuse ----
@needs_ref
def test_out_of_range_view_is_an_error_not_a_read():
    """an image too small for its last level: the reference's cell window leaves the level and rowRange / colRange must throw
    (as CV_Assert does), surfacing as ShimAssertion -- never as a silent out-of-bounds read"""
    img = synth.make_left(64, 48, seed=3, idx=0)
    with pytest.raises(R.ShimAssertion):
        R.Extractor(300, 1.2, NLEVELS, 20, 7)(img)


# ---- recorded reference results ----
def assert_record_equal(got, g, prefix):
    keys = [k[len(prefix):] for k in g.files if k.startswith(prefix)]
    assert sorted(keys) == sorted(got), (sorted(keys), sorted(got))
    for k in keys:
        want = g[prefix + k]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), prefix + k


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "mini_320x200.npz")), np.load(os.path.join(GOLDEN, "ref_orb_mini.npz"))


@pytest.mark.parametrize("case", ["plain", "intro"])
def test_oracle_equals_recorded_reference(golden, case):
    mini, ref = golden
    assert_record_equal(G.record(O.Extractor, mini["left"], mini["cost"] if case == "intro" else None), ref, case + "_")


@pytest.mark.parametrize("case", ["plain", "intro"])
def test_recorded_reference_equals_oracle_fixture(golden, case):
    """the two committed files agree with each other: what the oracle recorded in mini_320x200.npz is what the reference did"""
    mini, ref = golden
    assert ref[case + "_kps"].tobytes() == mini[case + "_kpsL"].tobytes()
    assert ref[case + "_desc"].tobytes() == mini[case + "_descL"].tobytes()
    assert np.array_equal(ref[case + "_pyr_crc"], mini[case + "_pyr_crc"])
    assert np.array_equal(ref[case + "_level_counts"], mini[case + "_level_counts"])
    if case == "intro":
        assert np.array_equal(ref["intro_qpyr_crc"], mini["intro_qpyr_crc"])


@needs_ref
@pytest.mark.parametrize("case", ["plain", "intro"])
def test_library_reproduces_recorded_reference(golden, case):
    mini, ref = golden
    assert_record_equal(G.record(R.Extractor, mini["left"], mini["cost"] if case == "intro" else None), ref, case + "_")


def test_fixture_is_results_only_and_small():
    ref = np.load(os.path.join(GOLDEN, "ref_orb_mini.npz"))
    assert all(k.split("_", 1)[0] in ("plain", "intro") for k in ref.files)
    assert ref["plain_kps"].dtype == O.KP_DTYPE and ref["plain_desc"].shape == (len(ref["plain_kps"]), 32)
    assert os.path.getsize(os.path.join(GOLDEN, "ref_orb_mini.npz")) <= os.path.getsize(os.path.join(GOLDEN, "mini_320x200.npz"))
