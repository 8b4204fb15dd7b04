"""ivf_stereo_match (k_stereo_rows, k_stereo_match, k_stereo_gate) on the hand-made keypoint scenes of tests/stereo_scenes.py: the
handles only supply the pyramids, the keypoints and descriptors are the caller's, so every gate of the match is set up by hand.
mvuRight and mvDepth must equal, byte for byte, the C oracle's and the numpy restatement's (tests/stereo_ref.py), whose per-keypoint
stages tests/test_stereo_ref_cpu.py asserts.  Every scene runs at a size whose row table is built in LDS (320x203) and at one where it
is built in global memory (160x801, H > 783).  The device's pyramid planes are compared with the oracle's first: a mismatch after that
can only be the matcher's."""
import numpy as np
import pytest

import iv_slam_amd as iv
from iv_slam_amd import _lib
import stereo_scenes as SC

pytestmark = pytest.mark.gpu
CASES = [(f, s) for f in SC.FAMILIES for s in SC.SIZES]


def handles(scene, ev):
    eL = iv.ORBextractor(scene.nfeatures, SC.SCALE_FACTOR, SC.NLEVELS, 20, 7); eR = iv.ORBextractor(scene.nfeatures, SC.SCALE_FACTOR, SC.NLEVELS, 20, 7)
    eL(scene.img_left); eR(scene.img_right)
    for e, want in ((eL, ev["pyr_left"]), (eR, ev["pyr_right"])):
        got = e.mvImagePyramid
        assert len(got) == len(want)
        for l in range(len(want)):
            assert got[l].shape == want[l].shape and np.array_equal(got[l], want[l]), "%s: pyramid level %d differs from the oracle" % (scene.name, l)
    assert np.array_equal(eL.GetScaleFactors(), SC.SCALE) and np.array_equal(eL.GetInverseScaleFactors(), SC.INV_SCALE)
    return eL, eR


def run_call(eL, eR, e, tag):
    kl, dl, kr, dr = e["arrays"]
    ur, dp = iv.ComputeStereoMatches(eL, eR, kl, dl, kr, dr, SC.BF, SC.B)
    for name, got, ref, orc in (("mvuRight", ur, e["ref"]["uright"], e["oracle"][0]), ("mvDepth", dp, e["ref"]["depth"], e["oracle"][1])):
        bad = np.flatnonzero(got.view(np.uint32) != orc.view(np.uint32))
        assert bad.size == 0, "%s: %s differs from the oracle at %s: %s, oracle %s, stages %s" % (
            tag, name, bad[:8], got[bad[:8]], orc[bad[:8]], [e["ref"]["stage"][i] for i in bad[:8]])
        assert got.tobytes() == ref.tobytes(), "%s: %s differs from the restatement" % (tag, name)
    return ur, dp


@pytest.mark.parametrize("family,size", CASES)
def test_scene(family, size):
    for scene in SC.build(family, size):
        ev = SC.evaluate(scene)
        eL, eR = handles(scene, ev)
        for e in ev["calls"]:
            assert e["ref"]["stage"] == e["call"].stage            # the scene is what it was built to be (asserted in full on the CPU)
            run_call(eL, eR, e, "%s/%s/%s" % (scene.name, e["call"].name, size))


@pytest.mark.parametrize("size", list(SC.SIZES))
def test_handle_reuse(size):
    """two calls on the same handles, the second with fewer right and fewer left keypoints: it must equal the same call on fresh
    handles.  (The outputs are n_left long, so what the first, longer call left in the handle's buffers beyond n_left is never
    returned; what it left in the row table and the scratch is what could leak.)"""
    scene, = SC.build("capacity", size)
    ev = SC.evaluate(scene)
    big, small = ev["calls"]
    assert len(small["arrays"][0]) < len(big["arrays"][0]) and len(small["arrays"][2]) < len(big["arrays"][2])
    eL, eR = handles(scene, ev)
    run_call(eL, eR, big, "capacity/row_cap")
    again = run_call(eL, eR, small, "capacity/smaller after row_cap")
    fL, fR = handles(scene, ev)
    fresh = run_call(fL, fR, small, "capacity/smaller on fresh handles")
    assert again[0].tobytes() == fresh[0].tobytes() and again[1].tobytes() == fresh[1].tobytes()
    assert len(again[0]) == len(small["arrays"][0])


def test_capacity_errors():
    """65535 right keypoints (index 0xffff is the matcher's `none`) and nfeatures + 1 left keypoints are refused"""
    scene, = SC.build("hamming", "lds")
    ev = SC.evaluate(scene)
    eL, eR = handles(scene, ev)
    kl, dl, kr, dr = ev["calls"][0]["arrays"]
    many_r = np.resize(kr, 65535); many_dr = np.resize(dr, (65535, 32))
    with pytest.raises(_lib.IvfError) as ei:
        iv.ComputeStereoMatches(eL, eR, kl, dl, many_r, many_dr, SC.BF, SC.B)
    assert ei.value.code == _lib.IVF_E_CAPACITY
    many_l = np.resize(kl, scene.nfeatures + 1); many_dl = np.resize(dl, (scene.nfeatures + 1, 32))
    with pytest.raises(_lib.IvfError) as ei:
        iv.ComputeStereoMatches(eL, eR, many_l, many_dl, kr, dr, SC.BF, SC.B)
    assert ei.value.code == _lib.IVF_E_CAPACITY
    # the largest accepted sizes right below them: nfeatures left keypoints (the first eight are the scene's)
    full_l = np.resize(kl, scene.nfeatures); full_dl = np.resize(dl, (scene.nfeatures, 32))
    ur, dp = iv.ComputeStereoMatches(eL, eR, full_l, full_dl, kr, dr, SC.BF, SC.B)
    import oracle_lib as O
    oL = O.Extractor(scene.nfeatures, SC.SCALE_FACTOR, SC.NLEVELS, 20, 7); oR = O.Extractor(scene.nfeatures, SC.SCALE_FACTOR, SC.NLEVELS, 20, 7)
    oL(scene.img_left); oR(scene.img_right)
    our, odp = O.stereo_match(oL, oR, full_l, full_dl, kr, dr, SC.BF, SC.B)
    assert ur.tobytes() == our.tobytes() and dp.tobytes() == odp.tobytes()
