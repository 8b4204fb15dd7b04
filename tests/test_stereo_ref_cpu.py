"""Frame::ComputeStereoMatches: the numpy restatement (tests/stereo_ref.py, written from Frame.cc) against the C oracle on hand-made
keypoint scenes (tests/stereo_scenes.py) and on extractor keypoints.  All comparisons are of bytes.  Every scene asserts the stage
each left keypoint was built to end at -- a keypoint that ends elsewhere is a failure, which is what keeps a scene from passing
vacuously -- and what else holds by construction: the winning iR, the pre-gate SAD, the best shift, the clamp value."""
import numpy as np
import pytest

import oracle_lib as O
import stereo_ref as SR
import stereo_scenes as SC
from iv_slam_amd import synth

F = np.float32
CASES = [(f, s) for f in SC.FAMILIES for s in SC.SIZES]


def row_count(kr, row):
    """how many right keypoints' bands cover `row` (Frame.cc:779-784)"""
    r = (F(2.0) * SC.SCALE[kr["octave"]]).astype(F)
    return int(((np.floor((kr["y"] - r).astype(F)) <= row) & (np.ceil((kr["y"] + r).astype(F)) >= row)).sum())


def check_call(scene, ev, e):
    c = e["call"]; ref = e["ref"]; kl, dl, kr, dr = e["arrays"]
    tag = "%s/%s" % (scene.name, c.name)
    assert len(c.stage) == len(kl) > 0
    assert ref["stage"] == c.stage, "%s: stages %s" % (tag, [(i, a, b) for i, (a, b) in enumerate(zip(ref["stage"], c.stage)) if a != b])
    for i, st in enumerate(c.stage):
        assert (ref["uright"][i] >= 0) == (ref["depth"][i] > 0) == (st == "matched"), tag
    for iL, key, val in c.checks:
        uL = F(kl["x"][iL])
        if key == "iR":
            assert ref["iR"][iL] == val, "%s: left %d won by %d, built for %d" % (tag, iL, ref["iR"][iL], val)
        elif key == "sad":
            assert ref["sad"][iL] == val, "%s: left %d SAD %d, built for %d" % (tag, iL, ref["sad"][iL], val)
        elif key == "bestinc":
            assert ref["bestinc"][iL] == val, "%s: left %d bestinc %d, built for %d" % (tag, iL, ref["bestinc"][iL], val)
        elif key == "row_count":
            assert row_count(kr, int(kl["y"][iL])) == val, tag
        elif key == "cols":
            assert ev["pyr_right"][val[0]].shape[1] == val[1], tag
        elif key == "clamp":
            assert ref["delta"][iL] == 0 and ref["uright"][iL] == F(np.float64(uL) - 0.01) and ref["depth"][iL] == F(F(SC.BF) / F(0.01)), tag
            assert ref["uright"][iL] < uL
        elif key == "closed_form":
            # octave 0, integer coordinates, SAD 0 at the best shift: deltaR = (d1 - d3) / (2 (d1 + d3)), |deltaR| <= 0.5, around uL - d
            want = F(F(uL - F(scene.d)) + ref["delta"][iL])
            assert ref["uright"][iL] == want and abs(float(ref["delta"][iL])) <= 0.5, tag
            assert ref["depth"][iL] == F(F(SC.BF) / F(uL - want)), tag
        else:
            raise AssertionError("unknown check %s" % key)


@pytest.mark.parametrize("family,size", CASES)
def test_scene(family, size):
    for scene in SC.build(family, size):
        ev = SC.evaluate(scene)
        assert scene.h % 4 != 0 and scene.img_left.min() >= 60 and scene.img_left.max() <= 190
        for e in ev["calls"]:
            our, odp = e["oracle"]
            assert e["ref"]["uright"].tobytes() == our.tobytes(), "%s/%s: mvuRight differs from the oracle" % (scene.name, e["call"].name)
            assert e["ref"]["depth"].tobytes() == odp.tobytes(), "%s/%s: mvDepth differs from the oracle" % (scene.name, e["call"].name)
            check_call(scene, ev, e)


def test_every_stage_is_built():
    """between them the scenes end keypoints at every stage the restatement knows, except `delta` (|deltaR| > 1 needs a best shift that is
    not a local minimum, which the first-minimum search over all eleven shifts cannot produce)"""
    seen = set()
    for family in SC.FAMILIES:
        for scene in SC.build(family, "lds"):
            for c in scene.calls:
                seen.update(c.stage)
    assert seen == set(SR.STAGES) - {"delta"}


@pytest.mark.parametrize("w,h,nf,seed", [(640, 240, 500, 3), (1242, 375, 1000, 0)])
def test_extractor_keypoints(w, h, nf, seed):
    L, R = synth.make_pair(w, h, seed=seed, idx=0)
    eL = O.Extractor(nf, 1.2, 8, 20, 7); eR = O.Extractor(nf, 1.2, 8, 20, 7)
    kl, dl = eL(L); kr, dr = eR(R)
    bf, b = 386.1448, 386.1448 / 718.856
    our, odp = O.stereo_match(eL, eR, kl, dl, kr, dr, bf, b)
    t = eL.tables()
    ref = SR.stereo_match([eL.pyramid(l) for l in range(8)], [eR.pyramid(l) for l in range(8)], t["scale"], t["inv_scale"], kl, dl, kr, dr, bf, b)
    assert ref["uright"].tobytes() == our.tobytes() and ref["depth"].tobytes() == odp.tobytes()
    assert int((our >= 0).sum()) > nf // 10
    assert {"matched", "gated", "hamming"} <= set(ref["stage"])


@pytest.mark.parametrize("mutation,family", [("th", "hamming"), ("tie", "ties")])
def test_wrong_restatement_is_caught(mutation, family):
    """the strength of the scenes: a restatement with `bestDist <= 75`, or with ties going to the later candidate, must differ from the
    oracle on the family built for that edge"""
    differs = False
    for scene in SC.build(family, "lds"):
        ev = SC.evaluate(scene)
        for e in ev["calls"]:
            kl, dl, kr, dr = e["arrays"]
            kw = dict(th_orb_dist=76) if mutation == "th" else dict(tie_last=True)
            bad = SR.stereo_match(ev["pyr_left"], ev["pyr_right"], SC.SCALE, SC.INV_SCALE, kl, dl, kr, dr, SC.BF, SC.B, **kw)
            differs |= bad["uright"].tobytes() != e["oracle"][0].tobytes()
    assert differs
