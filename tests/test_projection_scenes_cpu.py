"""CPU side of the projection-search scenes (tests/projection_scenes.py): on every scene the plain-Python restatement tests/projection_ref.py
and the oracle (oracle/projection_oracle.py around the C oracle's window search) give the same assignment and nmatches; every outcome code of
both searches is reached; and every gate's query leaves the loop where it was built to, on both sides of the gate, with the intermediates
(level, radius, candidate counts, distances) it was built for.  A scene that stops doing its job fails here, not silently on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_lib as O
import projection_oracle as PO
import projection_ref as R
import projection_scenes as S

F = np.float32
LOCAL = S.local_scenes()
MOTION = S.motion_scenes()


def same(a, b):
    if isinstance(b, (float, np.floating)):
        return np.array(a, F).tobytes() == np.array(b, F).tobytes() or (float(a) == float(b))
    return a == b


def check_expectations(sc, names, assign, outcome, infos):
    assert sc.expect or sc.holds
    for q, oc, vals in sc.expect:
        assert outcome[q] == oc, "%s: %s, built for '%s'" % (sc.name, S.describe(names, outcome, infos, q), names[oc])
        for key, val in vals.items():
            assert key in infos[q] and same(infos[q][key], val), "%s: query %d: %s is %r, built for %r" % (sc.name, q, key, infos[q].get(key), val)
    for k, q in sc.holds:
        assert assign[k] == q, "%s: keypoint %d holds %d, built for %d" % (sc.name, k, assign[k], q)


def test_logf_restatement_equals_the_oracle():
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.exp(rng.uniform(-8, 8, 4000)).astype(F), np.array([1.0, 0.875, 4.0, S.SCALE[1]], F),
                         np.array([S.level_edge(k)[j] / F(4) for k in range(8) for j in (0, 1)], F)])
    for x in xs:
        assert R.logf(x).tobytes() == F(O.lib.orc_logf(float(x))).tobytes(), float(x)


@pytest.mark.parametrize("k", range(8))
def test_level_edges_are_adjacent_floats_on_both_sides_of_the_level(k):
    lo, hi = S.level_edge(k)
    assert np.nextafter(lo, F(np.inf)) == hi
    cur = dict(logScale=F(O.lib.orc_logf(float(S.SCALE[1]))), scale=S.SCALE)
    assert PO.predict_scale_f32(O, lo, F(4), cur) == k and PO.predict_scale_f32(O, hi, F(4), cur) == min(k + 1, 7)
    assert S.scale_quotient(lo) <= k < S.scale_quotient(hi)


@pytest.mark.parametrize("sc", LOCAL, ids=lambda s: s.name)
def test_local_scene(sc):
    nm, assign, outcome, infos = S.ref_local(sc)
    onm, oassign = S.oracle_local(O, PO, sc)
    assert nm == onm and np.array_equal(assign, oassign), "%s: restatement %d, oracle %d\n%s" % (sc.name, nm, onm, S.explain(R.LOCAL_NAMES, assign, oassign, outcome, infos))
    assert nm == int(np.isin(outcome, (R.ACCEPTED, R.ACCEPTED_THEN_REPLACED)).sum())
    assert len(sc.rec["kps"]) <= S.NF and len(sc.holds) == len(sc.rec["kps"]), "every keypoint of a scene says what it must hold"
    check_expectations(sc, R.LOCAL_NAMES, assign, outcome, infos)


def test_local_scenes_reach_every_outcome_and_both_paths_of_the_greedy_walk():
    seen = np.zeros(12, int)
    widest = 0
    for sc in LOCAL:
        nm, assign, outcome, infos = S.ref_local(sc)
        seen += np.bincount(outcome, minlength=12)
        widest = max([widest] + [i.get("n_window", 0) for i in infos])
        print("%-22s %3d keypoints %3d points %3d matches; %s" % (sc.name, len(sc.rec["kps"]), len(sc.points), nm, ", ".join(
            "%s: %d" % (R.LOCAL_NAMES[c], n) for c, n in enumerate(np.bincount(outcome, minlength=12)) if n)))
    for c, n in enumerate(seen):
        assert n > 0, "no scene reaches '%s'" % R.LOCAL_NAMES[c]
    assert widest == 65
    groups = set(sc.group for sc in LOCAL)
    assert {g[0] for g in groups} == {1.0, 3.0} and {g[2] for g in groups} == {0.5, 0.8} and {len(sc.points) for sc in LOCAL} >= {0, 16, 17, 32, 33}


def test_the_second_candidate_at_256_is_no_second_best():
    """ORBmatcher.cc:76-121 by hand on the scene built for it: 80 against a second at 256 is accepted with nn_ratio 0.3 although
    80 > 0.3f * 256, because `dist < bestDist2` is strict and bestLevel2 stays -1; against 255 it is rejected"""
    sc = [s for s in LOCAL if s.name == "second_at_256"][0]
    nm, assign, outcome, infos = S.ref_local(sc)
    assert F(80) > F(F(0.3) * F(256)) and F(80) > F(F(0.3) * F(255)) and not F(76) > F(F(0.3) * F(256))
    assert outcome.tolist() == [R.ACCEPTED, R.RATIO_FAILED, R.ACCEPTED, R.ACCEPTED] and nm == 3
    assert S.oracle_local(O, PO, sc)[0] == 3


@pytest.mark.parametrize("sc", MOTION, ids=lambda s: s.name)
def test_motion_scene(sc):
    nm, assign, outcome, infos, passes = S.ref_motion(sc)
    onm, oassign = S.oracle_motion(O, PO, sc)
    assert nm == onm and np.array_equal(assign, oassign), "%s: restatement %d, oracle %d\n%s" % (sc.name, nm, onm, S.explain(R.MOTION_NAMES, assign, oassign, outcome, infos))
    assert passes == sc.passes
    # every removed entry took one off nmatches (:1507), whoever held the keypoint by then
    assert nm == int(np.isin(outcome, (R.M_ACCEPTED, R.M_ACCEPTED_THEN_REPLACED)).sum())
    assert len(sc.holds) == len(sc.cur["kps"]), "every current keypoint of a scene says what it must hold"
    check_expectations(sc, R.MOTION_NAMES, assign, outcome, infos)
    if sc.name.startswith("close_rule"):
        assert int((outcome == R.M_ACCEPTED).sum()) == sc.n_taken == nm and sorted(PO.update_last_frame_points(sc.last, S.TH_DEPTH)) == \
            [q for q in range(len(outcome)) if outcome[q] == R.M_ACCEPTED]



def test_motion_scenes_reach_every_outcome_and_every_list_length():
    seen = np.zeros(11, int)
    windows = set()
    for sc in MOTION:
        nm, assign, outcome, infos, passes = S.ref_motion(sc)
        seen += np.bincount(outcome, minlength=11)
        windows |= set(i.get("n_window", 0) for i in infos)
        print("%-18s %3d last %3d current %3d matches, %d pass(es); %s" % (sc.name, len(sc.last["kps"]), len(sc.cur["kps"]), nm, passes, ", ".join(
            "%s: %d" % (R.MOTION_NAMES[c], n) for c, n in enumerate(np.bincount(outcome, minlength=11)) if n)))
    for c, n in enumerate(seen):
        assert n > 0, "no scene reaches '%s'" % R.MOTION_NAMES[c]
    assert windows >= {0, 1, 2, 16, 17, 63, 64, 65}
    rot = [s for s in MOTION if s.name == "rotation"][0]
    infos = S.ref_motion(rot)[3]
    assert [i["bin"] for i in infos] == [b for _, _, b in S.ROTATIONS] and sum(i["negative_rot"] for i in infos) == 2 and sum(i["wrapped"] for i in infos) == 1
    fl = [s for s in MOTION if s.name == "flags"][0]
    nm, assign, outcome, infos, _ = S.ref_motion(fl)
    assert nm == 26 and int((outcome == R.ROT_REMOVED).sum()) == 2 and int((assign >= 0).sum()) == 23
