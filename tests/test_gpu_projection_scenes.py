"""The two projection searches of the batched tracker (ivf_tracker_search_local, ivf_tracker_run) on the hand-made scenes of
tests/projection_scenes.py: keypoints and map points ON every comparison of the reference's loops and one float beside it.  Bar: the
device's assignment and nmatches IDENTICAL to the oracle's (oracle/projection_oracle.py around the C oracle) and to the plain-Python
restatement's (tests/projection_ref.py), no tolerances; a failure names the scene, the query and where the restatement says it left the loop.
Scenes that share their call parameters run as the frame slots / pairs of ONE call and, in a second test, one call each."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import projection_ref as R
import projection_scenes as S
from test_gpu_track import iv, run_tracker  # noqa: F401  (iv: the module fixture)
from test_gpu_track_local import run_local

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
F = np.float32


def groups(scenes):
    out = {}
    for sc in scenes:
        out.setdefault(sc.group, []).append(sc)
    return list(out.values())


LOCAL = S.local_scenes()
MOTION = S.motion_scenes()


# ---- SearchLocalPoints ------------------------------------------------------------------------------------------------------------
def device_local(iv, scs, quality=None):
    th, nn_ratio, cos_limit, max_points = scs[0].group
    return run_local(iv, S.CAM, [sc.rec for sc in scs], list(range(len(scs))), [sc.points for sc in scs], [sc.T for sc in scs],
                     [sc.occupied for sc in scs], th, nn_ratio, max_points=max_points, cos_limit=cos_limit, quality=quality)


def check_local_scene(sc, got_a, got_nm, how):
    import projection_oracle as PO
    nC = len(sc.rec["kps"])
    nm, assign, outcome, infos = S.ref_local(sc)
    onm, oassign = S.oracle_local(O, PO, sc)
    assert nm == onm and np.array_equal(assign, oassign), sc.name
    got = got_a[:nC]
    assert np.array_equal(got, assign), "local scene %s (%s): device differs from the reference\n%s" % (sc.name, how, S.explain(R.LOCAL_NAMES, got, assign, outcome, infos))
    assert got_nm == nm, "local scene %s (%s): nmatches %d, reference %d; %s" % (sc.name, how, got_nm, nm, "; ".join(
        S.describe(R.LOCAL_NAMES, outcome, infos, q) for q in range(len(outcome)) if outcome[q] >= R.EMPTY_WINDOW)[:600])
    assert (got_a[nC:] == -1).all()


@pytest.mark.parametrize("scs", groups(LOCAL), ids=lambda g: "th%g_ratio%g_cos%g_cap%s" % g[0].group)
def test_local_scenes_as_the_frame_slots_of_one_call(iv, scs):
    a, nm = device_local(iv, scs)
    for k, sc in enumerate(scs):
        check_local_scene(sc, a[k], int(nm[k]), "slot %d of %d" % (k, len(scs)))


def test_local_scenes_one_call_each(iv):
    for sc in LOCAL:
        a, nm = device_local(iv, [sc])
        check_local_scene(sc, a[0], int(nm[0]), "alone")


def test_local_scenes_with_quality_arrays(iv):
    """one pass with the quality arrays given: UpdateQualityScores(F) (ORBmatcher.cc:128-132, :1108-1121) on the keypoints that received a
    point; scores on a 0.004 lattice, so differences fall on both sides of the 0.01 threshold and on ties"""
    import projection_oracle as PO
    scs = max(groups(LOCAL), key=len)
    rng = np.random.default_rng(23)
    off = np.cumsum([0] + [len(sc.points) for sc in scs])
    pq = (rng.integers(0, 250, int(off[-1])) * F(0.004)).astype(F); kq = (rng.integers(0, 250, (len(scs), S.NF)) * F(0.004)).astype(F)
    a, nm, gpq, gkq = device_local(iv, scs, quality=(pq, kq))
    changed = 0
    for k, sc in enumerate(scs):
        check_local_scene(sc, a[k], int(nm[k]), "with quality arrays")
        nC = len(sc.rec["kps"])
        ekq, epq = PO.update_quality_scores([int(v) for v in a[k, :nC]], kq[k, :nC], pq[off[k]:off[k + 1]])
        assert gkq[k, :nC].tobytes() == ekq.tobytes() and gpq[off[k]:off[k + 1]].tobytes() == epq.tobytes(), sc.name
        assert np.array_equal(gkq[k, nC:], kq[k, nC:])
        changed += int((ekq != kq[k, :nC]).sum())
    assert changed > 20


# ---- TrackWithMotionModel ---------------------------------------------------------------------------------------------------------
def device_motion(iv, scs, quality=None):
    recs, pairs, poses, flags = [], [], [], []
    for sc in scs:
        pairs.append((len(recs), len(recs) + 1))
        recs += [sc.last, sc.cur]
        poses.append((sc.T_last, sc.T_cur))
        flags += [sc.flags, np.zeros(len(sc.cur["kps"]), np.uint8)]
    return run_tracker(iv, S.CAM, recs, pairs, poses=poses, flags=flags if scs[0].use_flags else None, quality=quality, **scs[0].kw)


def check_motion_scene(sc, got_a, got_nm, how):
    import projection_oracle as PO
    nC = len(sc.cur["kps"])
    nm, assign, outcome, infos, passes = S.ref_motion(sc)
    onm, oassign = S.oracle_motion(O, PO, sc)
    assert nm == onm and np.array_equal(assign, oassign), sc.name
    got = got_a[:nC]
    assert np.array_equal(got, assign), "motion scene %s (%s): device differs from the reference\n%s" % (sc.name, how, S.explain(R.MOTION_NAMES, got, assign, outcome, infos))
    assert got_nm == nm, "motion scene %s (%s): nmatches %d, reference %d (%d passes); %s" % (sc.name, how, got_nm, nm, passes, "; ".join(
        S.describe(R.MOTION_NAMES, outcome, infos, q) for q in range(len(outcome)) if outcome[q] >= R.M_EMPTY_WINDOW)[:600])
    assert (got_a[nC:] == -1).all()


@pytest.mark.parametrize("scs", groups(MOTION), ids=lambda g: "%s%s" % (g[0].name, "_and_%d_more" % (len(g) - 1) if len(g) > 1 else ""))
def test_motion_scenes_as_the_pairs_of_one_call(iv, scs):
    a, nm = device_motion(iv, scs)
    for k, sc in enumerate(scs):
        check_motion_scene(sc, a[k], int(nm[k]), "pair %d of %d" % (k, len(scs)))


def test_motion_scenes_one_call_each(iv):
    for sc in MOTION:
        a, nm = device_motion(iv, [sc])
        check_motion_scene(sc, a[0], int(nm[0]), "alone")


@pytest.mark.parametrize("which", ["gates", "retry"])
def test_motion_scenes_with_quality_arrays(iv, which):
    """UpdateQualityScores(CurrentFrame) at the end of every SearchByProjection call (ORBmatcher.cc:1513-1515); the retried pair updates twice"""
    import projection_oracle as PO
    scs = [g for g in groups(MOTION) if any(sc.name.startswith(which) for sc in g)][0]
    rng = np.random.default_rng(29)
    pq = (rng.integers(0, 250, (len(scs), S.NF)) * F(0.004)).astype(F); kq = (rng.integers(0, 250, (len(scs), S.NF)) * F(0.004)).astype(F)
    a, nm, gpq, gkq = device_motion(iv, scs, quality=(pq, kq))
    changed = 0
    for k, sc in enumerate(scs):
        check_motion_scene(sc, a[k], int(nm[k]), "with quality arrays")
        q = (pq[k].copy(), kq[k].copy())
        S.oracle_motion(O, PO, sc, quality=q)
        assert gpq[k].tobytes() == q[0].tobytes() and gkq[k].tobytes() == q[1].tobytes(), sc.name
        changed += int((q[1] != kq[k]).sum())
    assert changed > 3
