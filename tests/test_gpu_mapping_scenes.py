"""The per-call mapping and loop-closing searches of ivf_match.hip (SearchByProjection(KF, Scw), both Fuse, SearchBySim3,
SearchForInitialization, SearchByBoW(KF, KF), SearchForTriangulation) on the hand-made scenes of tests/mapping_scenes.py: keypoints and
queries ON every comparison of the reference's loops and one step beside it.  Bar: results and counts IDENTICAL to the plain-Python
restatement (tests/mapping_ref.py), no tolerance anywhere; a failure names the scene, the slot and where the restatement says the item left
the loop.  Every scene runs through the host-array entry (iv.ORBmatcher.*) and, where one exists, through the resident-frame entry
(DeviceFrame.SearchKeyFramePoints / .FuseCandidates / .SearchBySim3); alone, and all scenes of one call concatenated into ONE call, where
`matched`, vMatchedDistance, vbMatched2 and the rotation histogram cross the scene boundaries (expected = the restatement on the whole)."""
import numpy as np
import pytest

import mapping_ref as R
import mapping_scenes as S
from test_gpu_parity import iv  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
ALL = S.all_scenes()
HAS_ORIENTATION = ("init", "bow", "triangulation")
HAS_RESIDENT = ("keyframe", "fuse", "fuse_scw", "sim3")


def run_resident(iv, sc):
    """the same call against frames that live on the device"""
    k1, k2, p = sc.rec1, sc.rec2, sc.params
    f2 = iv.DeviceFrame(k2["kps"], k2["desc"], k2["uright"], S.BOUNDS)
    if sc.search == "keyframe":
        m, nm = f2.SearchKeyFramePoints(sc.Q, sc.matched)
        return [m], nm
    if sc.search in ("fuse", "fuse_scw"):
        bi, bd = f2.FuseCandidates(p["inv_sigma2"], sc.Q)
        return [bi, bd], None
    f1 = iv.DeviceFrame(k1["kps"], k1["desc"], k1["uright"], S.BOUNDS)
    m, nf = f1.SearchBySim3(f2, sc.Q, sc.Q21)
    return [m], nf


def check(iv, sc, how):
    for ori in ((True, False) if sc.search in HAS_ORIENTATION else (True,)):
        res, n, outcome, infos = S.run_ref(sc, ori)
        entries = [("host arrays", lambda: S.run_entry(None, iv.ORBmatcher, sc, ori))]
        if sc.search in HAS_RESIDENT:
            entries.append(("resident frame", lambda: run_resident(iv, sc)))
        for entry, run in entries:
            got, gn = run()
            assert S.same_result(got, gn, res, n), "%s, %s, check_orientation %s: device count %s, restatement %s\n%s" % (
                how, entry, ori, gn, n, S.explain(sc, got, res, outcome, infos))


@pytest.mark.parametrize("search", list(ALL))
def test_scenes_one_call_each(iv, search):
    for sc in ALL[search]:
        check(iv, sc, "alone")


@pytest.mark.parametrize("search", list(ALL))
def test_scenes_of_one_call_concatenated(iv, search):
    for scs in S.groups(ALL[search]):
        check(iv, S.concat(scs if len(scs) > 1 else scs * 2), "%d scenes in one call" % max(len(scs), 2))
