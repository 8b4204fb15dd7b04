"""CPU side of the batched TrackReferenceKeyFrame matcher (ivf_tracker_search_by_bow): the numpy restatement tests/track_bow_ref.py equals the
C oracle's SearchByBoW on every scene of tests/track_bow_scenes.py, the scenes still reach every exit of the loop they were built for
(a scene that stops doing its job fails here, not silently on the GPU), and the two entry points are exported, bound and documented."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O
import track_bow_ref as R
import track_bow_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {d: S.scenes(d) for d in (3, 4)}


def restated(sc, levelsup=None, check_orientation=True, nn_ratio=0.7):
    kfv, ffv = S.node_ids(O, sc, levelsup)
    return R.search_by_bow(sc["kf"]["kps"], sc["kf"]["desc"], sc["kf"]["has"], kfv, sc["f"]["kps"], sc["f"]["desc"], ffv, nn_ratio, check_orientation)


@pytest.mark.parametrize("depth", [3, 4])
def test_trees_route_descriptors_by_their_address(depth):
    """the construction the scenes rest on: a descriptor lands on the leaf its address names, whatever its payload"""
    tree = S.TREES[depth]
    b = S.Builder(tree, 0)
    assert 18 <= len(b.nodes) <= 20 and tree["depth"] == depth
    kinds = sorted(set(len(c) for c in tree["children"] if c))
    assert min(kinds) >= 3 and max(kinds) == 5
    for nd in b.nodes:
        path, ids = S.path_of(tree, nd)
        d = np.stack([b.desc(nd, b.payload()) for _ in range(4)])
        wid, nid, wt = O.bow_transform(tree, d, depth - 2)
        assert (nid == ids[1]).all() and (wid == tree["word"][ids[-1]]).all(), nd
        assert (O.bow_transform(tree, d, depth)[1] == 0).all() and (O.bow_transform(tree, d, depth + 3)[1] == 0).all()
    d = b.desc([2], b.payload())[None]
    assert O.bow_transform(tree, d, depth - 2)[1][0] == 0                     # the leaf above the node level
    sp = S.path_to(tree, tree["stopped"])
    assert O.bow_transform(tree, b.desc(sp, b.payload())[None], depth - 2)[2][0] == 0.0


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("check_orientation", [True, False])
def test_restatement_equals_the_oracle_on_every_scene(depth, check_orientation):
    for sc in SCENES[depth]:
        for ls in (sc["levelsup"], depth, depth + 2):
            m, nm, outcome, _ = restated(sc, ls, check_orientation)
            om, onm = S.oracle(O, sc, ls, 0.7, check_orientation)
            assert nm == onm and np.array_equal(m, om), (sc["name"], ls)
            assert nm == int((m >= 0).sum()) == int((outcome == R.ACCEPTED).sum())
            assert check_orientation or not (outcome == R.ROT_REMOVED).any()


@pytest.mark.parametrize("depth", [3, 4])
def test_scenes_reach_every_exit_of_the_loop(depth):
    seen = np.zeros(8, int)
    by_name = {}
    for sc in SCENES[depth]:
        m, nm, outcome, neg = restated(sc)
        by_name[sc["name"]] = (sc, m, nm, outcome, neg)
        seen += np.bincount(outcome, minlength=8)
        print("%-20s %3d x %3d features, %2d matches; %s" % (sc["name"], len(sc["kf"]["kps"]), len(sc["f"]["kps"]), nm,
                                                            ", ".join("%s: %d" % (R.OUTCOME_NAMES[c], k) for c, k in enumerate(np.bincount(outcome, minlength=8)) if k)))
    for c in R.REQUIRED:
        assert seen[c] > 0, "no scene reaches '%s'" % R.OUTCOME_NAMES[c]
    sc, m, nm, outcome, neg = by_name["main"]
    assert nm >= 15 and neg >= 12, "the main scene yields %d final matches, %d through a negative rot" % (nm, neg)
    assert set(R.REQUIRED) <= set(outcome.tolist()) and (outcome == R.NOT_IN_VECTOR).sum() == 1
    kfv, ffv = S.node_ids(O, sc)
    kn, fn = sorted(kfv), sorted(ffv)
    assert kn[0] == 0 and 0 not in ffv and fn[1] not in kfv and kn[-1] > fn[-1] and fn[-1] not in kfv   # front and end: nodes on one side only
    assert any(a not in ffv for a in kn[1:-1]) and any(b not in kfv for b in fn[1:-1])     # and one of each in the middle
    # the gates, each at the feature built for it (keyframe features in the order main_scene adds them)
    k = 3 + 24
    assert outcome[k] == R.ACCEPTED and R.hamming(sc["kf"]["desc"][k], sc["f"]["desc"][m.tolist().index(k)]) == 50
    assert outcome[k + 1] == R.OVER_TH_LOW and outcome[k + 2] == R.ACCEPTED and outcome[k + 3] == R.RATIO_FAILED
    assert outcome[k + 4] == R.NODE_ABSENT and outcome[k + 5] == R.RATIO_FAILED                 # middle node; the tie
    assert outcome[k + 6:k + 8].tolist() == [R.ACCEPTED, R.ACCEPTED] and outcome[k + 8:k + 10].tolist() == [R.ACCEPTED, R.OVER_TH_LOW]
    assert outcome[k + 10:k + 12].tolist() == [R.ACCEPTED, R.ALL_CLAIMED] and outcome[k + 12:k + 14].tolist() == [R.NO_POINT, R.ACCEPTED]
    assert outcome[k + 14] == R.ROT_REMOVED
    f_tie = [i for i in range(len(sc["f"]["kps"])) if R.hamming(sc["f"]["desc"][i], sc["kf"]["desc"][k + 5]) == 10]
    assert len(f_tie) == 2 and (m[f_tie] == -1).all()
    sc, m, nm, outcome, neg = by_name["swapped_ends"]
    kfv, ffv = S.node_ids(O, sc)
    assert min(ffv) == 0 and 0 not in kfv and max(ffv) > max(kfv) and nm == 10
    sc, m, nm, outcome, neg = by_name["wide_nodes"]
    kfv, ffv = S.node_ids(O, sc)
    assert sorted(len(v) for v in ffv.values()) == [6, 70] and sorted(len(v) for v in kfv.values()) == [4, 70]
    assert m[[2, 65, 69]].tolist() == [0, 1, 2] and outcome[3] == R.RATIO_FAILED and nm == 7 and outcome[4 + 64] == R.RATIO_FAILED
    sc, m, nm, outcome, neg = by_name["one_node"]
    kfv, ffv = S.node_ids(O, sc)
    assert list(kfv) == [0] and list(ffv) == [0] and len(kfv[0]) == 80 and len(ffv[0]) == 90 and nm >= 15
    assert (outcome == R.NO_POINT).sum() == 9 and (outcome == R.ROT_REMOVED).sum() > 0
    sc, m, nm, outcome, neg = by_name["rotation_one_bin"]
    assert nm == 25 and (outcome == R.ROT_REMOVED).sum() == 5 and neg > 0                      # 25, 2, 1, 1, 1: the second bin is under a tenth
    sc, m, nm, outcome, neg = by_name["rotation_three_bins"]
    assert nm == 25 and (outcome == R.ROT_REMOVED).sum() == 4 and neg > 0                      # 12, 8, 5 stay; 3 and 1 go
    for w in ("f", "kf"):
        assert by_name["empty_" + w][2] == 0 and not (by_name["empty_" + w][1] >= 0).any()


def test_new_entry_points_are_exported_bound_and_documented():
    from iv_slam_amd import _lib, track
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    for name in ("ivf_tracker_search_by_bow", "ivf_tracker_points_from_keyframe"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % name, hdr, flags=re.S)
        assert m and "Tracking.cc:" in m.group(1), "%s: the header comment cites the reference" % name
    assert len(_lib._SIGS["ivf_tracker_search_by_bow"][1]) == 17 and len(_lib._SIGS["ivf_tracker_points_from_keyframe"][1]) == 9
    assert callable(track.BatchTracker.search_by_bow) and callable(track.BatchTracker.points_from_keyframe)


@pytest.mark.parametrize("name", ["large", "small"])
def test_size_sweep_inputs_are_not_vacuous(name):
    """the records of tests/test_gpu_bow_sizes.py under the oracle alone: a record with more than 64 words, a word that five keypoints
    reach, a keypoint lost to a stopped word; every (keyframe, frame) pair with 16 or more keypoints on both sides has a match, with the
    nodes one level below the root and with every feature in node 0"""
    import test_gpu_bow_sizes as Z
    Z.assert_sweep_not_vacuous(name)
    for kind in ("level1", "root"):
        Z.assert_pairs_not_vacuous(name, kind)
