"""CPU side of the mapping and loop-closing search scenes (tests/mapping_scenes.py): on every scene the plain-Python restatement
tests/mapping_ref.py and the C oracle give the same result and count; every `expect` and `holds` entry of every scene is met, intermediates
included; every outcome code of every search is reached; the 128- and 129-candidate windows have exactly those counts; and every injected
fault of mapping_ref.FAULTS changes the restatement's result on a scene this module names.  A scene that stops standing on its gate fails
here, not silently on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O
import mapping_ref as R
import mapping_scenes as S

F = np.float32
ALL = S.all_scenes()
FLAT = [sc for k in ALL for sc in ALL[k]]
HAS_ORIENTATION = ("init", "bow", "triangulation")
# the scene on which each injected fault must change the result
CAUGHT_BY = {
    ("keyframe", "window_le"): "strict_radius", ("keyframe", "level_up"): "octaves", ("keyframe", "th_lt"): "occupancy_and_th",
    ("fuse", "window_le"): "strict_radius", ("fuse", "level_up"): "octaves", ("fuse", "th_lt"): "chi_square", ("fuse", "chi2_float"): "chi_square",
    ("fuse_scw", "window_le"): "strict_radius", ("fuse_scw", "level_up"): "octaves", ("fuse_scw", "th_lt"): "chi_square",
    ("sim3", "window_le"): "strict_radius", ("sim3", "level_up"): "octaves", ("sim3", "th_lt"): "agreement_and_th",
    ("sim3", "no_agreement_check"): "agreement_and_th",
    ("init", "window_le"): "window", ("init", "th_lt"): "th_and_ratio", ("init", "no_decrement_on_steal"): "steals", ("init", "decrement_twice"): "steals",
    ("bow", "th_le"): "nodes_and_gates", ("bow", "ignores_matched2"): "nodes_and_gates",
    ("triangulation", "th_lt"): "gates", ("triangulation", "sets_matched2"): "gates", ("triangulation", "first_minimum"): "gates",
    ("triangulation", "epipolar_float"): "tilted_dsqr", ("triangulation", "epipole_gate_on_stereo"): "gates",
}


def same(a, b):
    if isinstance(b, (float, np.floating)):
        return np.array(a, F).tobytes() == np.array(b, F).tobytes() or float(a) == float(b)
    return a == b


def sid(sc):
    return "%s-%s" % (sc.search, sc.name)


@pytest.mark.parametrize("sc", FLAT, ids=sid)
def test_scene(sc):
    for ori in ((True, False) if sc.search in HAS_ORIENTATION else (True,)):
        res, n, outcome, infos = S.run_ref(sc, ori)
        ores, on = S.run_entry(O, None, sc, ori)
        assert S.same_result(res, n, ores, on), "restatement %s, oracle %s (orientation %s)\n%s" % (n, on, ori, S.explain(sc, ores, res, outcome, infos))
    res, n, outcome, infos = S.run_ref(sc, True)
    assert sc.expect and sc.holds
    for item, oc, vals in sc.expect:
        assert outcome[item] == oc, "%s: %s, built for '%s'" % (sid(sc), S.describe(outcome, infos, item), R.NAMES[oc])
        for key, val in vals.items():
            assert key in infos[item] and same(infos[item][key], val), "%s: item %d: %s is %r, built for %r" % (sid(sc), item, key, infos[item].get(key), val)
    assert sorted(sc.holds) == list(range(len(res[0]))), "every output slot of a scene says what it must hold"
    for slot, val in sc.holds.items():
        assert res[0][slot] == val, "%s: slot %d holds %d, built for %d" % (sid(sc), slot, res[0][slot], val)
    if n is not None and sc.search != "sim3":
        assert n == int(np.isin(outcome, (R.ACCEPTED,)).sum()), "every accepted item that was not stolen or removed counts once"
    if hasattr(sc, "nmatches"):
        assert {o: S.run_ref(sc, o)[1] for o in (True, False)} == sc.nmatches


@pytest.mark.parametrize("search", list(ALL))
def test_every_outcome_is_reached(search):
    seen = np.zeros(len(R.NAMES), int)
    for sc in ALL[search]:
        res, n, outcome, infos = S.run_ref(sc)
        seen += np.bincount(outcome, minlength=len(R.NAMES))
        print("%-14s %-18s %3d + %3d keypoints, count %s; %s" % (search, sc.name, len(sc.rec1["kps"]), len(sc.rec2["kps"]), n, ", ".join(
            "%s: %d" % (R.NAMES[c], k) for c, k in enumerate(np.bincount(outcome, minlength=len(R.NAMES))) if k)))
    for c in R.CODES[search]:
        assert seen[c] > 0, "no %s scene reaches '%s'" % (search, R.NAMES[c])
    assert set(np.nonzero(seen)[0]) <= set(R.CODES[search])


@pytest.mark.parametrize("search", ["keyframe", "fuse", "fuse_scw", "sim3"])
def test_the_long_windows_hold_128_and_129_candidates(search):
    for n in (128, 129):
        sc = [s for s in ALL[search] if s.name == "window_%d" % n][0]
        infos = S.run_ref(sc)[3]
        assert infos[0]["n_window"] == n and infos[0]["n_level"] == n and len(sc.rec2["kps"]) == n
        assert len(O.features_in_area(sc.rec2["kps"], S.BOUNDS, float(sc.Q["u"][0]), float(sc.Q["v"][0]), float(sc.Q["radius"][0]), -1, 0)) == n


@pytest.mark.parametrize("search,fault", sorted(CAUGHT_BY), ids=lambda v: str(v))
def test_injected_fault_is_caught(search, fault):
    name = CAUGHT_BY[(search, fault)]
    sc = [s for s in ALL[search] if s.name == name][0]
    caught = [s.name for s in ALL[search]
              if any(not S.same_result(*S.run_ref(s, ori)[:2], *S.run_ref(s, ori, fault)[:2]) for ori in (True, False))]
    print("%s with fault %s: caught by %s" % (search, fault, ", ".join(caught)))
    assert name in caught, "fault '%s' passes the scene built for it (%s)" % (fault, name)
    assert not S.same_result(*S.run_ref(sc, True)[:2], *S.run_ref(sc, True, fault)[:2]), "caught only with the orientation check off"


def test_every_listed_fault_has_a_scene():
    assert sorted(CAUGHT_BY) == sorted((s, f) for s in R.FAULTS for f in R.FAULTS[s])


def test_the_feature_vector_walk_makes_both_jumps():
    sc = ALL["bow"][0]
    walk = R.search_by_bow_keyframes(sc.rec1["kps"], sc.rec1["desc"], sc.has1, sc.fv1, sc.rec2["kps"], sc.rec2["desc"], sc.has2, sc.fv2, 0.75, True)[4]
    assert walk == sc.walk and walk["jumps1"] > 0 and walk["jumps2"] > 0


@pytest.mark.parametrize("search", list(ALL))
def test_concatenated_scenes_equal_the_oracle(search):
    """the scenes of one call as one call: restatement against oracle on the whole (the GPU module runs the device on the same)"""
    for scs in S.groups(ALL[search]):
        c = S.concat(scs if len(scs) > 1 else scs * 2)
        for ori in ((True, False) if search in HAS_ORIENTATION else (True,)):
            res, n, outcome, infos = S.run_ref(c, ori)
            ores, on = S.run_entry(O, None, c, ori)
            assert S.same_result(res, n, ores, on), S.explain(c, ores, res, outcome, infos)
