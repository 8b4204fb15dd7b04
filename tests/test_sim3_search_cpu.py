"""CPU side of the two batched loop-closing searches (ivf_tracker_search_by_bow_keyframes, ivf_tracker_search_by_sim3): the restatement
tests/sim3_search_ref.py gives what every exact scene of tests/sim3_search_scenes.py states by hand, with the intended floats bit for bit;
it agrees with oracle/projection_oracle.py, an independent statement of the same two projection loops; the generic scenes keep every gate
quantity away from its threshold; the BoW scenes reach every way a KF1 feature can leave the loop; and tests/golden/sim3_search_noise.json,
the spreads measured here, is current.

The spreads are measured on the reference side only: the restatement run a second time entirely in f64.  `spread_px` = the largest
|f32 - f64| of any u, v; `spread_m` = of any z, dist3D.  Every gate quantity of a generic scene -- z against 0, u and v against the four
bounds and against every keypoint's +-r, dist3D against both range ends and every level boundary max_distance / 1.2^k -- must lie further
from its threshold than 64 x the spread of its unit: the device differs from the restatement only in libm and in how a scalar * Mat
product rounds, differences of the same kind and smaller.  A scene that fails this is moved (another seed), the test is not loosened.
`python tests/test_sim3_search_cpu.py --write` rewrites the file."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import mapping_ref as M
import sim3_search_ref as R
import sim3_search_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_PATH = os.path.join(ROOT, "tests", "golden", "sim3_search_noise.json")
F, D = np.float32, np.float64
SCENES = SC.sim3_scenes()
BOW = SC.bow_scenes()
EXACT = sorted(n for n, s in SCENES.items() if s["kind"] == "exact")
GENERIC = sorted(n for n, s in SCENES.items() if s["kind"] == "generic")
_REF = {}


def ref(name, f64=False):
    """the restatement on a scene, computed once and shared (tests/test_gpu_sim3_search.py reads it too)"""
    if (name, f64) not in _REF:
        s = SCENES[name]
        _REF[name, f64] = R.search(s["cam"], s["kf1"], s["kf2"], s["sim3"], s["match12"], s["inlier"], s["th"], f64=f64, nf=s["nf"])
    return _REF[name, f64]


def bow_ref(name, nn_ratio=SC.NN_RATIO, check_orientation=True):
    key = ("bow", name, nn_ratio, check_orientation)
    if key not in _REF:
        s = BOW[name]
        _REF[key] = R.search_by_bow_keyframes(s["tree"], s["levelsup"], s["kf1"], s["kf1"]["has"], s["kf2"], s["kf2"]["has"], nn_ratio, check_orientation, nf=s["nf"])
    return _REF[key]


def bits(x):
    return np.array(x, F).view(np.uint32)


@pytest.mark.parametrize("name", EXACT)
def test_exact_scenes_give_what_they_state_bit_for_bit(name):
    s, o = SCENES[name], ref(name)
    e = s["expect"]
    for key, n in (("match1", s["kf1"]["n"]), ("match2", s["kf2"]["n"]), ("matches", s["kf1"]["n"])):
        want = np.full(s["nf"], -1, np.int32)
        for i, j in e[key].items():
            want[i] = j
        assert np.array_equal(o[key], want), "%s %s: differs at %r" % (name, key, np.nonzero(o[key] != want)[0][:8])
    assert o["nfound"] == e["nfound"]
    info = (o["info1"], o["info2"])
    for side, i, field, value in s["exact"]:
        it = info[side][i]
        if field in it:                                                      # a point that is not projected (bad, already matched) has none
            assert bits(it[field]) == bits(value), "%s side %d keypoint %d: %s = %r, intended %r" % (name, side, i, field, it[field], value)
    for side, i, st in s["stage"]:
        assert R.STAGE_NAMES[info[side][i]["stage"]] == st, (name, side, i, R.STAGE_NAMES[info[side][i]["stage"]], st)


def test_the_exact_scenes_stand_on_every_boundary():
    """one side of each comparison, by what the restatement saw: the hand-made scenes are not vacuous"""
    o = ref("image_edges"); b = SC.EXACT_CAM["bounds"]
    us = [float(it["u"]) for it in o["info1"] if "u" in it]; vs = [float(it["v"]) for it in o["info1"] if "v" in it]
    assert b[0] in us and b[2] in us and b[1] in vs and b[3] in vs
    o = ref("depth_sign")
    zs = [it["z"] for it in o["info1"] if "z" in it]
    assert any(z == 0 and not np.signbit(z) for z in zs) and any(z == 0 and np.signbit(z) for z in zs) and any(z < 0 for z in zs)
    o = ref("range_ends")
    on = [it for it in o["info1"] if it.get("dist") is not None]
    assert sum(it["dist"] == it["min_d"] for it in on) == 1 and sum(it["dist"] == it["max_d"] for it in on) == 1
    assert sum(it["stage"] == R.TOO_NEAR for it in on) == 1 and sum(it["stage"] == R.TOO_FAR for it in on) == 1
    s, o = SCENES["radius_edge"], ref("radius_edge")
    dx = sorted(float(abs(s["kf2"]["kps"]["x"][j] - o["q12"]["u"][i]) + abs(s["kf2"]["kps"]["y"][j] - o["q12"]["v"][i])) for i, j in ((0, 0), (1, 1), (2, 2), (3, 3)))
    assert dx == [7.25, 7.25, 7.5, 7.5] and float(o["q12"]["radius"][0]) == 7.5
    s, o = SCENES["octaves"], ref("octaves")
    assert o["q12"]["level"][0] == 2 and sorted(s["kf2"]["kps"]["octave"].tolist()) == [0, 1, 2, 3] and o["infos"][0][0]["n_level"] == 2
    o = ref("th_high")
    assert sorted(it["best_dist"] for it in o["infos"][0]) == [0, 100, 101] and sorted(it["best_dist"] for it in o["infos"][1]) == [0, 100, 101]
    s, o = SCENES["equal_distances"], ref("equal_distances")
    assert o["match1"][0] == 1 and M.hamming(s["kf1"]["points"]["desc"][0], s["kf2"]["desc"][0]) == M.hamming(s["kf1"]["points"]["desc"][0], s["kf2"]["desc"][1]) == 10
    assert ref("window_65")["infos"][0][0]["n_window"] == 65 and ref("window_130")["infos"][0][0]["n_window"] == 130
    assert SCENES["empty_kf1"]["kf1"]["n"] == 0 and SCENES["empty_kf2"]["kf2"]["n"] == 0
    s = SCENES["full_records"]
    assert s["kf1"]["n"] == s["kf2"]["n"] == SC.NF and ref("full_records")["nfound"] == SC.NF
    o = ref("bookkeeping")
    assert (o["outcome"][0] == M.NO_AGREEMENT).sum() == 1 and SCENES["bookkeeping"]["match12"].max() == 100000


@pytest.mark.parametrize("name", GENERIC)
def test_generic_scenes_find_the_planted_correspondences(name):
    s, o = SCENES[name], ref(name)
    n = s["kf1"]["n"]
    assert np.array_equal(o["matches"], s["expect_matches"]), name
    assert o["nfound"] == n - int((R.matches_in(s["kf1"], s["match12"], s["inlier"]) >= 0).sum())


def as_oracle(s, o):
    """the scene in the form oracle/projection_oracle.py's _sim3_side takes"""
    cam = s["cam"]
    target = dict(bounds=cam["bounds"], scale=cam["scale"], logScale=float(np.log(np.float64(cam["scale"][1]))))
    sides = []
    for kf in (s["kf1"], s["kf2"]):
        pool = [dict(bad=bool(p["flags"] & 1), pos=np.array(p["pos"], F), minDist=p["min_distance"], maxDist=p["max_distance"], desc=p["desc"]) for p in kf["points"]]
        T = np.asarray(kf["pose"], F).reshape(3, 4)
        sides.append((list(range(kf["n"])), pool, T[:, :3], T[:, 3]))
    return target, sides


@pytest.mark.parametrize("name", EXACT + GENERIC)
def test_the_restatement_agrees_with_the_projection_oracle(name):
    """oracle/projection_oracle.py states the same two loops (its scalar * Mat product rounds in float, ours in double: equal at s = 1, where
    the exact scenes live, and within the recorded spread elsewhere; its PredictScale uses the double log: equal away from a level boundary)"""
    import projection_oracle as PO
    s, o = SCENES[name], ref(name)
    cam = s["cam"]
    target, sides = as_oracle(s, o)
    sR12, t12, sR21, t21 = R.similarity(s["sim3"])
    m_in = o["m_in"]
    done1 = [bool(m >= 0) for m in m_in]
    done2 = [any(m == j for m in m_in) for j in range(s["kf2"]["n"])]
    gold = json.load(open(NOISE_PATH))
    for (pts, pool, Ra, ta), done, Rb, tb, q in ((sides[0], done1, sR21, t21, o["q12"]), (sides[1], done2, sR12, t12, o["q21"])):
        with np.errstate(all="ignore"):
            g = PO._sim3_side(pts, done, pool, Ra, ta, Rb, tb, target, cam["fx"], cam["fy"], cam["cx"], cam["cy"], s["th"])
        assert np.array_equal(g["valid"], q["valid"]) and np.array_equal(g["level"], q["level"]) and np.array_equal(g["radius"], q["radius"]), name
        if s["kind"] == "exact":
            assert g["u"].tobytes() == q["u"].tobytes() and g["v"].tobytes() == q["v"].tobytes(), name
        elif len(pts):
            assert max(np.abs(g["u"] - q["u"]).max(), np.abs(g["v"] - q["v"]).max()) <= 64 * gold["spread_px"], name


def measure():
    """-> dict(spread_px, spread_m, margin_px, margin_m, n_queries) over the generic scenes"""
    sp_px = sp_m = 0.0; mg_px = mg_m = np.inf; nq = 0
    for name in GENERIC:
        s, a, b = SCENES[name], ref(name), ref(name, f64=True)
        cam = s["cam"]; bd = [float(x) for x in cam["bounds"]]
        for key in ("matches", "match1", "match2"):
            assert np.array_equal(a[key], b[key]), "%s: the f64 run gives another %s" % (name, key)
        for ia, ib, tgt in ((a["info1"], b["info1"], s["kf2"]), (a["info2"], b["info2"], s["kf1"])):
            for x, y in zip(ia, ib):
                assert x["stage"] == y["stage"] and x.get("lv") == y.get("lv"), name
                if "z" not in x:
                    continue
                sp_m = max(sp_m, abs(float(x["z"]) - float(y["z"]))); mg_m = min(mg_m, abs(float(y["z"])))
                if "u" not in x:
                    continue
                u, v = float(y["u"]), float(y["v"])
                sp_px = max(sp_px, abs(float(x["u"]) - u), abs(float(x["v"]) - v))
                mg_px = min(mg_px, abs(u - bd[0]), abs(u - bd[2]), abs(v - bd[1]), abs(v - bd[3]))
                if "dist" not in x:
                    continue
                d = float(y["dist"])
                sp_m = max(sp_m, abs(float(x["dist"]) - d))
                mg_m = min(mg_m, abs(d - float(y["min_d"])), abs(d - float(y["max_d"])))
                mg_m = min([mg_m] + [abs(d - float(x["max_distance"]) / float(D(cam["scale"][1])) ** k) for k in range(len(cam["scale"]) + 1)])
                if x["stage"] != R.VALID:
                    continue
                nq += 1
                r = float(F(F(s["th"]) * F(cam["scale"][x["lv"]])))
                kx = tgt["kps"]["x"].astype(D); ky = tgt["kps"]["y"].astype(D)
                mg_px = min(mg_px, float(np.abs(np.abs(kx - u) - r).min()), float(np.abs(np.abs(ky - v) - r).min()))
    return dict(spread_px=sp_px, spread_m=sp_m, margin_px=float(mg_px), margin_m=float(mg_m), n_queries=nq)


_MEASURED = []


def measured():
    if not _MEASURED:
        _MEASURED.append(measure())
    return _MEASURED[0]


def test_generic_scenes_keep_every_gate_64_spreads_from_its_threshold():
    m = measured()
    print(m)
    assert m["n_queries"] >= 150
    assert m["margin_px"] > 64 * m["spread_px"], "a projection sits %.3g px from a gate, the spread is %.3g px: move the scene" % (m["margin_px"], m["spread_px"])
    assert m["margin_m"] > 64 * m["spread_m"], "a depth or distance sits %.3g from a gate, the spread is %.3g: move the scene" % (m["margin_m"], m["spread_m"])


def test_noise_file_is_current():
    gold, m = json.load(open(NOISE_PATH)), measured()
    for k in ("spread_px", "spread_m"):
        assert m[k] <= 1.5 * gold[k] and gold[k] <= 1.5 * max(m[k], 1e-12), (k, m[k], gold[k])
    assert gold["n_queries"] == m["n_queries"]
    for k in ("margin_px", "margin_m"):
        assert abs(gold[k] - m[k]) <= 1e-3 * gold[k], (k, m[k], gold[k])


def test_bow_scenes_reach_every_gate():
    seen = set()
    for name in BOW:
        m12, nm, outcome, infos, (fv1, fv2) = bow_ref(name)
        seen |= set(int(x) for x in outcome)
        assert nm == int((m12 >= 0).sum())
    assert seen >= {M.NODE_NOT_SHARED, M.MAP_POINT, M.OCCUPIED, M.OVER_TH, M.RATIO_FAILED, M.ACCEPTED, M.ROT_REMOVED}, sorted(seen)
    m12, nm, outcome, infos, _ = bow_ref("bow_gates")
    d = sorted((it["best_dist"], int(o)) for it, o in zip(infos, outcome) if it.get("best_dist") in (49, 50))
    assert d == [(49, M.ACCEPTED), (50, M.OVER_TH)], d
    edge = sorted((it["best_dist"], it["best_dist2"], int(o)) for it, o in zip(infos, outcome) if it.get("best_dist") == 21)
    assert edge == [(21, 28, M.RATIO_FAILED), (21, 29, M.ACCEPTED)], edge
    s = BOW["bow_gates"]
    dead = int(np.nonzero(s["kf2"]["has"] == 0)[0][0])
    assert dead not in m12.tolist() and any(it.get("best_dist") == 10 and o == M.ACCEPTED for it, o in zip(infos, outcome))
    sizes = set()
    for name in ("bow_wide_kf1", "bow_wide_kf2"):
        fv1, fv2 = bow_ref(name)[4]
        sizes |= {(len(fv1[n]), len(fv2[n])) for n in fv1 if n in fv2}
    assert sizes == {(1, 64), (65, 130), (64, 1), (130, 65)}, sizes
    # the strict threshold and vbMatched2 matter: the misreadings mapping_ref can inject change the result of bow_gates
    for fault in M.FAULTS["bow"]:
        s = BOW["bow_gates"]
        fv1, fv2 = bow_ref("bow_gates")[4]
        g = M.search_by_bow_keyframes(s["kf1"]["kps"], s["kf1"]["desc"], s["kf1"]["has"], fv1, s["kf2"]["kps"], s["kf2"]["desc"], s["kf2"]["has"], fv2, SC.NN_RATIO, True, fault=fault)
        assert not np.array_equal(g[0], m12[:len(g[0])]), fault


if __name__ == "__main__":
    if "--write" in sys.argv:
        with open(NOISE_PATH, "w") as f:
            json.dump(measure(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", NOISE_PATH)
