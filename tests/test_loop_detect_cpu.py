"""The restatement of LoopClosing::DetectLoop (tests/loop_detect_ref.py) on the hand-made scenes of tests/loop_detect_scenes.py, no GPU:
every scene gives the result it was built for, the reference-shaped form (lists, sets, fields that outlive a query) equals the parallel
formulation the device runs, stale fields do not matter, and every injected fault changes at least one scene's result -- so the scenes
can tell the device from each of those mistakes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_detect_ref as L
import loop_detect_scenes as Z

F = np.float32
SCENES = Z.scenes()
GROUP_SCENES = Z.group_scenes()
CAND_FAULTS = ["keep_connected", "connected_max", "connected_neighbour", "ge_common", "gt_min_score", "stale_neighbour", "neighbour_min_score", "ge_retain",
               "no_dedupe", "index_order", "visible_inclusive", "ignore_live", "bad_connected", "min_visible", "min_from_zero", "reverse"]
GROUP_FAULTS = ["flagged_blocks_enough", "push_every", "gt_th", "no_self", "keep_on_empty", "last_first"]


def answer(results):
    """everything the device writes for the queries, bits included"""
    out = []
    for r in results:
        if r is None or isinstance(r, int):
            out.append(r)
        else:
            out.append((F(r["min_score"]).tobytes(), list(r["cand"]), r["common"].tobytes(), r["scores"].tobytes()))
    return out


def group_answer(res):
    groups, out = res
    return [(sorted(g), c) for g, c in groups], {k: v.tobytes() for k, v in out.items()}


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scenes_give_what_they_were_built_for(sc):
    res = Z.run(sc)
    for i, r in enumerate(res):
        if sc["cand"] is not None:
            want = sc["cand"][i]
            assert (r is None or isinstance(r, int)) if want is None else r["cand"] == want, (sc["name"], i, r)
        if sc["min_score"] is not None and sc["min_score"][i] is not None:
            assert F(r["min_score"]).tobytes() == F(sc["min_score"][i]).tobytes(), (sc["name"], i, r["min_score"])
    if "scored" in sc:                                         # the threshold scene: at minCommonWords not scored, one above scored
        for (k0, k2), r in zip(sc["scored"], res):
            bits = r["scores"].view(np.uint32)
            assert bits[k0] != L.NO_SCORE_BITS and bits[k0 + 1] == L.NO_SCORE_BITS and bits[k2] != L.NO_SCORE_BITS and r["common"][k0 + 1] > 0
            assert r["common"][k0 + 3] == 0, "the connected keyframe shares a word and counts none"


@pytest.mark.parametrize("sc", SCENES + [Z.sizes_scene()] + [Z.random_scene(s) for s in range(40)], ids=lambda s: s["name"])
def test_reference_form_equals_the_parallel_formulation(sc):
    """... of both calls, and fields preset to anything (mnLoopQuery equal to nothing the call uses) change nothing"""
    ref, short = Z.run(sc), Z.run(sc, shortcut=True)
    assert answer(ref) == answer(short)
    n = len(sc["kf_vecs"])
    rng = np.random.default_rng(3)
    stale = dict(sc, fields=dict(query=rng.integers(0, 50, n).tolist(), words=rng.integers(0, 99, n).tolist(), score=rng.uniform(0, 9, n)))
    assert answer(Z.run(stale)) == answer(ref)
    assert group_answer(Z.run_groups(sc, ref)) == group_answer(Z.run_groups(sc, ref, step=L.consistency_step_shortcut))


@pytest.mark.parametrize("fault", CAND_FAULTS)
def test_every_candidate_fault_changes_a_scene(fault):
    seen = [sc["name"] for sc in SCENES if answer(Z.run(sc, fault)) != answer(Z.run(sc))]
    assert seen, fault
    print(fault, "->", seen)


def test_two_gates_no_scene_can_see():
    """(int)(maxCommonWords * 0.8f) against a double 0.8: the products differ first beyond 2^23 words and a vector holds at most 4096, so
    the property is checked over the whole range.  bestAccScore starting at minScore against 0: every accScore is an entry's score plus
    scores that are >= 0, and an entry's score is >= minScore, so the running maximum passes the start at the first entry either way."""
    for n in range(0, 4097):
        assert L.R.min_common_words(n) == L.R.min_common_words(n, "double08") == (4 * n) // 5
    for sc in SCENES + [Z.random_scene(s) for s in range(40)]:
        assert answer(Z.run(sc, "double08")) == answer(Z.run(sc)) == answer(Z.run(sc, "best_from_zero"))


def test_a_neighbour_below_min_score_is_accumulated():
    sc = [s for s in SCENES if s["name"] == "empty_row"][0]
    fields = L.Fields(3)
    r = L.detect(fields, sc["kf_vecs"], sc["neigh"], sc["live"], sc["conn"], 2, 2)
    assert r["scores"][1] == F(0.875) and r["scores"][1] < r["min_score"] == F(1) and F(r["scores"][0] + r["scores"][1]) == sc["acc"][1] and r["cand"] == [0]


@pytest.mark.parametrize("sc", GROUP_SCENES, ids=[s["name"] for s in GROUP_SCENES])
def test_group_scenes_give_what_they_were_built_for(sc):
    groups, out = Z.run_groups(sc, sc["lists"])
    if sc["want_groups"] is not None:
        assert [(sorted(g), c) for g, c in groups] == [(sorted(g), c) for g, c in sc["want_groups"]]
    for i, want in enumerate(sc["want_enough"]):
        assert out["enough"][i, :out["nenough"][i]].tolist() == want and (out["enough"][i, out["nenough"][i]:] == -1).all()
    assert group_answer((groups, out)) == group_answer(Z.run_groups(sc, sc["lists"], step=L.consistency_step_shortcut))
    over = "overflow" in sc["name"]
    assert out["status"].any() == over
    if over:
        first = int(np.argmax(out["status"]))
        assert out["status"][first:].all() and not out["nenough"][first:].any() and not out["select"][first:].any()


def test_pairs_are_current_keyframe_then_candidate_and_need_both_records():
    sc = [s for s in GROUP_SCENES if s["name"] == "four_in_sequence"][0]
    _, out = Z.run_groups(sc, sc["lists"])
    assert out["pairs"][3, 0].tolist() == [28 + 2, 4 + 2] and out["select"][3].tolist() == [1, 0, 0, 0]
    sc2 = dict(sc, kf_record=np.where(np.arange(30) == 4, -1, sc["kf_record"]))
    _, out = Z.run_groups(sc2, sc["lists"])
    assert out["enough"][3, 0] == 4 and out["pairs"][3, 0].tolist() == [-1, -1] and not out["select"][3].any()


def test_four_queries_in_one_call_equal_four_calls():
    for sc in GROUP_SCENES + [s for s in SCENES if s["name"] in ("batch", "visible")]:
        lists = sc["lists"] if "lists" in sc else Z.run(sc)
        whole = Z.run_groups(sc, lists)
        groups = list(sc["groups"]); parts = []
        sticky = False
        for i in range(len(sc["queries"])):
            one = dict(sc, queries=sc["queries"][i:i + 1], groups=groups)
            groups, out = Z.run_groups(one, lists[i:i + 1])
            sticky = sticky or bool(out["status"][0])
            parts.append(out)
            if sticky:
                break                                          # the status of a call is sticky inside the call only: compare up to there
        n = len(parts)
        for k in whole[1]:
            assert np.concatenate([p[k] for p in parts]).tobytes() == whole[1][k][:n].tobytes(), (sc["name"], k)
        if not sticky:
            assert [(sorted(g), c) for g, c in groups] == [(sorted(g), c) for g, c in whole[0]]


@pytest.mark.parametrize("fault", GROUP_FAULTS)
def test_every_group_fault_changes_a_scene(fault):
    seen = [sc["name"] for sc in GROUP_SCENES if group_answer(Z.run_groups(sc, sc["lists"], fault=fault)) != group_answer(Z.run_groups(sc, sc["lists"]))]
    assert seen, fault
    print(fault, "->", seen)


def test_state_packing_clears_the_rows_beyond_the_count():
    member, size, count, n = L.pack_state([({5, 2}, 3), ({9}, 0)], 4, 3)
    assert member.tolist() == [[2, 5, -1], [9, -1, -1], [-1, -1, -1], [-1, -1, -1]] and size.tolist() == [2, 1, 0, 0] and count.tolist() == [3, 0, 0, 0] and n.tolist() == [2]
