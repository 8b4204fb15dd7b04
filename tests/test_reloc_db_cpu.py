"""The restatement of DetectRelocalizationCandidates (tests/reloc_db_ref.py) on the hand-made scenes (tests/reloc_db_scenes.py), without
a GPU: every scene reaches the exit it was built for, the (smallest shared word, keyframe index) ordering the device uses equals the
inverted-file ordering, the scenes' descriptors reach the words they name, and each injected fault changes the answer of a scene."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O
import reloc_db_ref as R
import reloc_db_scenes as D

F = np.float32
SCENES = D.scenes()


def answer(res):
    return (tuple(res["cand"]), res["scores"].tobytes(), res["common"].tobytes())


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scene_reaches_the_exit_it_was_built_for(sc):
    for f, k, stage in sc["expect"]:
        got = int(D.run(sc, f)["stage"][k])
        assert got == stage, "%s frame %d keyframe %d: %s, built for %s" % (sc["name"], f, k, R.STAGE_NAMES[got], R.STAGE_NAMES[stage])
    for f, k in sc.get("scored", []):
        assert int(D.run(sc, f)["stage"][k]) >= R.DROPPED
    if sc["cand"] is not None:
        for f, want in enumerate(sc["cand"]):
            assert D.run(sc, f)["cand"] == want, (sc["name"], f)


def test_every_exit_is_reached_by_some_scene():
    seen = set()
    for sc in SCENES:
        for f in range(len(sc["frame_vecs"])):
            seen |= set(int(s) for s in D.run(sc, f)["stage"])
    assert seen == set(range(6))
    wide = SCENES[-1]
    assert len(wide["kf_vecs"]) > 64 and max(len(v) for v in wide["kf_vecs"]) > 64 and max(len(v) for v in wide["frame_vecs"]) > 64
    assert (wide["neigh"][0] >= 0).all() and (wide["live"] == 0).any() and (wide["kf_record"] < 0).any()
    order = [s for s in SCENES if s["name"] == "order_max1"][0]
    assert len(D.run(order, 0)["cand"]) > order["max_cand"] and D.run(order, 0)["cand"] != sorted(D.run(order, 0)["cand"])


def test_descriptors_reach_the_words_the_scenes_name():
    """the C oracle's transform on the descriptors of a word list gives those word ids, and BowVector accumulation on its output is
    the scene's vector: a word that k keypoints reach holds k successive additions"""
    for sc in SCENES:
        for words in sc["kf_words"] + sc["frame_words"]:
            if not words:
                continue
            wid, _, wt = O.bow_transform(sc["tree"], D.descriptors(sc["tree"], words, 3), 0)
            assert wid.tolist() == list(words)
            assert R.bow_vector(wid, wt) == D.vec(sc["tree"], words)
    t = D.TREE3; u = D.usable_words(t)
    w = D.weights_of(t, [u[21]])[0]
    v = dict(R.bow_vector([u[21]] * 3 + [u[4]], D.weights_of(t, [u[21]] * 3 + [u[4]])))
    w4 = D.weights_of(t, [u[4]])[0]
    assert v[u[21]] == (0.0 + w + w + w) / (w4 + (0.0 + w + w + w)) and R.bow_vector([D.stopped_word(t)] * 4, [0.0] * 4) == []


def test_shortcut_order_equals_the_inverted_file_order():
    for sc in SCENES:
        for f in range(len(sc["frame_vecs"])):
            assert R.detect_shortcut(sc["kf_vecs"], sc["neigh"], sc["frame_vecs"][f], sc["live"], sc["reloc"]) == D.run(sc, f)["cand"], (sc["name"], f)
    many = reordered = 0
    for seed in range(300):
        rs = D.random_scene(seed)
        for fv in rs["frame_vecs"]:
            ref = R.detect(rs["kf_vecs"], rs["neigh"], fv, rs["live"], rs["reloc"])["cand"]
            assert R.detect_shortcut(rs["kf_vecs"], rs["neigh"], fv, rs["live"], rs["reloc"]) == ref, seed
            many += len(ref) > 1; reordered += ref != sorted(ref)
    assert many >= 100 and reordered >= 30                                # the random set is about the order: enough queries must have one


@pytest.mark.parametrize("fault", ["reverse", "ge_common", "ge_best", "ge_retain", "ignore_reloc"])
def test_injected_fault_changes_the_answer_of_a_scene(fault):
    seen = [(sc["name"], f) for sc in SCENES for f in range(len(sc["frame_vecs"])) if answer(D.run(sc, f)) != answer(D.run(sc, f, fault))]
    assert seen, "no scene sees the fault %r" % fault


def test_the_float_product_of_the_threshold_cannot_be_told_from_the_double_one():
    """(int)(maxCommonWords * 0.8f) against (int)(maxCommonWords * 0.8): 0.8f and 0.8 both lie above 4/5, so for a multiple of 5 both
    products lie at or just above the integer and truncate to it, and for every other count the fraction is at least 0.2 -- far from the
    2^-24 relative distance between the two products.  They differ first beyond 2^23 common words; a vector holds at most 4096.  So no
    scene can see this fault: the property is checked over the whole range instead, and the scenes pin the values at 4, 5, 10 and 15."""
    for n in range(0, 4097):
        assert R.min_common_words(n) == R.min_common_words(n, "double08") == (4 * n) // 5
    for sc in SCENES:
        for f in range(len(sc["frame_vecs"])):
            assert answer(D.run(sc, f)) == answer(D.run(sc, f, "double08"))


def test_lookup_size_cases_are_not_vacuous():
    """the hand-packed databases of tests/test_gpu_bow_sizes.py under the restatement alone: every (frame, keyframe) word-count pair is
    met and a scored keyframe's shared words lie in two 64-word rounds of its list"""
    import test_gpu_bow_sizes as Z
    for nK in Z.N_KEYFRAMES:
        Z.assert_lookup_not_vacuous(nK)
