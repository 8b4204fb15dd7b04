"""The sizes at which the text the BoW units share (iv_slam_amd/csrc/ivf_bow.h: sort_keys_and_runs, sorted_find; ivf_track_db.hip:
shared_word_rounds) changes shape.  Every comparison is bit for bit.

Sort and scan.  A tracker of 520 features (no power of two, no multiple of 16: the last descent workgroup is partial, the key array is
sized for 1024) and records of n in SIZES keypoints: the network runs on 256, 512 and 1024 keys, a thread owns 1, 2 and 4 sorted keys,
runs of equal ids cross a thread's slice.  Two ragged trees with stopped words and early leaves: SMALL (about 100 words: many keypoints
per word) and LARGE (more than 500 words: the norm of a 513-keypoint record takes more than one 64-lane round).  Record K_n holds the
first n of 520 random descriptors, record F_n the same n descriptors with FLIPS bits flipped each, in another order.
  * ivf_tracker_bow_vectors of all 26 records against the per-call ORBVocabulary.transform and tests/reloc_db_ref.py;
  * ivf_tracker_search_by_bow of every (K_a, F_b) against the C oracle's SearchByBoW and the per-call ORBmatcher.SearchByBoW, with the
    nodes one level below the root and with levelsup = depth (every feature in node 0: one run of length n).
Lookup.  ivf_tracker_reloc_candidates at 256 features on hand-packed vectors: frames of 0, 1, 63, 64, 65 words against keyframes of 0, 1,
63, 64, 65, 129 words in databases of 1, 31, 32, 33, 65 keyframes (the 32-keyframe tile, the four-wave stride), the shared words at the
first, the last and the 64th / 65th place of a keyframe's list; all six outputs against tests/reloc_db_ref.py.

What makes the inputs not vacuous is computed with the oracle alone (sweep_facts, pair_oracle, lookup_facts) and asserted both here and,
without a device, in tests/test_track_bow_cpu.py and tests/test_reloc_db_cpu.py."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import reloc_db_ref as R
import reloc_db_scenes as D
import track_bow_scenes as S
from test_gpu_track import iv  # noqa: F401  (the module fixture)

F = np.float32
NF = 520
SIZES = (0, 1, 2, 15, 16, 17, 255, 256, 257, 511, 512, 513, 520)
FLIPS, SEED = 3, 41                                  # bits flipped per frame descriptor; the seed of descriptors, order and angles
TREES = {"small": dict(k=5, depth=3, seed=7, early_leaf_frac=0.1, stop_frac=0.1),
         "large": dict(k=10, depth=3, seed=9, early_leaf_frac=0.05, stop_frac=0.05)}


@functools.lru_cache(maxsize=None)
def tree_of(name):
    return O.make_vocabulary(**TREES[name])


@functools.lru_cache(maxsize=None)
def sides():
    """-> ({n: keyframe side}, {n: frame side}): dict(kps, desc[, has]) as tests/track_bow_scenes.py's scenes hold them"""
    rng = np.random.default_rng(SEED)
    desc = rng.integers(0, 256, (NF, 32), dtype=np.uint8)
    twin = desc.copy()
    for i in range(NF):
        for b in rng.permutation(256)[:FLIPS]:
            twin[i, b // 8] ^= np.uint8(1 << (b % 8))
    angle = rng.uniform(0.0, 359.0, NF).astype(F)
    xy = np.stack([rng.uniform(20, S.W - 20, NF), rng.uniform(20, S.H - 20, NF)], 1).astype(F)

    def side(idx, d, with_has):
        kp = np.zeros(len(idx), S.KP_DTYPE)
        kp["x"] = xy[idx, 0]; kp["y"] = xy[idx, 1]; kp["size"] = 31; kp["angle"] = angle[idx]
        out = dict(kps=kp, desc=np.ascontiguousarray(d[idx]).reshape(len(idx), 32))
        if with_has:
            out["has"] = (idx % 7 != 3).astype(np.uint8)                                 # every seventh keyframe keypoint holds no map point
        return out
    kf = {n: side(np.arange(n), desc, True) for n in SIZES}
    f = {n: side(rng.permutation(n), twin, False) for n in SIZES}
    return kf, f


def records():
    """-> the 26 gather records: K_n at SIZES.index(n), F_n at 13 + SIZES.index(n)"""
    kf, f = sides()
    tree = tree_of("small")                                                              # records_of reads the two sides only
    recs = [S.records_of(dict(tree=tree, kf=kf[n], f=f[n])) for n in SIZES]
    return [r[0] for r in recs] + [r[1] for r in recs]


@functools.lru_cache(maxsize=None)
def sweep_facts(name):
    """the oracle's transform of every record on the tree -> (per record (word ids, weights), most words of a record, most keypoints on
    one live word, keypoints lost to stopped words)"""
    tree = tree_of(name)
    per, most_words, most_on_word, lost = [], 0, 0, 0
    for rec in records():
        if len(rec["desc"]) == 0:
            per.append((np.zeros(0, np.int32), np.zeros(0, np.float64))); continue
        wid, _, wt = O.bow_transform(tree, rec["desc"], 0)
        live = wid[wt > 0]
        most_words = max(most_words, len(set(live.tolist())))
        most_on_word = max(most_on_word, int(np.bincount(live).max()) if len(live) else 0)
        lost += int((wt <= 0).sum())
        per.append((wid, wt))
    return per, most_words, most_on_word, lost


def assert_sweep_not_vacuous(name):
    _, most_words, most_on_word, lost = sweep_facts(name)
    assert most_words > 64, "%s: no record with more than 64 words (the norm's second round)" % name
    assert most_on_word >= 5, "%s: no word with 5 keypoints (a run longer than a thread's slice of 4)" % name
    assert lost > 0, "%s: no keypoint on a stopped word" % name


def levelsup_of(name, kind):
    depth = TREES[name]["depth"]
    return depth - 1 if kind == "level1" else depth


def scene_of(name, a, b, levelsup):
    kf, f = sides()
    return dict(name="K%d x F%d" % (a, b), tree=tree_of(name), levelsup=levelsup, kf=kf[a], f=f[b])


@functools.lru_cache(maxsize=None)
def pair_oracle(name, kind):
    """the C oracle's SearchByBoW of every (K_a, F_b) -> {(a, b): (assignment, nmatches)}"""
    ls = levelsup_of(name, kind)
    return {(a, b): S.oracle(O, scene_of(name, a, b, ls), ls, 0.7, True) for a in SIZES for b in SIZES}


def assert_pairs_not_vacuous(name, kind):
    for (a, b), (_, nm) in pair_oracle(name, kind).items():
        assert nm >= 1 or min(a, b) < 16, "%s %s: K%d x F%d has no match" % (name, kind, a, b)
        assert nm == 0 or min(a, b) > 0


# ---- sort and scan: mBowVec ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TREES))
def test_bow_vectors_at_every_sort_size(iv, name):
    from test_gpu_reloc_db import device_bow_vectors
    from test_gpu_track_bow import make_tracker, vocabulary
    assert_sweep_not_vacuous(name)
    per = sweep_facts(name)[0]
    recs = records()
    V = vocabulary(iv, tree_of(name))
    tr = make_tracker(iv, NF, 2)
    frames = list(range(len(recs)))
    word, value, cnt = device_bow_vectors(iv, tr, V, recs, frames, NF)
    for s, rec in enumerate(recs):
        n_kp = len(rec["desc"]); n = int(cnt[s])
        bow = V.transform(rec["desc"], 0)[0] if n_kp else {}
        want = R.bow_vector(*per[s])
        what = "%s record %d (%d keypoints)" % (name, s, n_kp)
        assert n == len(bow) == len(want), what
        assert word[s, :n].tolist() == sorted(bow) == [w for w, _ in want] and (word[s, n:] == -1).all() and not value[s, n:].any(), what
        assert value[s, :n].tobytes() == np.array([bow[w] for w in sorted(bow)], np.float64).tobytes(), what + ": per-call path"
        assert value[s, :n].tobytes() == np.array([x for _, x in want], np.float64).tobytes(), what + ": restatement"
    again = device_bow_vectors(iv, tr, V, recs, frames, NF)
    assert again[0].tobytes() == word.tobytes() and again[1].tobytes() == value.tobytes() and again[2].tobytes() == cnt.tobytes()


# ---- sort and scan: mFeatVec, and the node merge's lookup ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["level1", "root"])
@pytest.mark.parametrize("name", sorted(TREES))
def test_search_by_bow_at_every_sort_size(iv, name, kind):
    from test_gpu_track_bow import make_tracker, run_bow, vocabulary
    assert_pairs_not_vacuous(name, kind)
    want = pair_oracle(name, kind)
    ls = levelsup_of(name, kind)
    kf, f = sides()
    recs = records()
    pairs = [(SIZES.index(a), len(SIZES) + SIZES.index(b)) for a in SIZES for b in SIZES]
    V = vocabulary(iv, tree_of(name))
    tr = make_tracker(iv, NF, len(pairs))
    assign, nm = run_bow(iv, tr, V, ls, recs, pairs, NF)
    m = iv.ORBmatcher(0.7, True)
    fv = {(side, n): V.transform(d[n]["desc"], ls)[1] for side, d in (("kf", kf), ("f", f)) for n in SIZES if n}
    for k, (a, b) in enumerate((a, b) for a in SIZES for b in SIZES):
        om, onm = want[(a, b)]
        what = "%s %s K%d x F%d" % (name, kind, a, b)
        assert nm[k] == onm, "%s: nmatches %d, oracle %d" % (what, nm[k], onm)
        assert np.array_equal(assign[k, :b], om) and (assign[k, b:] == -1).all(), what
        if a and b:
            gm, gn = m.SearchByBoW(kf[a]["kps"], kf[a]["desc"], kf[a]["has"], fv[("kf", a)], f[b]["kps"], f[b]["desc"], fv[("f", b)])
            assert gn == nm[k] and np.array_equal(gm, assign[k, :b]), what + ": per-call path"
    again = run_bow(iv, tr, V, ls, recs, pairs, NF)
    assert again[0].tobytes() == assign.tobytes() and again[1].tobytes() == nm.tobytes()


# ---- lookup chunks and keyframe tiles -----------------------------------------------------------------------------------------------
LOOKUP_NF = 256
FRAME_WORDS = (0, 1, 63, 64, 65)
KF_WORDS = (65, 129, 64, 63, 1, 0)                   # keyframe k holds KF_WORDS[k % 6] words
N_KEYFRAMES = (1, 31, 32, 33, 65)
MASTER = [1001 + 2000 * i for i in range(65)]        # the frames' words (odd): the frame of c words holds the first c; a keyframe's own are even


def kf_shared_places(k, ck):
    """[(place in the keyframe's list, index into MASTER)] of the words keyframe k shares with the frames"""
    mode = (k // 6 + k) % 4
    want = ([(63, 0), (64, 1)], [(0, 0)], [(ck - 1, 62)], [(0, 0), (ck - 1, 64)])[mode]   # 64th / 65th place, first, last, both ends
    got = sorted(set((q, i) for q, i in want if 0 <= q < ck))
    if len(got) == 2 and got[0][0] == got[1][0]:
        got = got[:1]
    return got or ([(ck - 1, 0)] if ck else [])


@functools.lru_cache(maxsize=None)
def lookup_case(nK):
    """-> the database and the five frames in the form of tests/reloc_db_scenes.py's scenes"""
    rng = np.random.default_rng(100 + nK)

    def vec(words):
        v = rng.uniform(0.1, 1.0, len(words)); v /= v.sum() if len(words) else 1.0
        return [(int(w), float(x)) for w, x in zip(words, v)]
    kf_vecs = []
    for k in range(nK):
        ck = KF_WORDS[k % 6]
        shared = dict(kf_shared_places(k, ck))
        words, cur, step = [], 2 * (k % 7) - 2, 2 * (1 + k % 5)
        for q in range(ck):
            cur = MASTER[shared[q]] if q in shared else cur + step - (cur + step) % 2
            assert not words or cur > words[-1]
            words.append(cur)
        kf_vecs.append(vec(words))
    live = np.array([0 if k % 11 == 5 else 1 for k in range(nK)], np.uint8)
    return dict(name="lookup_%d" % nK, tree=D.TREE3, nf=LOOKUP_NF, kf_vecs=kf_vecs, frame_vecs=[vec(MASTER[:c]) for c in FRAME_WORDS],
                neigh=rng.integers(-1, nK, (nK, R.NEIGH)).astype(np.int32), live=live, reloc=rng.uniform(0.0, 0.05, nK).astype(F),
                kf_record=np.where(np.arange(nK) % 9 == 4, -1, np.arange(nK)).astype(np.int32), frame_record=np.arange(len(FRAME_WORDS), dtype=np.int32) + 100,
                max_cand=4)


def lookup_facts(nK):
    """with the restatement alone: (a scored keyframe whose shared words lie in two 64-word rounds of its list, the word counts met)"""
    sc = lookup_case(nK)
    two_rounds, counts = False, set()
    for fv in sc["frame_vecs"]:
        res = R.detect(sc["kf_vecs"], sc["neigh"], fv, sc["live"], sc["reloc"])
        fw = set(w for w, _ in fv)
        for k, vec in enumerate(sc["kf_vecs"]):
            at = [q for q, (w, _) in enumerate(vec) if w in fw]
            assert res["common"][k] == (len(at) if sc["live"][k] else 0)
            counts.add((len(fv), len(vec)))
            if not np.isnan(res["scores"][k]) and at and at[0] < 64 <= at[-1]:
                two_rounds = True
    return two_rounds, counts


def assert_lookup_not_vacuous(nK):
    two_rounds, counts = lookup_facts(nK)
    assert two_rounds, "%d keyframes: no scored keyframe whose shared words span two 64-word rounds" % nK
    assert counts >= set((cf, ck) for cf in FRAME_WORDS for ck in KF_WORDS[:min(nK, 6)])


@pytest.mark.gpu
@pytest.mark.parametrize("nK", N_KEYFRAMES)
def test_reloc_candidates_at_every_lookup_size(iv, nK):
    from test_gpu_reloc_db import device_candidates, expected
    from test_gpu_track_bow import make_tracker, vocabulary
    assert_lookup_not_vacuous(nK)
    sc = lookup_case(nK)
    V = vocabulary(iv, sc["tree"])
    tr = make_tracker(iv, LOOKUP_NF, 2)
    got = device_candidates(iv, tr, V, sc, sc["frame_vecs"])
    want = expected(sc, sc["frame_vecs"])
    for key in ("ncand", "cand", "pairs", "select", "common", "scores"):
        assert got[key].tobytes() == want[key].tobytes(), "%d keyframes, %s:\n%r\n%r" % (nK, key, got[key], want[key])
    again = device_candidates(iv, tr, V, sc, sc["frame_vecs"])
    for key in got:
        assert again[key].tobytes() == got[key].tobytes(), key
