"""loop_detect_scenes.py -- hand-made scenes for ivf_tracker_loop_candidates / ivf_tracker_loop_consistency (test infrastructure only),
shared by tests/test_loop_detect_cpu.py (the restatement of tests/loop_detect_ref.py gives the result each scene was built for, its
shortcut form agrees, injected faults are seen) and tests/test_gpu_loop_detect.py (the device against the restatement).

A candidate scene is a keyframe database of vectors [(word, value)], its neighbour and connected tables, and queries (keyframe, visible,
select) that the restatement runs in order on one Fields object.  Most vectors are uniform over 8 (or 2, 4) words, so every score is a
dyadic number that float holds exactly: score = (common words) / 8 for two 8-word vectors.  `cand` / `min_score` give, per query, what
the scene was built for.  A group scene is a connected table, a start state, and queries with their candidate lists."""
import numpy as np

import loop_detect_ref as L
import reloc_db_scenes as D

F = np.float32
W8 = list(range(8))                                            # the query's words in most scenes


def uv(words):
    return [(int(w), 1.0 / len(words)) for w in sorted(words)]


def scene(name, kf, queries, neigh=None, conn=None, live=None, kf_record=None, max_cand=4, nf=64, fields=None, cand=None, min_score=None, th=3,
          group_cap=8, member_cap=8):
    n = len(kf)
    for v in kf:
        assert len(v) <= nf and [w for w, _ in v] == sorted({w for w, _ in v})
    return dict(name=name, nf=nf, kf_vecs=[list(v) for v in kf], neigh=D.neigh_rows(neigh or {}, n), conn=[list((conn or {}).get(k, [])) for k in range(n)],
                live=None if live is None else np.array(live, np.uint8), kf_record=np.arange(n, dtype=np.int32) + 3 if kf_record is None else np.array(kf_record, np.int32),
                queries=[tuple(q) for q in queries], max_cand=max_cand, fields=fields or {}, cand=cand, min_score=min_score, th=th, group_cap=group_cap,
                member_cap=member_cap, groups=[])


def csr(conn):
    start = np.zeros(len(conn) + 1, np.int32)
    for k, r in enumerate(conn):
        start[k + 1] = start[k] + len(r)
    return start, np.array([c for r in conn for c in r], np.int32)


def run(sc, fault=None, shortcut=False):
    """the scene's queries in order on one Fields object -> per query a result dict, None (not selected) or -1 (no such keyframe)"""
    n = len(sc["kf_vecs"])
    fields = L.Fields(n, **sc["fields"])
    out = []
    for q, visible, select in sc["queries"]:
        if not select:
            out.append(None)
        elif not 0 <= q < n:
            out.append(-1)
        elif shortcut:
            out.append(L.detect_shortcut(sc["kf_vecs"], sc["neigh"], sc["live"], sc["conn"], q, visible))
        else:
            out.append(L.detect(fields, sc["kf_vecs"], sc["neigh"], sc["live"], sc["conn"], q, visible, fault))
    return out


def run_groups(sc, results, fault=None, step=L.consistency_step):
    """the consistency call over the scene's queries with the candidates `results` (of run(), or lists) -> (groups, outputs)"""
    qs = [(q, None if (r is None or isinstance(r, int)) else (r["cand"] if isinstance(r, dict) else r)) for (q, _, _), r in zip(sc["queries"], results)]
    return L.consistency(list(sc["groups"]), qs, sc["conn"], len(sc["conn"]), sc["kf_record"], sc["th"], sc["max_cand"], sc["group_cap"], sc["member_cap"],
                         step=step, fault=fault)


# ---- candidates --------------------------------------------------------------------------------------------------------------------
def connected_scene():
    """keyframe 0 equals the query (score 1, 8 shared words) and is connected: it is no candidate, does not set maxCommonWords (6, from
    keyframe 1: minCommonWords 4, so keyframe 3 with 5 words is scored; with 8 it would be 6 and nobody would be) and is not accumulated
    as keyframe 1's neighbour.  Keyframe 2, connected, sets minScore = 0.5."""
    kf = [uv(W8), uv(W8[:6] + [20, 21]), uv(W8[:4] + [30, 31, 32, 33]), uv(W8[:5] + [40, 41, 42]), uv(W8)]
    return scene("connected", kf, [(4, 4, 1)], neigh={1: [0]}, conn={4: [0, 2]}, cand=[[1, 3]], min_score=[0.5])


def threshold_scene():
    """maxCommonWords of 4, 5, 10 and 15 -> minCommonWords 3, 4, 8, 12: a keyframe at exactly minCommonWords is not scored, one at
    minCommonWords + 1 is.  Every query has a connected keyframe that shares one word, so that minScore is small."""
    kf = []; queries = []; conn = {}; scored = []
    base = 0
    for n, mn in ((4, 3), (5, 4), (10, 8), (15, 12)):
        assert L.R.min_common_words(n) == mn
        block = list(range(base, base + n)); spare = list(range(base + 100, base + 110)); base += n
        k0 = len(kf)
        kf += [uv(block), uv(block[:mn] + spare[:3]), uv(block[:mn + 1] + spare[3:5]), uv(block[:1] + spare[5:8]), uv(block)]
        conn[k0 + 4] = [k0 + 3]
        queries.append((k0 + 4, k0 + 4, 1))
        scored.append((k0, k0 + 2))
    sc = scene("threshold", kf, queries, conn=conn, nf=256)
    sc["scored"] = scored
    return sc


def min_score_scene():
    """si == minScore exactly and one ulp below.  Connected keyframe 0 gives minScore 0.5; keyframe 1 holds the same vector (si = 0.5: an
    entry, >=); keyframe 2 scores 0.5 - 2^-25, the float below (scored, no entry, but accumulated as keyframe 1's neighbour: accScore
    rounds to 1.0); keyframe 3 scores 0.5 and is dropped by 0.75 * 1.0 -- it would be retained if keyframe 2 did not count."""
    a = 0.5 - 2.0 ** -25
    kf = [[(0, 0.5), (9, 0.5)], [(0, 0.5), (9, 0.5)], [(0, a), (10, 1.0 - a)], [(0, 0.5), (12, 0.5)], [(0, 0.5), (1, 0.5)]]
    assert F(L.R.l1_score(kf[4], kf[2])) == np.nextafter(F(0.5), F(0)) and F(L.R.l1_score(kf[4], kf[1])) == F(0.5)
    return scene("min_score", kf, [(4, 4, 1)], neigh={1: [2]}, conn={4: [0]}, cand=[[1]], min_score=[0.5])


def stale_scene():
    """keyframe 0 (6 shared words, scored) lists keyframe 1, which shares one word (0 < mnLoopWords <= minCommonWords): it adds nothing,
    whatever mLoopScore it holds from another query (5.0 here) -- relocalization's rule would add it and move pBestKF"""
    kf = [uv(W8[:6] + [20, 21]), uv([0, 30, 31, 32, 33, 34, 35, 36]), uv(W8[:4] + [40, 41, 42, 43]), uv(W8)]
    return scene("stale", kf, [(3, 3, 1)], neigh={0: [1]}, conn={3: [2]}, fields=dict(score=[0, 5.0, 0, 0], query=[7, 7, 7, 7], words=[9, 9, 9, 9]),
                 cand=[[0]], min_score=[0.5])


def retain_scene():
    """accScore == 0.75f * bestAccScore exactly is dropped.  Keyframes 1 and 2 score 0.5 each, 1 lists 2: accScore 1.0; keyframe 3 scores
    0.75 alone.  All share two words (maxCommonWords 2: minCommonWords 1)."""
    kf = [[(0, 0.5), (25, 0.5)], [(1, 0.25), (2, 0.25), (23, 0.5)], [(1, 0.25), (2, 0.25), (24, 0.5)], [(0, 0.5), (1, 0.25), (22, 0.25)],
          [(0, 0.5), (1, 0.25), (2, 0.25)]]
    assert F(0.75) * F(1.0) == F(0.75)
    return scene("retain", kf, [(4, 4, 1)], neigh={1: [2]}, conn={4: [0]}, cand=[[1]], min_score=[0.5])


def order_scene(max_cand):
    """list order = (smallest shared word, keyframe index), not index order: keyframe 0 first shares word 2, keyframe 1 word 0,
    keyframe 2 word 1, keyframe 3 word 0.  With max_candidates 2 the list is longer than the row."""
    kf = [uv(W8[2:] + [20, 21]), uv(W8[:6] + [22, 23]), uv(W8[1:7] + [24, 25]), uv(W8[:7] + [26]), uv(W8[:4] + [30, 31, 32, 33]), uv(W8)]
    return scene("order_max%d" % max_cand, kf, [(5, 5, 1)], conn={5: [4]}, max_cand=max_cand, cand=[[1, 3, 2, 0]], min_score=[0.5])


def dedupe_scene():
    """two retained entries name one pBestKF: keyframe 2 lists keyframe 3 (greater score: pBestKF moves) and keyframe 3, whose own entry
    lists keyframe 1, keeps itself.  Keyframe 3 comes out once, at its own entry's place."""
    sc = order_scene(4)
    sc.update(name="dedupe", neigh=D.neigh_rows({2: [3], 3: [1]}, 6), cand=[[3]])
    return sc


def visible_scene():
    """visible = 4 for query keyframe 6: keyframe 3 (index visible - 1) is in the inverted file, keyframe 4 (index visible, equal to the
    query) is not.  Keyframe 1 is erased (equal to the query: in no list, and nothing as keyframe 3's neighbour); erased keyframe 0 in the
    connected row is skipped (it shares no word: it would make minScore -0.0f); connected keyframe 5 is beyond visible and still sets
    minScore = 0.25.  A second query with visible = 5 sees keyframe 4."""
    kf = [uv(range(50, 58)), uv(W8), uv(W8[:4] + [30, 31, 32, 33]), uv(W8[:6] + [20, 21]), uv(W8), uv([0, 1, 40, 41, 42, 43, 44, 45]), uv(W8)]
    return scene("visible", kf, [(6, 4, 1), (6, 5, 1)], neigh={3: [1]}, conn={6: [0, 2, 5]}, live=[0, 0, 1, 1, 1, 1, 1], cand=[[3], [4]], min_score=[0.25, 0.25])


def empty_row_scene():
    """an empty connected row: minScore stays 1.  Only keyframe 0 (equal to the query, score exactly 1) is an entry; keyframe 1 (0.875)
    is scored below minScore and still accumulated as its neighbour"""
    kf = [uv(W8), uv(W8[:7] + [20]), uv(W8)]
    sc = scene("empty_row", kf, [(2, 2, 1)], neigh={0: [1]}, cand=[[0]], min_score=[1.0])
    sc["acc"] = (0, F(1.875))
    return sc


def zero_scene():
    """a connected keyframe that shares no word scores -0.0f and minScore keeps those bits; the second query's vector is empty (every
    score is -0.0f, nothing is shared); the third is not selected; the fourth names no keyframe"""
    kf = [uv(range(50, 58)), uv([0, 1, 20, 21, 22, 23, 24, 25]), uv(W8), []]
    return scene("zero", kf, [(2, 2, 1), (3, 3, 1), (2, 2, 0), (9, 2, 1)], conn={2: [0], 3: [0, 1]}, cand=[[1], [], None, None], min_score=[-0.0, -0.0, None, None])


def sum_order_scene():
    """a score whose sum shows the order of its additions (the scene of tests/reloc_db_scenes.py): terms -2M, -2^-54, -2^-54 with
    2M = 0.5 + 2^-25; in ascending word order the small terms are lost one by one and -score / 2 narrows to 0.25, added first they make
    one ulp and it narrows to the float above.  minScore, from the connected keyframe, is 0.25 too: si == minScore once more."""
    M = 0.25 + 2.0 ** -26; tiny = 2.0 ** -55
    v = [(3, M), (5, tiny), (8, tiny)]
    assert F(L.R.l1_score(v, v)) == F(0.25) and F(L.R.l1_score(v, v, "reverse")) == np.nextafter(F(0.25), F(1))
    return scene("sum_order", [v, [(3, 0.5), (9, 0.5)], v], [(2, 2, 1)], conn={2: [1]}, cand=[[0]], min_score=[0.25])


def batch_scene():
    """eight consecutive keyframes appended to a database of sixty, each queried with visible = its own index, from one snapshot: vectors
    of up to 80 words on nfeatures 256, connected rows of 0 to 12 (repeats, -1 and out-of-range entries among them), ten neighbours on
    some keyframes, erased keyframes, keyframes without a record"""
    t = D.TREE3; u = D.usable_words(t)
    rng = np.random.default_rng(77)
    nK = 68
    kf = []
    for k in range(nK):
        n = (70, 66, 3, 1, 40)[k % 5] if k % 2 else int(rng.integers(1, len(u)))
        kf.append(D.vec(t, [int(w) for w in rng.permutation(u)[:n]] + ([int(u[k % 7])] * 2 if k % 3 == 0 else [])))
    neigh = {k: [int(x) for x in rng.permutation(nK)[:(10 if k % 4 == 0 else int(rng.integers(0, 10)))]] for k in range(nK)}
    conn = {k: [int(x) for x in rng.integers(-1, nK + 2, int(rng.integers(0, 13)))] for k in range(nK)}
    live = (rng.uniform(size=nK) > 0.1).astype(np.uint8)
    rec = np.where(rng.uniform(size=nK) > 0.15, np.arange(nK) + 4, -1)
    return scene("batch", kf, [(k, k, 1 if k != 63 else 0) for k in range(60, 68)], neigh=neigh, conn=conn, live=live, kf_record=rec, max_cand=3, nf=256,
                 group_cap=6, member_cap=16, th=1)


def scenes():
    return [connected_scene(), threshold_scene(), min_score_scene(), stale_scene(), retain_scene(), order_scene(4), order_scene(2), dedupe_scene(),
            visible_scene(), empty_row_scene(), zero_scene(), sum_order_scene(), batch_scene()]


SIZES = (0, 1, 63, 64, 65, 130)


def sizes_scene():
    """the minScore kernel at query and connected vectors of 0, 1, 63, 64, 65 and 130 words (nfeatures 256): keyframes 0-5 are connected
    to each of the queries 6-11, every vector drawn from 200 words so that every pair with words shares some"""
    rng = np.random.default_rng(5)

    def rvec(n):
        ws = sorted(int(w) for w in rng.permutation(200)[:n])
        vals = rng.uniform(0.01, 1.0, n)
        return [(w, float(x / vals.sum())) for w, x in zip(ws, vals)]
    kf = [rvec(n) for n in SIZES + SIZES]
    return scene("sizes", kf, [(6 + i, 6, 1) for i in range(6)], conn={6 + i: list(range(6)) for i in range(6)}, nf=256)


def random_scene(seed):
    """a seeded random database over few words: many ties, many shared neighbours and connected keyframes, queries in sequence"""
    rng = np.random.default_rng(seed)
    nK = int(rng.integers(2, 24)); nW = int(rng.integers(3, 30))

    def rvec():
        n = int(rng.integers(0, nW + 1))
        ws = sorted(int(w) for w in rng.permutation(nW)[:n])
        vals = rng.uniform(0.01, 1.0, n)
        return [(w, float(x / vals.sum())) for w, x in zip(ws, vals)]
    neigh = {k: [int(x) for x in rng.integers(0, nK, int(rng.integers(0, 11)))] for k in range(nK)}
    conn = {k: [int(x) for x in rng.integers(0, nK, int(rng.integers(0, 4)))] for k in range(nK)}
    live = None if seed % 3 == 0 else (rng.uniform(size=nK) > 0.2).astype(np.uint8)
    queries = [(int(q), int(rng.integers(0, nK + 1)), 1) for q in rng.integers(0, nK, 4)]
    return scene("random%d" % seed, [rvec() for _ in range(nK)], queries, neigh=neigh, conn=conn, live=live, max_cand=3, group_cap=5, member_cap=6, th=2)


# ---- groups ------------------------------------------------------------------------------------------------------------------------
def group_scene(name, n, conn, groups, queries, th=3, max_cand=4, group_cap=6, member_cap=6, kf_record=None, want_groups=None, want_enough=None):
    """queries: [(keyframe, candidate list or None)]"""
    sc = scene(name, [[] for _ in range(n)], [(q, q, 1) for q, _ in queries], conn=conn, kf_record=kf_record, max_cand=max_cand, th=th, group_cap=group_cap,
               member_cap=member_cap)
    sc.update(groups=[(set(g), c) for g, c in groups], lists=[c for _, c in queries], want_groups=want_groups, want_enough=want_enough)
    return sc


def group_scenes():
    G = group_scene
    return [
        G("no_previous", 30, {3: [4, 9], 5: []}, [], [(20, [3, 5])], want_groups=[({3, 4, 9}, 0), ({5}, 0)], want_enough=[[]]),
        # candidate 3 meets group 1 only as itself, candidate 5 meets group 0 only through its connected keyframe 11; counters 1 -> 2 = th, 0 -> 1 = th - 1
        G("self_and_connected", 30, {3: [20], 5: [11, 21]}, [({10, 11}, 0), ({3}, 1)], [(25, [3, 5])], th=2,
          want_groups=[({3, 20}, 2), ({5, 11, 21}, 1)], want_enough=[[3]]),
        # two candidates consistent with one previous group: one entry (the first candidate's), both enough
        G("two_candidates_one_group", 30, {1: [7], 2: [7]}, [({7}, 2)], [(25, [1, 2])], want_groups=[({1, 7}, 3)], want_enough=[[1, 2]]),
        # one candidate consistent with two previous groups: two entries, enough once
        G("one_candidate_two_groups", 30, {1: [7, 8]}, [({7}, 2), ({8}, 0)], [(25, [1])], want_groups=[({1, 7, 8}, 3), ({1, 7, 8}, 1)], want_enough=[[1]]),
        # a group continued by its first consistent candidate while a later candidate opens a new one; the pushes interleave by candidate
        G("interleaved", 30, {1: [7], 2: [], 4: [8, 7]}, [({8}, 0), ({7}, 1)], [(25, [1, 2, 4])], th=2,
          want_groups=[({1, 7}, 2), ({2}, 0), ({4, 7, 8}, 1)], want_enough=[[1, 4]]),
        G("empty_clears", 30, {1: [7]}, [({7}, 2), ({8}, 0)], [(25, []), (26, [1])], want_groups=[({1, 7}, 0)], want_enough=[[], []]),
        G("not_selected_keeps", 30, {1: [7]}, [({7}, 2)], [(25, None), (26, [1])], want_groups=[({1, 7}, 3)], want_enough=[[], [1]]),
        G("four_in_sequence", 30, {1: [7], 2: [1], 3: [2, 9], 4: [3]}, [], [(25, [1]), (26, [2]), (27, [3, 1]), (28, [4])], th=3,
          kf_record=[-1 if k == 3 else k + 2 for k in range(30)], want_enough=[[], [], [], [4]]),
        # the three overflows: the state stays, this and every later query report status 1
        G("member_overflow", 30, {1: [7, 8, 9], 2: []}, [({7}, 2)], [(25, [1]), (26, [2])], member_cap=3, want_groups=[({7}, 2)], want_enough=[[], []]),
        G("group_overflow", 30, {1: [], 2: [], 3: []}, [({7}, 2)], [(24, [1, 2]), (25, [1, 2, 3]), (26, [])], group_cap=2, want_groups=[({1}, 0), ({2}, 0)],
          want_enough=[[], [], []]),
        G("candidate_overflow", 30, {1: [7], 2: [7]}, [({7}, 2)], [(25, [1, 2, 5]), (26, [1])], max_cand=2, want_groups=[({7}, 2)], want_enough=[[], []]),
        # exactly at the caps: exact
        G("at_the_caps", 30, {1: [7, 8], 2: []}, [({7}, 2)], [(25, [1, 2])], member_cap=3, group_cap=2, max_cand=2, want_groups=[({1, 7, 8}, 3), ({2}, 0)],
          want_enough=[[1]]),
    ]
