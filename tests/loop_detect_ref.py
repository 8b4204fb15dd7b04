"""loop_detect_ref.py -- plain-Python restatement of what ivf_tracker_loop_candidates and ivf_tracker_loop_consistency replace (test
infrastructure only): LoopClosing::DetectLoop (ORB/src/LoopClosing.cc:108-234) with KeyFrameDatabase::DetectLoopCandidates
(ORB/src/KeyFrameDatabase.cc:76-197), written the way the reference runs: an inverted file per word, lists, sets, and per-keyframe
mnLoopQuery / mnLoopWords / mLoopScore fields that live in a Fields object ACROSS queries (and can be preset to anything), so that stale
fields are shown not to matter.  Vectors and L1Scoring::score are tests/reloc_db_ref.py's.  Python floats are the reference's doubles,
np.float32 every float it holds.

Each function has an independent "shortcut" form, the parallel formulation the device runs (set intersections, order keys, a consistency
matrix); tests/test_loop_detect_cpu.py proves the two equal on every scene.

`fault` (the reference forms only), for the test that the scenes can tell each of them from the reference.  Candidates:
"keep_connected" (connected keyframes are not excluded), "connected_max" (they are excluded but still raise maxCommonWords),
"connected_neighbour" (a connected neighbour that would have been scored is accumulated), "double08", "ge_common", "gt_min_score" (si > minScore at :136),
"stale_neighbour" (relocalization's rule: a neighbour sharing a word adds its mLoopScore, scored or not), "neighbour_min_score" (a
neighbour counts only if its own score reached minScore), "best_from_zero", "ge_retain", "no_dedupe", "index_order" (candidates by
keyframe index), "visible_inclusive" (k <= visible), "ignore_live", "bad_connected" (minScore over erased keyframes too), "min_visible"
(minScore under the visible limit), "min_from_zero" (-0.0f is lost: max(minScore, 0)), "reverse" (the score's sum backwards).
Consistency: "flagged_blocks_enough", "push_every", "gt_th", "no_self", "keep_on_empty", "last_first" (a previous group is continued by its
LAST consistent candidate)."""
import numpy as np

import reloc_db_ref as R

F = np.float32
NEIGH = R.NEIGH
NO_SCORE_BITS = R.NO_SCORE_BITS
NCAND_SKIPPED, NCAND_BAD_QUERY = -2, -1


class Fields:
    """mnLoopQuery / mnLoopWords / mLoopScore of every keyframe, and the mnId the next query gets (unique per query, as keyframe ids are)"""

    def __init__(self, n, query=None, words=None, score=None):
        self.query = [-1] * n if query is None else list(query)
        self.words = [0] * n if words is None else list(words)
        self.score = np.zeros(n, F) if score is None else np.array(score, F)
        self.next_id = 1000


def row(conn, k, n):
    return [int(c) for c in conn[k] if 0 <= int(c) < n]


def min_score(vecs, live, conn, q, visible, fault=None):
    """LoopClosing.cc:129-143"""
    ms = F(1)
    for c in row(conn, q, len(vecs)):
        if live is not None and not live[c] and fault != "bad_connected":
            continue                                           # isBad (:135)
        if fault == "min_visible" and c >= visible:
            continue
        s = F(R.l1_score(vecs[q], vecs[c], fault))
        if s < ms:
            ms = s
    if fault == "min_from_zero" and not ms > 0:
        ms = F(0)
    return ms


def detect(fields, vecs, neigh, live, conn, q, visible, fault=None):
    """one query of keyframe q.  -> dict(min_score, cand, common [nK], scores [nK] (NaN bits where not scored))"""
    nK = len(vecs)
    ms = min_score(vecs, live, conn, q, visible, fault)
    lim = visible + 1 if fault == "visible_inclusive" else visible
    inside = [k < lim and k != q for k in range(nK)]
    inv = R.inverted_file([v if inside[k] else [] for k, v in enumerate(vecs)], None if fault == "ignore_live" else live)
    connected = set(row(conn, q, nK))
    qid = fields.next_id
    fields.next_id += 1
    sharing = []
    shadow = {}                                                # faults only: the words of the excluded connected keyframes
    for w, _ in vecs[q]:                                       # :86-105
        for k in inv.get(w, []):
            if fields.query[k] != qid:
                fields.words[k] = 0
                if k not in connected or fault == "keep_connected":
                    fields.query[k] = qid
                    sharing.append(k)
            fields.words[k] += 1
            if k in connected:
                shadow[k] = shadow.get(k, 0) + 1
    common = np.array([fields.words[k] if fields.query[k] == qid else 0 for k in range(nK)], np.int32)
    scores = np.full(nK, NO_SCORE_BITS, np.uint32).view(F)
    out = dict(min_score=ms, cand=[], common=common, scores=scores)
    if not sharing:
        return out
    max_common = 0
    for k in sharing:                                          # :114-118
        if fields.words[k] > max_common:
            max_common = fields.words[k]
    if fault == "connected_max":
        max_common = max([max_common] + list(shadow.values()))
    min_common = R.min_common_words(max_common, "double08" if fault == "double08" else None)
    score_and_match = []
    for k in sharing:                                          # :125-139
        if fields.words[k] > min_common or (fault == "ge_common" and fields.words[k] == min_common):
            si = F(R.l1_score(vecs[q], vecs[k], fault))
            fields.score[k] = si
            scores[k] = si
            if si > ms or (si == ms and fault != "gt_min_score"):
                score_and_match.append((si, k))
    if not score_and_match:
        return out
    if fault == "connected_neighbour":
        for k, n in shadow.items():
            if n > min_common:
                fields.query[k] = qid; fields.words[k] = n; fields.score[k] = F(R.l1_score(vecs[q], vecs[k]))
    acc_list = []
    best_acc = F(0) if fault == "best_from_zero" else ms       # :145
    for si, k in score_and_match:                              # :148-173
        best = si; acc = si; best_kf = k
        for nb in neigh[k]:
            nb = int(nb)
            if nb < 0 or nb >= nK:
                continue
            ok = fields.query[nb] == qid and fields.words[nb] > min_common
            if fault == "stale_neighbour":
                ok = fields.query[nb] == qid
            if fault == "neighbour_min_score":
                ok = ok and fields.score[nb] >= ms
            if ok:
                s = fields.score[nb]
                acc = F(acc + s)
                if s > best:
                    best_kf = nb; best = s
        acc_list.append((acc, best_kf, k))
        if acc > best_acc:
            best_acc = acc
    min_retain = F(0.75) * best_acc                            # :176
    added = set()
    for acc, best_kf, k in acc_list:                           # :182-193
        if acc > min_retain or (fault == "ge_retain" and acc == min_retain):
            if best_kf not in added or fault == "no_dedupe":
                out["cand"].append(best_kf); added.add(best_kf)
    if fault == "index_order":
        out["cand"].sort()
    return out


def detect_shortcut(vecs, neigh, live, conn, q, visible):
    """the same query the way the device runs it, with no field that outlives it"""
    nK = len(vecs)
    qw = {w for w, _ in vecs[q]}
    connected = set(row(conn, q, nK))
    live_ = lambda k: live is None or bool(live[k])
    ms = None
    for j, c in enumerate(row(conn, q, nK)):                   # the first entry of the row that holds the smallest score below 1
        if live_(c):
            s = F(R.l1_score(vecs[q], vecs[c]))
            if s < F(1) and (ms is None or s < ms):
                ms = s
    ms = F(1) if ms is None else ms
    common = np.zeros(nK, np.int32); minw = {}
    for k in range(nK):
        if k < visible and k != q and live_(k) and k not in connected:
            sh = [w for w, _ in vecs[k] if w in qw]
            common[k] = len(sh)
            if sh:
                minw[k] = sh[0]
    min_common = R.min_common_words(int(common.max()) if nK else 0)
    scores = np.full(nK, NO_SCORE_BITS, np.uint32).view(F)
    score = {}
    for k in range(nK):
        if common[k] > min_common:
            score[k] = F(R.l1_score(vecs[q], vecs[k])); scores[k] = score[k]
    entries = [k for k in score if score[k] >= ms]
    acc = {}; best_of = {}
    best_acc = ms
    for k in entries:
        best = score[k]; a = score[k]; bk = k
        for nb in neigh[k]:
            nb = int(nb)
            if 0 <= nb < nK and nb in score:
                a = F(a + score[nb])
                if score[nb] > best:
                    bk = nb; best = score[nb]
        acc[k] = a; best_of[k] = bk
        if a > best_acc:
            best_acc = a
    place = {}
    for k in entries:
        if acc[k] > F(0.75) * best_acc:
            key = (minw[k], k)
            if best_of[k] not in place or key < place[best_of[k]]:
                place[best_of[k]] = key
    return dict(min_score=ms, cand=[b for b, _ in sorted(place.items(), key=lambda it: it[1])], common=common, scores=scores)


# ---- the consistency groups --------------------------------------------------------------------------------------------------------
def consistency_step(groups, cand, conn, nK, th, fault=None):
    """LoopClosing.cc:148-216 for one query with candidates.  groups: [(set, counter)] -> (new groups, enough-consistent candidates)"""
    if not cand:
        return (list(groups) if fault == "keep_on_empty" else []), []
    current = []
    flagged = [False] * len(groups)
    enough = []
    for c in cand:
        group = set(row(conn, c, nK)) if 0 <= c < nK else set()
        if fault != "no_self" and 0 <= c < nK:
            group.add(c)
        b_enough = False; b_some = False
        for iG, (prev, count) in enumerate(groups):
            consistent = False
            for m in sorted(group):
                if m in prev:
                    consistent = True; b_some = True
                    break
            if consistent:
                n = count + 1
                if not flagged[iG] or fault in ("push_every", "last_first"):
                    if fault == "last_first":
                        current = [e for e in current if e[2] != iG]
                    current.append((set(group), n, iG))
                    flagged_before = flagged[iG]
                    flagged[iG] = True
                else:
                    flagged_before = True
                if (n > th if fault == "gt_th" else n >= th) and not b_enough and not (fault == "flagged_blocks_enough" and flagged_before):
                    enough.append(c); b_enough = True
        if not b_some:
            current.append((set(group), 0, -1))
    return [(g, n) for g, n, _ in current], enough


def consistency_step_shortcut(groups, cand, conn, nK, th):
    """the parallel formulation: a consistency matrix, the first consistent candidate of every previous group, entries by candidate"""
    if not cand:
        return [], []
    grp = [((set(row(conn, c, nK)) | {c}) if 0 <= c < nK else set()) for c in cand]
    cons = [[bool(g & prev) for prev, _ in groups] for g in grp]
    first = [next((i for i in range(len(cand)) if cons[i][iG]), -1) for iG in range(len(groups))]
    current = []
    for i in range(len(cand)):
        current += [(grp[i], groups[iG][1] + 1) for iG in range(len(groups)) if first[iG] == i]
        if not any(cons[i]):
            current.append((grp[i], 0))
    enough = [c for i, c in enumerate(cand) if any(cons[i][iG] and groups[iG][1] + 1 >= th for iG in range(len(groups)))]
    return current, enough


def pack_state(groups, group_cap, member_cap):
    """(member [group_cap, member_cap], size, count, n_groups [1]) with every row at or beyond n_groups cleared"""
    member = np.full((group_cap, member_cap), -1, np.int32); size = np.zeros(group_cap, np.int32); count = np.zeros(group_cap, np.int32)
    for e, (g, n) in enumerate(groups):
        m = sorted(g)
        member[e, :len(m)] = m; size[e] = len(m); count[e] = n
    return member, size, count, np.array([len(groups)], np.int32)


def consistency(groups, queries, conn, nK, kf_record, th, max_cand, group_cap, member_cap, step=consistency_step, fault=None):
    """the queries of one call in order.  queries: [(keyframe, cand list in full or None = not selected / no such keyframe)].
    -> (groups after the call, dict(enough [nQ, max_cand], nenough, pairs [nQ, max_cand, 2], select [nQ, max_cand], status))"""
    nQ = len(queries)
    out = dict(enough=np.full((nQ, max_cand), -1, np.int32), nenough=np.zeros(nQ, np.int32), pairs=np.full((nQ, max_cand, 2), -1, np.int32),
               select=np.zeros((nQ, max_cand), np.int32), status=np.zeros(nQ, np.int32))
    over = False
    for qi, (q, cand) in enumerate(queries):
        enough = []
        if not over and cand is not None:
            if len(cand) > max_cand:
                over = True
            else:
                new, enough = step(groups, list(cand), conn, nK, th, fault) if fault else step(groups, list(cand), conn, nK, th)
                if len(new) > group_cap or any(len(g) > member_cap for g, _ in new):
                    over = True; enough = []
                else:
                    groups = new
        out["status"][qi] = 1 if over else 0
        out["nenough"][qi] = len(enough)
        for j, c in enumerate(enough):
            out["enough"][qi, j] = c
            rq = kf_record[q] if 0 <= q < nK else -1
            rc = kf_record[c] if 0 <= c < nK else -1
            if rq >= 0 and rc >= 0:
                out["pairs"][qi, j] = (rq, rc); out["select"][qi, j] = 1
    return groups, out


def cand_rows(results, max_cand):
    """(cand [nQ, max_cand], ncand [nQ]) as ivf_tracker_loop_candidates writes them; a result of None is a query that was not selected,
    -1 one whose keyframe is outside the database: their cand rows are not written (marked -7 here and in the device test's prefill)"""
    cand = np.full((len(results), max_cand), -7, np.int32); ncand = np.zeros(len(results), np.int32)
    for i, r in enumerate(results):
        if r is None or isinstance(r, int):
            ncand[i] = NCAND_SKIPPED if r is None else NCAND_BAD_QUERY
            continue
        cand[i] = -1
        cand[i, :min(len(r["cand"]), max_cand)] = r["cand"][:max_cand]
        ncand[i] = len(r["cand"])
    return cand, ncand
