"""reloc_db_ref.py -- plain-Python / numpy restatement of what ivf_tracker_bow_vectors and ivf_tracker_reloc_candidates replace (test
infrastructure only): BowVector accumulation and L1 normalisation (Thirdparty/DBoW2/DBoW2/BowVector.cpp:34-46, :62-84, as
TemplatedVocabulary::transform drives them, TemplatedVocabulary.h:1126-1204), L1Scoring::score (ScoringObject.cpp:23-68) and
KeyFrameDatabase::DetectRelocalizationCandidates (ORB/src/KeyFrameDatabase.cc:199-309), written with real per-word inverted lists and the
reference's own loops.  Python floats are the reference's doubles, np.float32 every float it holds.  Besides the candidates it says, per
keyframe, where the keyframe left the function: the scenes of tests/reloc_db_scenes.py are built to reach every such exit.

detect() takes a `fault` for tests/test_reloc_db_cpu.py, which checks that the scenes can tell each of them from the reference:
"reverse" (the score's sum in descending word order), "double08" (0.8 in double), "ge_common" / "ge_best" / "ge_retain" (>= for > at
:246, :277, :297) and "ignore_reloc" (a neighbour that was not scored contributes 0)."""
import numpy as np

F = np.float32
NEIGH = 10
NO_SCORE_BITS = 0x7FC00000                                     # d_scores of a keyframe that was not scored (include/ivfront.h)
# where a keyframe left DetectRelocalizationCandidates
ABSENT, BELOW, DROPPED, RETAINED, REPLACED, DUPLICATE = range(6)
STAGE_NAMES = ["absent: shares no word", "below the common-word threshold", "scored, dropped by 0.75 * bestAccScore",
               "retained as itself", "retained, replaced by a neighbour", "retained, its pBestKF was already added"]


def bow_vector(words, weights):
    """mBowVec of one frame as [(word, value)] ascending, from the word id and weight of every keypoint in keypoint order"""
    v = {}
    for w, wt in zip(words, weights):
        wt = float(wt)
        if wt > 0:                                             # TemplatedVocabulary.h:1157
            v[int(w)] = v.get(int(w), 0.0) + wt                # operator[] makes 0.0, addWeight adds (BowVector.cpp:34-46)
    norm = 0.0
    for w in sorted(v):
        norm += abs(v[w])                                      # BowVector.cpp:67-71
    if norm > 0.0:
        for w in v:
            v[w] /= norm
    return [(w, v[w]) for w in sorted(v)]


def _lower_bound(v, word, lo):
    while lo < len(v) and v[lo][0] < word:
        lo += 1
    return lo


def l1_score(v1, v2, fault=None):
    """L1Scoring::score(v1, v2) -> double"""
    i = j = 0
    terms = []
    while i < len(v1) and j < len(v2):
        if v1[i][0] == v2[j][0]:
            vi, wi = v1[i][1], v2[j][1]
            terms.append(abs(vi - wi) - abs(vi) - abs(wi))
            i += 1; j += 1
        elif v1[i][0] < v2[j][0]:
            i = _lower_bound(v1, v2[j][0], i)
        else:
            j = _lower_bound(v2, v1[i][0], j)
    if fault == "reverse":
        terms.reverse()
    score = 0.0
    for t in terms:
        score += t
    return -score / 2.0


def inverted_file(vecs, live):
    """mvInvertedFile after add() of every keyframe in index order and erase() of the erased ones"""
    inv = {}
    for k, vec in enumerate(vecs):
        for w, _ in vec:
            inv.setdefault(w, []).append(k)
    for k, vec in enumerate(vecs):
        if live is not None and not live[k]:
            for w, _ in vec:
                inv[w].remove(k)
    return inv


def min_common_words(max_common, fault=None):
    if fault == "double08":
        return int(max_common * 0.8)
    return int(F(max_common) * F(0.8))                         # int minCommonWords = maxCommonWords*0.8f (:235)


def detect(vecs, neigh, fvec, live=None, reloc=None, fault=None):
    """one query.  vecs: the keyframes' vectors; neigh [nK][10]; fvec: the frame's vector; live / reloc: arrays or None.
    -> dict(cand: keyframe indices in the reference's order, common [nK], scores: float32 [nK] (NaN bits where not scored),
    stage [nK], replaced_by [nK])"""
    nK = len(vecs)
    inv = inverted_file(vecs, live)
    words = [0] * nK
    query = [False] * nK
    sharing = []
    for w, _ in fvec:                                          # :207-222
        for k in inv.get(w, []):
            if not query[k]:
                words[k] = 0; query[k] = True; sharing.append(k)
            words[k] += 1
    stage = np.full(nK, ABSENT, np.int32)
    replaced_by = np.full(nK, -1, np.int32)
    scores = np.full(nK, NO_SCORE_BITS, np.uint32).view(F)
    out = dict(cand=[], common=np.array(words, np.int32), scores=scores, stage=stage, replaced_by=replaced_by)
    if not sharing:
        return out
    max_common = 0
    for k in sharing:
        if words[k] > max_common:
            max_common = words[k]
    min_common = min_common_words(max_common, fault)
    state = np.zeros(nK, F) if reloc is None else np.array(reloc, F)     # mRelocScore of every keyframe
    is_scored = [False] * nK
    scored = []
    for k in sharing:                                          # :242-253
        if words[k] > min_common or (fault == "ge_common" and words[k] == min_common):
            si = F(l1_score(fvec, vecs[k], fault))
            state[k] = si; scores[k] = si; is_scored[k] = True
            scored.append((si, k))
        else:
            stage[k] = BELOW
    if not scored:
        return out
    acc_list = []
    best_acc = F(0)
    for si, k in scored:                                       # :262-287
        best = si; acc = si; best_kf = k
        for nb in neigh[k]:
            nb = int(nb)
            if nb < 0 or nb >= nK:
                continue
            if live is not None and not live[nb]:
                continue
            if not query[nb]:
                continue                                       # :273
            s = state[nb]
            if fault == "ignore_reloc" and not is_scored[nb]:
                s = F(0)
            acc = F(acc + s)
            if s > best or (fault == "ge_best" and s == best):
                best_kf = nb; best = s
        acc_list.append((acc, best_kf, k))
        if acc > best_acc:
            best_acc = acc
    min_retain = F(0.75) * best_acc                            # :290
    added = set()
    for acc, best_kf, k in acc_list:                           # :294-306
        if acc > min_retain or (fault == "ge_retain" and acc == min_retain):
            if best_kf not in added:
                out["cand"].append(best_kf); added.add(best_kf)
                stage[k] = RETAINED if best_kf == k else REPLACED
            else:
                stage[k] = DUPLICATE
            if best_kf != k:
                replaced_by[k] = best_kf
        else:
            stage[k] = DROPPED
    return out


def detect_shortcut(vecs, neigh, fvec, live=None, reloc=None):
    """the same query the way the device runs it: shared words by intersection, scored keyframes ordered by (smallest shared word,
    keyframe index), every distinct pBestKF at the smallest order key of the retained entries that name it -> cand"""
    nK = len(vecs)
    fw = {w: v for w, v in fvec}
    common = np.zeros(nK, np.int64); minw = np.zeros(nK, np.int64)
    for k, vec in enumerate(vecs):
        if live is not None and not live[k]:
            continue
        sh = [w for w, _ in vec if w in fw]
        common[k] = len(sh); minw[k] = sh[0] if sh else 0
    min_common = min_common_words(int(common.max()) if nK else 0)
    score = {k: F(l1_score(fvec, vecs[k])) for k in range(nK) if common[k] > min_common}
    state = np.zeros(nK, F) if reloc is None else np.array(reloc, F)
    acc = {}; best_of = {}
    best_acc = F(0)
    for k, si in score.items():
        best = si; a = si; bk = k
        for nb in neigh[k]:
            nb = int(nb)
            if nb < 0 or nb >= nK or (live is not None and not live[nb]) or common[nb] == 0:
                continue
            s = score[nb] if nb in score else state[nb]
            a = F(a + s)
            if s > best:
                bk = nb; best = s
        acc[k] = a; best_of[k] = bk
        if a > best_acc:
            best_acc = a
    place = {}
    for k in score:
        if acc[k] > F(0.75) * best_acc:
            key = (int(minw[k]), k)
            if best_of[k] not in place or key < place[best_of[k]]:
                place[best_of[k]] = key
    return [b for b, _ in sorted(place.items(), key=lambda it: it[1])]


def outputs(res, kf_record, frame_record, max_cand):
    """the rows ivf_tracker_reloc_candidates writes for one frame: (cand [max_cand], ncand, pairs [max_cand, 2], select [max_cand])"""
    cand = np.full(max_cand, -1, np.int32); pairs = np.full((max_cand, 2), -1, np.int32); select = np.zeros(max_cand, np.int32)
    for j, k in enumerate(res["cand"][:max_cand]):
        cand[j] = k
        if kf_record[k] >= 0:
            pairs[j] = (kf_record[k], frame_record); select[j] = 1
    return cand, len(res["cand"]), pairs, select
