"""reloc_db_scenes.py -- hand-made scenes for ivf_tracker_bow_vectors / ivf_tracker_reloc_candidates (test infrastructure only), shared by
tests/test_reloc_db_cpu.py (the restatement of tests/reloc_db_ref.py reaches the exit each scene was built for; injected faults are seen)
and tests/test_gpu_reloc_db.py (the device against the restatement).  Everything is drawn from fixed seeds.

A scene is a small keyframe database and a few lost frames.  Where a keyframe or a frame is given as a list of word ids (one per keypoint,
in keypoint order) on a tree of tests/track_bow_scenes.py, its vector is reloc_db_ref.bow_vector of those words and the tree's weights,
and descriptors() turns the list into descriptors that descend to exactly those words, so the same scene runs through the device's
ivf_tracker_bow_vectors.  Where a gate needs exact values (a sum whose order shows, an accScore of exactly 0.75f * bestAccScore) the
vectors or the mRelocScore state are given as numbers.  `expect` lists (frame, keyframe, stage) for the exits the scene was built for
and `cand` the candidate list of every frame where the scene is about the order."""
import numpy as np

import reloc_db_ref as R
import track_bow_scenes as S

F = np.float32
TREE2 = S.make_tree(2, 31)
TREE3 = S.TREES[3]


def leaf_of_word(tree):
    return {int(w): i for i, w in enumerate(tree["word"]) if w >= 0}


def weights_of(tree, words):
    lw = leaf_of_word(tree)
    return [tree["weight"][lw[w]] for w in words]


def usable_words(tree):
    """word ids with a positive weight, ascending"""
    lw = leaf_of_word(tree)
    return [w for w in sorted(lw) if tree["weight"][lw[w]] > 0]


def stopped_word(tree):
    return int(tree["word"][tree["stopped"]])


def vec(tree, words):
    return R.bow_vector(words, weights_of(tree, words))


def descriptors(tree, words, seed):
    """one descriptor per word id of the list that descends to that word's leaf (the address bytes of tests/track_bow_scenes.py), random payload"""
    lw = leaf_of_word(tree)
    b = S.Builder(tree, seed)
    return np.array([b.desc(S.path_to(tree, lw[w]), b.payload()) for w in words], np.uint8).reshape(len(words), 32)


def neigh_rows(rows, n):
    out = np.full((n, R.NEIGH), -1, np.int32)
    for k, r in rows.items():
        out[k, :len(r)] = r
    return out


def scene(name, tree, kf, frames, neigh=None, live=None, reloc=None, kf_record=None, frame_record=None, max_cand=4, expect=(), cand=None, nf=64):
    """kf / frames: each entry a list of word ids, or a vector [(word, value)]"""
    def both(x):
        if len(x) and isinstance(x[0], tuple):
            return None, list(x)
        return list(x), vec(tree, x)
    kfs = [both(x) for x in kf]; frs = [both(x) for x in frames]
    n = len(kfs)
    for wl, v in kfs + frs:
        assert len(v) <= nf and (wl is None or len(wl) <= nf)
    return dict(name=name, tree=tree, nf=nf, kf_words=[a for a, _ in kfs], kf_vecs=[b for _, b in kfs], frame_words=[a for a, _ in frs],
                frame_vecs=[b for _, b in frs], neigh=neigh_rows(neigh or {}, n), live=None if live is None else np.array(live, np.uint8),
                reloc=None if reloc is None else np.array(reloc, F),
                kf_record=np.arange(n, dtype=np.int32) if kf_record is None else np.array(kf_record, np.int32),
                frame_record=(n + np.arange(len(frs), dtype=np.int32)) if frame_record is None else np.array(frame_record, np.int32),
                max_cand=max_cand, expect=list(expect), cand=cand)


def run(sc, f, fault=None, reloc="scene"):
    return R.detect(sc["kf_vecs"], sc["neigh"], sc["frame_vecs"][f], sc["live"], sc["reloc"] if isinstance(reloc, str) else reloc, fault)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
def basic_scene():
    """no shared word; an empty vector (every word stopped, norm 0); a word reached by several keypoints (k-fold addition)"""
    t = TREE3; u = usable_words(t); st = stopped_word(t)
    kf = [u[0:5], [u[20], u[21], u[21], u[21], u[22], st], [st, st]]
    frames = [u[10:15], [st] * 5, [u[21]] * 4 + [u[20], u[22], u[22], u[30]]]
    return scene("basic", t, kf, frames,
                 expect=[(0, 0, R.ABSENT), (0, 1, R.ABSENT), (1, 0, R.ABSENT), (1, 1, R.ABSENT), (2, 0, R.ABSENT), (2, 1, R.RETAINED), (2, 2, R.ABSENT)],
                 cand=[[], [], [1]])


def threshold_scene():
    """maxCommonWords of 4, 5, 10 and 15: minCommonWords = (int)(max * 0.8f) = 3, 4, 8, 12; per maximum a keyframe at exactly
    minCommonWords (below: the test is a strict >) and one at minCommonWords + 1 (scored)"""
    t = TREE3; u = usable_words(t)
    kf = []; frames = []; expect = []
    base = 0
    spare = u[40:]
    for f, (n, mn) in enumerate(((4, 3), (5, 4), (10, 8), (15, 12))):
        assert R.min_common_words(n) == mn
        block = u[base:base + n]; base += n
        frames.append(block)
        k0 = len(kf)
        kf += [block, block[:mn] + spare[:3], block[:mn + 1] + spare[3:5]]
        expect += [(f, k0, R.RETAINED), (f, k0 + 1, R.BELOW)]
    sc = scene("threshold", t, kf, frames, expect=expect)
    sc["scored"] = [(f, 3 * f + 2) for f in range(4)]
    return sc


def neighbour_scene(reloc_value):
    """covisibility accumulation.  Frame 0 holds ten words.  Keyframe 0 holds them and three more and lists as neighbours: 1 (shares no
    word: skipped, whatever mRelocScore it holds), 2 (shares one word, below the threshold: contributes its mRelocScore of BEFORE the call
    -- nothing with a NULL array, so that keyframe 0 is dropped; with 0.9 keyframe 0 is retained and 2 becomes its pBestKF), 3 (erased,
    though its vector shares every word: skipped, and absent as a sharer), -1 padding.  Keyframe 4 (lower score) lists 5 (greater score):
    pBestKF moves, 5 comes out at 4's place and 5's own entry (which lists 4: no move) is a duplicate.  Keyframes 6 and 7 hold the same vector and list each
    other: an equal score does not move pBestKF."""
    t = TREE3; u = usable_words(t)
    fw = u[0:10]
    kf = [fw + u[44:47], u[30:34], [fw[0]] + u[34:38], fw, fw[:9] + u[38:41], fw[:9] + u[41:42], fw[1:10] + u[42:44], fw[1:10] + u[42:44]]
    live = [1, 1, 1, 0, 1, 1, 1, 1]
    neigh = {0: [1, 2, 3], 4: [5], 5: [4], 6: [7], 7: [6]}
    reloc = None if reloc_value is None else [0, 7.0, reloc_value, 9.0, 0, 0, 0, 0]
    assert reloc_value is None or F(R.l1_score(vec(t, fw), vec(t, kf[0]))) < F(reloc_value)
    expect = [(0, 1, R.ABSENT), (0, 2, R.BELOW), (0, 3, R.ABSENT), (0, 4, R.REPLACED), (0, 5, R.DUPLICATE), (0, 6, R.RETAINED), (0, 7, R.RETAINED),
              (0, 0, R.DROPPED if reloc_value is None else R.REPLACED)]
    cand = [[5, 6, 7]] if reloc_value is None else [[2, 5, 6, 7]]
    return scene("neighbours_reloc_%s" % ("null" if reloc_value is None else "value"), t, kf, [fw], neigh=neigh, live=live, reloc=reloc,
                 expect=expect, cand=cand, max_cand=6)


def retain_scene(above):
    """accScore exactly 0.75f * bestAccScore is dropped (strict >); one float above it is retained.  Keyframes 0 and 1 are scored; each
    lists a neighbour that shares one word and is below the threshold, whose mRelocScore of before the call makes the sums exact:
    accScore(0) = 4, accScore(1) = 3 (or the next float above 3)."""
    t = TREE3; u = usable_words(t)
    fw = u[0:10]
    kf = [fw, fw[:9] + u[30:31], [fw[0]] + u[31:35], [fw[1]] + u[35:39]]
    neigh = {0: [2], 1: [3]}
    fv = vec(t, fw)
    s0 = F(R.l1_score(fv, vec(t, kf[0]))); s1 = F(R.l1_score(fv, vec(t, kf[1])))

    def complement(s, targets):
        c = np.nextafter(F(targets[0]) - s, F(-9))
        for _ in range(16):
            if F(s + c) in targets:
                return c
            c = np.nextafter(c, F(9))
        raise AssertionError("no float completes %r to %r" % (s, targets))
    up = [np.nextafter(F(3), F(9))]
    up.append(np.nextafter(up[0], F(9)))                      # one or two floats above 3: whichever a float sum reaches
    reloc = [0, 0, complement(s0, [F(4)]), complement(s1, up if above else [F(3)])]
    assert F(0.75) * F(4) == F(3)
    expect = [(0, 0, R.REPLACED), (0, 1, R.REPLACED if above else R.DROPPED), (0, 2, R.BELOW), (0, 3, R.BELOW)]
    return scene("retain_%s" % ("above" if above else "exact"), t, kf, [fw], neigh=neigh, reloc=reloc, expect=expect, cand=[[2, 3] if above else [2]])


def order_scene(max_cand):
    """first-encounter order differs from index order: keyframe 1 holds the frame's smallest word, keyframe 0 does not; with
    max_candidates = 1 there are more candidates than slots.  Keyframe 1 has no gather record."""
    t = TREE2; u = usable_words(t)
    fw = [u[1], u[2], u[8], u[9]]
    kf = [[u[2], u[8], u[9]], [u[1], u[2], u[8]], [u[9], u[10], u[11], u[12], u[13]]]
    return scene("order_max%d" % max_cand, t, kf, [fw], kf_record=[5, -1, 6], frame_record=[9], max_cand=max_cand,
                 expect=[(0, 0, R.RETAINED), (0, 1, R.RETAINED), (0, 2, R.BELOW)], cand=[[1, 0]])


def sum_order_scene():
    """a score whose sum shows the order of its additions: terms -2M, -2^-54, -2^-54 with 2M = 0.5 + 2^-25.  In ascending word order each
    small term is half an ulp of the running sum and is lost (ties to even); added first they make one ulp.  -score / 2 is then M
    = 0.25 + 2^-26, halfway between two floats (narrowed to the even one, 0.25), or one double above it (narrowed to 0.25 + 2^-25)."""
    M = 0.25 + 2.0 ** -26; tiny = 2.0 ** -55
    v = [(3, M), (5, tiny), (8, tiny)]
    sc = scene("sum_order", TREE2, [v, [(3, 0.5), (9, 0.5)]], [v], expect=[(0, 0, R.RETAINED)])
    assert F(R.l1_score(v, v)) == F(0.25) and F(R.l1_score(v, v, "reverse")) == np.nextafter(F(0.25), F(1))
    return sc


def wide_scene():
    """70 keyframes, vectors of up to 80 words (nfeatures 256), a frame of more than 64 words, ten neighbours on some keyframes, erased
    keyframes, keyframes without a record, an mRelocScore state: every lane stride and wave boundary of the kernels is crossed"""
    t = TREE3; u = usable_words(t)
    rng = np.random.default_rng(41)
    nK = 70
    assert len(u) >= 72
    kf = []
    for k in range(nK):
        n = (70, 66, 3, 1, 40)[k % 5] if k < 60 else int(rng.integers(1, len(u)))
        kf.append([int(w) for w in rng.permutation(u)[:n]] + ([int(u[k % 7])] * 2 if k % 3 == 0 else []))
    frames = [[int(w) for w in rng.permutation(u)[:68]] + [int(u[3])] * 3, [int(w) for w in rng.permutation(u)[:30]], [int(u[5]), int(u[6])],
              [int(w) for w in rng.permutation(u)[:72]]]
    neigh = {}
    for k in range(nK):
        m = 10 if k % 4 == 0 else int(rng.integers(0, 10))
        neigh[k] = [int(x) for x in rng.permutation(nK)[:m]]
    live = (rng.uniform(size=nK) > 0.1).astype(np.uint8)
    reloc = rng.uniform(0, 0.4, nK).astype(F)
    rec = np.where(rng.uniform(size=nK) > 0.15, np.arange(nK) + 4, -1)
    return scene("wide", t, kf, frames, neigh=neigh, live=live, reloc=reloc, kf_record=rec, frame_record=[0, 1, 2, 3], max_cand=3, nf=256)


def scenes():
    return [basic_scene(), threshold_scene(), neighbour_scene(None), neighbour_scene(0.9), retain_scene(False), retain_scene(True),
            order_scene(4), order_scene(1), sum_order_scene(), wide_scene()]


def random_scene(seed):
    """a seeded random database of numeric vectors over few words: many ties of the smallest shared word, many shared neighbours"""
    rng = np.random.default_rng(seed)
    nK = int(rng.integers(1, 24)); nW = int(rng.integers(3, 30))

    def rvec():
        n = int(rng.integers(0, nW + 1))
        ws = sorted(int(w) for w in rng.permutation(nW)[:n])
        vals = rng.uniform(0.01, 1.0, n)
        return [(w, float(x / vals.sum())) for w, x in zip(ws, vals)]
    vecs = [rvec() for _ in range(nK)]
    neigh = np.full((nK, R.NEIGH), -1, np.int32)
    for k in range(nK):
        m = int(rng.integers(0, R.NEIGH + 1))
        neigh[k, :m] = rng.integers(0, nK, m)
    live = None if seed % 3 == 0 else (rng.uniform(size=nK) > 0.2).astype(np.uint8)
    reloc = None if seed % 2 == 0 else rng.uniform(0, 1, nK).astype(F)
    return dict(kf_vecs=vecs, neigh=neigh, live=live, reloc=reloc, frame_vecs=[rvec() for _ in range(3)])
