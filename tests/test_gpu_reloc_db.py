"""ivf_tracker_bow_vectors / ivf_tracker_reloc_candidates (iv_slam_amd/csrc/ivf_track_db.hip) -- the first two lines of
Tracking::Relocalization (ORB/src/Tracking.cc:2274-2285) for many lost frames on the device -- against the per-call ivf_bow_transform +
ivf_bow_vectors path and against the restatement of tests/reloc_db_ref.py on the hand-made scenes of tests/reloc_db_scenes.py.  Every
comparison is bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O
import reloc_db_ref as R
import reloc_db_scenes as D
import track_bow_scenes as S
from test_gpu_track import scale_table, iv  # noqa: F401  (iv: the module fixture)
from test_gpu_track_bow import vocabulary, make_tracker

pytestmark = pytest.mark.gpu
F = np.float32
SCENES = D.scenes()


def record_of(desc):
    n = len(desc)
    kp = np.zeros(n, S.KP_DTYPE); kp["x"] = 30.0 + np.arange(n) % 500; kp["y"] = 40.0; kp["size"] = 31
    return dict(kps=kp, desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32), uright=np.full(n, -1.0, F), depth=np.full(n, -1.0, F))


def pack_vecs(vecs, nf, counts=None):
    n = len(vecs)
    word = np.full((n, nf), -1, np.int32); value = np.zeros((n, nf), np.float64); cnt = np.zeros(n, np.int32)
    for k, v in enumerate(vecs):
        cnt[k] = len(v)
        for j, (w, x) in enumerate(v):
            word[k, j] = w; value[k, j] = x
    if counts is not None:
        cnt[:] = counts
    return word, value, cnt


def device_bow_vectors(iv, tr, V, recs, frames, nf):
    """-> (word [n, nf], value [n, nf], n [n]) from the device, prefilled with marks"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev)
    word = torch.full((len(frames), nf), -7, dtype=torch.int32, device=dev); value = torch.full((len(frames), nf), 7.5, dtype=torch.float64, device=dev)
    cnt = torch.full((len(frames),), -7, dtype=torch.int32, device=dev)
    tr.bow_vectors(V, block, fr, word, value, cnt)
    torch.cuda.synchronize()
    return word.cpu().numpy(), value.cpu().numpy(), cnt.cpu().numpy()


def device_candidates(iv, tr, V, sc, frame_vecs, frame_counts=None, max_cand=None, with_optional=True):
    """-> dict of the arrays ivf_tracker_reloc_candidates wrote for the scene's database and the given frames"""
    import torch
    dev = torch.device("cuda:0")
    nf = tr.nfeatures; nK = len(sc["kf_vecs"]); nF = len(frame_vecs); mc = max_cand or sc["max_cand"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw, kv, kn = pack_vecs(sc["kf_vecs"], nf); fw, fv, fn = pack_vecs(frame_vecs, nf, frame_counts)
    out = dict(cand=torch.full((nF, mc), -7, dtype=torch.int32, device=dev), ncand=torch.full((nF,), -7, dtype=torch.int32, device=dev),
               pairs=torch.full((nF * mc, 2), -7, dtype=torch.int32, device=dev), select=torch.full((nF * mc,), -7, dtype=torch.int32, device=dev))
    if with_optional:
        out["scores"] = torch.full((nF, nK), 7.0, dtype=torch.float32, device=dev); out["common"] = torch.full((nF, nK), -7, dtype=torch.int32, device=dev)
    tr.reloc_candidates(V, t(kw), t(kv), t(kn), t(sc["neigh"]), t(sc["kf_record"]), t(fw), t(fv), t(fn), t(sc["frame_record"][:nF]),
                        out["cand"], out["ncand"], out["pairs"], out["select"], kf_live=None if sc["live"] is None else t(sc["live"]),
                        kf_reloc_score=None if sc["reloc"] is None else t(sc["reloc"]), scores=out.get("scores"), common=out.get("common"))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def expected(sc, frame_vecs, max_cand=None):
    mc = max_cand or sc["max_cand"]
    nK = len(sc["kf_vecs"]); nF = len(frame_vecs)
    e = dict(cand=np.zeros((nF, mc), np.int32), ncand=np.zeros(nF, np.int32), pairs=np.zeros((nF * mc, 2), np.int32), select=np.zeros(nF * mc, np.int32),
             scores=np.zeros((nF, nK), F), common=np.zeros((nF, nK), np.int32))
    for f, fv in enumerate(frame_vecs):
        res = R.detect(sc["kf_vecs"], sc["neigh"], fv, sc["live"], sc["reloc"])
        e["cand"][f], e["ncand"][f], e["pairs"][f * mc:(f + 1) * mc], e["select"][f * mc:(f + 1) * mc] = R.outputs(res, sc["kf_record"], sc["frame_record"][f], mc)
        e["scores"][f] = res["scores"]; e["common"][f] = res["common"]
    return e


def test_bow_vectors_equal_the_per_call_path(iv):
    """every word list of the scenes as a record of descriptors (stopped words, k keypoints on one word, more than 64 words) and 200 random
    descriptors on a ragged random tree; frame slots in another order than the records, one record twice, two record indices outside the
    block: word ids and value bits equal ivf_bow_transform + ivf_bow_vectors and the restatement; a second run is byte-identical"""
    nf = 256
    for tree, lists in ((D.TREE3, [w for sc in SCENES if sc["tree"] is D.TREE3 for w in sc["kf_words"] + sc["frame_words"] if w is not None]),
                        (D.TREE2, [w for sc in SCENES if sc["tree"] is D.TREE2 for w in sc["kf_words"] + sc["frame_words"] if w is not None]),
                        (O.make_vocabulary(5, 3, seed=5, early_leaf_frac=0.1, stop_frac=0.1), None)):
        if lists is None:
            rng = np.random.default_rng(3)
            descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (200, 1, 0, 256)]
        else:
            descs = [D.descriptors(tree, w, 7 + i) if w else np.zeros((0, 32), np.uint8) for i, w in enumerate(lists)]
        V = vocabulary(iv, tree)
        tr = make_tracker(iv, nf, 2)
        recs = [record_of(d) for d in descs]
        frames = list(range(len(recs)))[::-1] + [0, len(recs) + 2, -1]
        word, value, cnt = device_bow_vectors(iv, tr, V, recs, frames, nf)
        most = 0
        for s, r in enumerate(frames):
            if not 0 <= r < len(recs):
                assert cnt[s] == -1 and (word[s] == -7).all() and (value[s] == 7.5).all()
                continue
            bow, _ = V.transform(descs[r], 0) if len(descs[r]) else ({}, {})
            n = cnt[s]
            assert n == len(bow) and word[s, :n].tolist() == sorted(bow) and (word[s, n:] == -1).all() and not value[s, n:].any()
            assert value[s, :n].tobytes() == np.array([bow[w] for w in sorted(bow)], np.float64).tobytes(), (r, n)
            if len(descs[r]):
                wid, _, wt = O.bow_transform(tree, descs[r], 0)
                assert [(int(w), float(x)) for w, x in zip(word[s, :n], value[s, :n])] == R.bow_vector(wid, wt)
            most = max(most, n)
        assert most > 64 or lists is None or tree is D.TREE2
        again = device_bow_vectors(iv, tr, V, recs, frames, nf)
        assert again[0].tobytes() == word.tobytes() and again[1].tobytes() == value.tobytes() and again[2].tobytes() == cnt.tobytes()


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_reloc_candidates_equal_the_restatement(iv, sc):
    """every scene through the ABI, with one more frame whose d_bow_n is -1 (a record index ivf_tracker_bow_vectors refused): all six
    outputs equal the restatement byte for byte, a second run is byte-identical, and the outputs without the optional arrays are the same"""
    V = vocabulary(iv, sc["tree"])
    tr = make_tracker(iv, sc["nf"], 2)
    fvs = sc["frame_vecs"] + [sc["frame_vecs"][0]]
    counts = [len(v) for v in sc["frame_vecs"]] + [-1]
    sc = dict(sc, frame_record=np.concatenate([sc["frame_record"], [77]]).astype(np.int32))
    got = device_candidates(iv, tr, V, sc, fvs, counts)
    want = expected(sc, fvs[:-1] + [[]])
    for k in ("ncand", "cand", "pairs", "select", "common", "scores"):
        assert got[k].tobytes() == want[k].tobytes(), "%s %s:\n%r\n%r" % (sc["name"], k, got[k], want[k])
    if sc["cand"] is not None:
        for f, c in enumerate(sc["cand"]):
            assert got["ncand"][f] == len(c) and got["cand"][f, :min(len(c), sc["max_cand"])].tolist() == c[:sc["max_cand"]]
    again = device_candidates(iv, tr, V, sc, fvs, counts)
    bare = device_candidates(iv, tr, V, sc, fvs, counts, with_optional=False)
    for k in got:
        assert again[k].tobytes() == got[k].tobytes() and (k not in bare or bare[k].tobytes() == got[k].tobytes()), k


def test_one_handle_grows_its_scratch_and_takes_an_empty_database(iv):
    """a small database, then the 70-keyframe one, then the small one again on one handle (the scratch grows once); n_keyframes = 0 and
    n_frames = 0; max_candidates above and below the count"""
    import torch
    V = vocabulary(iv, D.TREE3)
    tr = make_tracker(iv, 256, 2)
    small, wide = SCENES[1], SCENES[-1]
    for sc in (small, wide, small):
        for mc in (1, 2, 9):
            got = device_candidates(iv, tr, V, sc, sc["frame_vecs"], max_cand=mc)
            want = expected(sc, sc["frame_vecs"], mc)
            for k in want:
                assert got[k].tobytes() == want[k].tobytes(), (sc["name"], mc, k)
    empty = dict(wide, kf_vecs=[], neigh=np.zeros((0, 10), np.int32), live=None, reloc=None, kf_record=np.zeros(0, np.int32))
    got = device_candidates(iv, tr, V, empty, wide["frame_vecs"])
    assert (got["ncand"] == 0).all() and (got["cand"] == -1).all() and (got["pairs"] == -1).all() and (got["select"] == 0).all()
    got = device_candidates(iv, tr, V, wide, [])
    assert got["ncand"].size == 0


def test_argument_errors(iv):
    import torch
    from iv_slam_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    V = vocabulary(iv, D.TREE3)
    tr = make_tracker(iv, 64, 2)
    sc = SCENES[0]
    nf = 64; nK = len(sc["kf_vecs"]); nF = len(sc["frame_vecs"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw, kv, kn = (t(a) for a in pack_vecs(sc["kf_vecs"], nf)); fw, fv, fn = (t(a) for a in pack_vecs(sc["frame_vecs"], nf))
    ng, kr, fr = t(sc["neigh"]), t(sc["kf_record"]), t(sc["frame_record"])
    cand = torch.zeros((nF, 2), dtype=torch.int32, device=dev); nc = torch.zeros(nF, dtype=torch.int32, device=dev)
    pairs = torch.zeros((nF * 2, 2), dtype=torch.int32, device=dev); sel = torch.zeros(nF * 2, dtype=torch.int32, device=dev)
    p = lambda x: None if x is None else x.data_ptr()

    def call(h=tr._h, voc=V._h, kw=kw, kv=kv, kn=kn, ng=ng, kr=kr, nK=nK, fw=fw, fv=fv, fn=fn, fr=fr, nF=nF, mc=2, cand=cand, nc=nc, pairs=pairs, sel=sel):
        return lib.ivf_tracker_reloc_candidates(h, voc, p(kw), p(kv), p(kn), None, p(ng), None, p(kr), nK, p(fw), p(fv), p(fn), p(fr), nF, mc,
                                                p(cand), p(nc), p(pairs), p(sel), None, None, None)
    assert call() == _lib.IVF_OK
    for bad in (dict(h=None), dict(voc=None), dict(kw=None), dict(kv=None), dict(kn=None), dict(ng=None), dict(kr=None), dict(fw=None), dict(fv=None),
                dict(fn=None), dict(fr=None), dict(cand=None), dict(nc=None), dict(pairs=None), dict(sel=None), dict(mc=0), dict(mc=-3), dict(nK=-1),
                dict(nF=-1)):
        assert call(**bad) == _lib.IVF_E_INVALID, bad
    # ivf_tracker_bow_vectors
    from iv_slam_amd import dist as ivd
    block = torch.from_numpy(ivd.pack_records([record_of(np.zeros((3, 32), np.uint8))], nf).reshape(-1)).to(dev)
    frames = torch.zeros(1, dtype=torch.int32, device=dev)
    w = torch.zeros((1, nf), dtype=torch.int32, device=dev); v = torch.zeros((1, nf), dtype=torch.float64, device=dev); n = torch.zeros(1, dtype=torch.int32, device=dev)

    def bow(h=tr._h, voc=V._h, block=block, rb=tr.record_bytes, nrec=1, frames=frames, nfr=1, w=w, v=v, n=n):
        return lib.ivf_tracker_bow_vectors(h, voc, p(block), rb, nrec, p(frames), nfr, p(w), p(v), p(n), None)
    assert bow() == _lib.IVF_OK
    for bad in (dict(h=None), dict(voc=None), dict(block=None), dict(frames=None), dict(w=None), dict(v=None), dict(n=None), dict(nfr=-1),
                dict(rb=tr.record_bytes + 8), dict(nrec=0)):
        assert bow(**bad) == _lib.IVF_E_INVALID, bad
    torch.cuda.synchronize()


def test_chain_bow_vectors_candidates_search_by_bow(iv):
    """records -> bow_vectors (keyframes and lost frames of one block) -> reloc_candidates -> search_by_bow with the produced d_pairs /
    d_select, all on one stream with no host read in between.  The block holds the keyframe and the frame of two matcher scenes of
    tests/track_bow_scenes.py; keyframe 2 has no gather record.  d_nmatches equals what the same pairs give when the table is built on
    the host from the restatement, and the lost frame of the main scene finds its keyframe"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    tree = S.TREES[3]; nf = S.NF
    scs = S.scenes(3)
    recs = S.records_of(scs[0]) + S.records_of(scs[2])                       # 0: keyframe, 1: frame (main); 2: keyframe, 3: frame (wide nodes)
    V = vocabulary(iv, tree)
    kf_rec = [0, 2, 0]; fr_rec = [1, 3]; mc = 3
    tr = make_tracker(iv, nf, len(fr_rec) * mc)
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    nK, nF = len(kf_rec), len(fr_rec)
    kw = torch.empty((nK, nf), dtype=torch.int32, device=dev); kv = torch.empty((nK, nf), dtype=torch.float64, device=dev); kn = torch.empty(nK, dtype=torch.int32, device=dev)
    fw = torch.empty((nF, nf), dtype=torch.int32, device=dev); fv = torch.empty((nF, nf), dtype=torch.float64, device=dev); fn = torch.empty(nF, dtype=torch.int32, device=dev)
    neigh = np.full((nK, 10), -1, np.int32); neigh[0, 0] = 1
    krec = np.array([0, 2, -1], np.int32)
    cand = torch.empty((nF, mc), dtype=torch.int32, device=dev); nc = torch.empty(nF, dtype=torch.int32, device=dev)
    pairs = torch.empty((nF * mc, 2), dtype=torch.int32, device=dev); sel = torch.empty(nF * mc, dtype=torch.int32, device=dev)
    assign = torch.full((nF * mc, nf), -7, dtype=torch.int32, device=dev); nm = torch.full((nF * mc,), -7, dtype=torch.int32, device=dev)
    tr.bow_vectors(V, block, t(kf_rec, torch.int32), kw, kv, kn)
    tr.bow_vectors(V, block, t(fr_rec, torch.int32), fw, fv, fn)
    tr.reloc_candidates(V, kw, kv, kn, torch.from_numpy(neigh).to(dev), torch.from_numpy(krec).to(dev), fw, fv, fn, t(fr_rec, torch.int32), cand, nc, pairs, sel)
    tr.search_by_bow(V, block, pairs, assign, nm, levelsup=1, select=sel)
    torch.cuda.synchronize()
    # the same table from the restatement on the host
    def vec_of(r):
        wid, _, wt = O.bow_transform(tree, recs[r]["desc"], 0)
        return R.bow_vector(wid, wt)
    kvecs = [vec_of(r) for r in kf_rec]
    hp = np.full((nF * mc, 2), -1, np.int32); hs = np.zeros(nF * mc, np.int32); hc = []
    for f, r in enumerate(fr_rec):
        res = R.detect(kvecs, neigh, vec_of(r))
        c, n, pr, s = R.outputs(res, krec, r, mc)
        hp[f * mc:(f + 1) * mc] = pr; hs[f * mc:(f + 1) * mc] = s; hc.append(res["cand"])
    assert pairs.cpu().numpy().tobytes() == hp.tobytes() and sel.cpu().numpy().tobytes() == hs.tobytes() and nc.cpu().tolist() == [len(c) for c in hc]
    assign2 = torch.full((nF * mc, nf), -7, dtype=torch.int32, device=dev); nm2 = torch.full((nF * mc,), -7, dtype=torch.int32, device=dev)
    tr.search_by_bow(V, block, torch.from_numpy(hp).to(dev), assign2, nm2, levelsup=1, select=torch.from_numpy(hs).to(dev))
    torch.cuda.synchronize()
    nm = nm.cpu().numpy()
    assert nm.tobytes() == nm2.cpu().numpy().tobytes() and assign.cpu().numpy().tobytes() == assign2.cpu().numpy().tobytes()
    slot = [j for j in range(mc) if hs[j] and hp[j, 0] == 0]
    assert slot and nm[slot[0]] == S.oracle(O, scs[0], 1)[1] and nm[slot[0]] > 20, "the main scene's lost frame finds its keyframe"
    assert (nm[hs == 0] == -2).all()
    print("chain: candidates %r, pairs %r, select %r, nmatches %r" % (hc, hp.tolist(), hs.tolist(), nm.tolist()))
