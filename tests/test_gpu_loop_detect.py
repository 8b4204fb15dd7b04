"""ivf_tracker_loop_candidates / ivf_tracker_loop_consistency (iv_slam_amd/csrc/ivf_track_loop.hip) -- LoopClosing::DetectLoop
(ORB/src/LoopClosing.cc:108-234) for a batch of new keyframes on the device -- through iv_slam_amd.LoopSearch against the restatement of
tests/loop_detect_ref.py on the hand-made scenes of tests/loop_detect_scenes.py.  Every comparison is bit for bit; what a call must
leave unwritten is prefilled with marks and compared too."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_detect_ref as L
import loop_detect_scenes as Z
import oracle_lib as O
import reloc_db_ref as R
import reloc_db_scenes as D
import track_bow_scenes as S
from test_gpu_track import scale_table, iv  # noqa: F401  (iv: the module fixture)
from test_gpu_track_bow import vocabulary, make_tracker
from test_gpu_reloc_db import device_candidates, expected as reloc_expected, pack_vecs

pytestmark = pytest.mark.gpu
F = np.float32
SCENES = Z.scenes() + [Z.sizes_scene()]
GROUP_SCENES = Z.group_scenes()
CAND_KEYS = ("min_score", "cand", "ncand", "scores", "common")
GROUP_KEYS = ("group_member", "group_size", "group_count", "n_groups", "enough", "nenough", "pairs", "select", "status")
MARK_F, MARK_I = 7.0, -7                                       # what the outputs hold before a call


def device_loop(iv, tr, sc, lists=None, with_optional=True, groups=None, calls=(1, 2)):
    """the scene through both calls on one stream (lists: the candidates given instead of call 1's) -> dict of every array written"""
    import torch
    dev = torch.device("cuda:0")
    ls = iv.LoopSearch(tr)
    nf = tr.nfeatures; nK = len(sc["kf_vecs"]); nQ = len(sc["queries"]); mc = sc["max_cand"]; gc, mem = sc["group_cap"], sc["member_cap"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev)
    start, conn = (t(a) for a in Z.csr(sc["conn"]))
    qk, qv, qs = (t(np.array([q[i] for q in sc["queries"]], np.int32)) for i in range(3))
    out = dict(min_score=full((nQ,), MARK_F, torch.float32), cand=full((nQ, mc), MARK_I, torch.int32), ncand=full((nQ,), MARK_I, torch.int32))
    if with_optional:
        out.update(scores=full((nQ, nK), MARK_F, torch.float32), common=full((nQ, nK), MARK_I, torch.int32))
    if lists is None and 1 in calls:
        kw, kv, kn = (t(a) for a in pack_vecs(sc["kf_vecs"], nf))
        ls.loop_candidates(kw, kv, kn, t(sc["neigh"]), start, conn, qk, qv, out["min_score"], out["cand"], out["ncand"],
                           kf_live=None if sc["live"] is None else t(sc["live"]), query_select=qs, scores=out.get("scores"), common=out.get("common"))
    elif lists is not None:
        c, n = L.cand_rows([None if x is None else dict(cand=x) for x in lists], mc)
        out["cand"], out["ncand"] = t(c), t(n)
    if 2 in calls:
        member, size, count, ng = (t(a) for a in L.pack_state(sc["groups"] if groups is None else groups, gc, mem))
        out.update(group_member=member, group_size=size, group_count=count, n_groups=ng, enough=full((nQ, mc), MARK_I, torch.int32),
                   nenough=full((nQ,), MARK_I, torch.int32), pairs=full((nQ, mc, 2), MARK_I, torch.int32), select=full((nQ, mc), MARK_I, torch.int32),
                   status=full((nQ,), MARK_I, torch.int32))
        ls.loop_consistency(t(sc["kf_record"]), start, conn, qk, out["cand"], out["ncand"], member, size, count, ng, out["enough"], out["nenough"],
                            out["pairs"], out["select"], out["status"], th=sc["th"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def expected(sc, lists=None, groups=None):
    """the same arrays from the restatement"""
    nK = len(sc["kf_vecs"]); nQ = len(sc["queries"]); mc = sc["max_cand"]
    e = {}
    if lists is None:
        res = Z.run(sc)
        e["cand"], e["ncand"] = L.cand_rows(res, mc)
        e["min_score"] = np.full(nQ, MARK_F, F); e["scores"] = np.full((nQ, nK), MARK_F, F); e["common"] = np.full((nQ, nK), MARK_I, np.int32)
        for i, r in enumerate(res):
            if isinstance(r, dict):
                e["min_score"][i] = r["min_score"]; e["scores"][i] = r["scores"]; e["common"][i] = r["common"]
    else:
        res = lists
        e["cand"], e["ncand"] = L.cand_rows([None if x is None else dict(cand=x) for x in lists], mc)
    state, out = Z.run_groups(dict(sc, groups=sc["groups"] if groups is None else groups), res)
    e["group_member"], e["group_size"], e["group_count"], e["n_groups"] = L.pack_state(state, sc["group_cap"], sc["member_cap"])
    e.update(out)
    return e, state


def assert_equal(got, want, keys, what):
    for k in keys:
        assert got[k].tobytes() == want[k].tobytes(), "%s %s:\n%r\n%r" % (what, k, got[k], want[k])


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scenes_equal_the_restatement(iv, sc):
    """every candidate scene through both calls (the sizes scene: minScore at query and connected vectors of 0, 1, 63, 64, 65 and 130
    words): all outputs, the -0.0f bits of min_score, the optional arrays, the group state and the status equal the restatement byte
    for byte; a second run on the handle is byte-identical and so are the outputs without the optional arrays"""
    tr = make_tracker(iv, sc["nf"], 2)
    got = device_loop(iv, tr, sc)
    want, _ = expected(sc)
    assert_equal(got, want, CAND_KEYS + GROUP_KEYS, sc["name"])
    if sc["name"] == "zero":
        assert got["min_score"][:2].view(np.uint32).tolist() == [0x80000000, 0x80000000] and got["ncand"].tolist() == [1, 0, -2, -1]
    if sc["name"] == "sizes":
        assert (got["min_score"][1:] < 1).all() and got["min_score"][0].view(np.uint32) == 0x80000000
    again = device_loop(iv, tr, sc)
    bare = device_loop(iv, tr, sc, with_optional=False)
    for k in got:
        assert again[k].tobytes() == got[k].tobytes() and (k not in bare or bare[k].tobytes() == got[k].tobytes()), k


@pytest.mark.parametrize("sc", GROUP_SCENES, ids=[s["name"] for s in GROUP_SCENES])
def test_group_scenes_equal_the_restatement(iv, sc):
    """the consistency call on given candidate lists: the state arrays (rows beyond n_groups cleared), enough, pairs, select and status"""
    tr = make_tracker(iv, 64, 2)
    got = device_loop(iv, tr, sc, lists=sc["lists"])
    want, state = expected(sc, lists=sc["lists"])
    assert_equal(got, want, GROUP_KEYS, sc["name"])
    if sc["want_groups"] is not None:
        assert [(sorted(g), c) for g, c in state] == [(sorted(g), c) for g, c in sc["want_groups"]]


def test_four_queries_in_one_call_equal_four_calls(iv):
    sc = [s for s in GROUP_SCENES if s["name"] == "four_in_sequence"][0]
    tr = make_tracker(iv, 64, 2)
    whole = device_loop(iv, tr, sc, lists=sc["lists"])
    groups = list(sc["groups"])
    for i in range(4):
        one = dict(sc, queries=sc["queries"][i:i + 1])
        got = device_loop(iv, tr, one, lists=sc["lists"][i:i + 1], groups=groups)
        for k in ("enough", "nenough", "pairs", "select", "status"):
            assert got[k].tobytes() == whole[k][i:i + 1].tobytes(), (i, k)
        groups = [(set(int(m) for m in got["group_member"][e, :got["group_size"][e]]), int(got["group_count"][e])) for e in range(int(got["n_groups"][0]))]
    for k in ("group_member", "group_size", "group_count", "n_groups"):
        assert got[k].tobytes() == whole[k].tobytes(), k
    assert whole["nenough"].tolist() == [0, 0, 0, 1]


def test_one_handle_grows_its_scratch_and_takes_an_empty_database(iv):
    """a small scene, then the 68-keyframe batch, then the small one again on ONE handle, each equal to the restatement and to a fresh
    handle; then a database of no keyframes and a call of no queries"""
    import torch
    by_name = {s["name"]: s for s in SCENES}
    tr = make_tracker(iv, 256, 2)
    for name in ("connected", "threshold", "batch", "connected"):
        sc = dict(by_name[name], nf=256)
        got = device_loop(iv, tr, sc)
        assert_equal(got, expected(sc)[0], CAND_KEYS + GROUP_KEYS, name)
        fresh = device_loop(iv, make_tracker(iv, 256, 2), sc)
        assert_equal(got, fresh, CAND_KEYS + GROUP_KEYS, name + " on a fresh handle")
    empty = Z.scene("empty", [], [(0, 0, 1), (0, 0, 0)], nf=256)
    empty["groups"] = [({1, 2}, 1)]
    got = device_loop(iv, tr, empty)
    assert got["ncand"].tolist() == [-1, -2] and (got["cand"] == MARK_I).all() and (got["min_score"] == MARK_F).all()
    assert got["n_groups"].tolist() == [1] and got["nenough"].tolist() == [0, 0] and got["status"].tolist() == [0, 0] and (got["select"] == 0).all()
    none = dict(by_name["connected"], queries=[], nf=256)
    got = device_loop(iv, tr, none)
    assert got["ncand"].size == 0 and got["n_groups"].tolist() == [0]


def test_argument_errors(iv):
    """IVF_E_INVALID before any launch: null arrays, negative counts, max_candidates / group_cap / member_cap < 1"""
    import torch
    from iv_slam_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    tr = make_tracker(iv, 64, 2)
    sc = SCENES[0]
    nf = 64; nK = len(sc["kf_vecs"]); nQ = 1; mc, gc, mem = 2, 3, 4
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    kw, kv, kn = (t(a) for a in pack_vecs(sc["kf_vecs"], nf))
    start, conn = (t(a) for a in Z.csr(sc["conn"]))
    ng, kr, qk, qv = t(sc["neigh"]), t(sc["kf_record"]), t(np.array([4], np.int32)), t(np.array([4], np.int32))
    ms = torch.zeros(nQ, dtype=torch.float32, device=dev)
    cand, nc, gm, gs, gcnt, n, en, nen, pairs, sel, status = z(nQ, mc), z(nQ), z(gc, mem), z(gc), z(gc), z(1), z(nQ, mc), z(nQ), z(nQ, mc, 2), z(nQ, mc), z(nQ)
    p = lambda x: None if x is None else x.data_ptr()

    def candidates(h=tr._h, kw=kw, kv=kv, kn=kn, ng=ng, nK=nK, start=start, conn=conn, nconn=conn.numel(), qk=qk, qv=qv, nQ=nQ, mc=mc, ms=ms, cand=cand, nc=nc):
        return lib.ivf_tracker_loop_candidates(h, p(kw), p(kv), p(kn), None, p(ng), nK, p(start), p(conn), nconn, p(qk), p(qv), None, nQ, mc, p(ms), p(cand),
                                               p(nc), None, None, None)
    assert candidates() == _lib.IVF_OK
    for bad in (dict(h=None), dict(kw=None), dict(kv=None), dict(kn=None), dict(ng=None), dict(start=None), dict(conn=None), dict(qk=None), dict(qv=None),
                dict(ms=None), dict(cand=None), dict(nc=None), dict(mc=0), dict(mc=-3), dict(nK=-1), dict(nQ=-1), dict(nconn=-1)):
        assert candidates(**bad) == _lib.IVF_E_INVALID, bad

    def consistency(h=tr._h, kr=kr, nK=nK, start=start, conn=conn, nconn=conn.numel(), qk=qk, nQ=nQ, cand=cand, nc=nc, mc=mc, gm=gm, gs=gs, gcnt=gcnt, n=n,
                    gc=gc, mem=mem, en=en, nen=nen, pairs=pairs, sel=sel, status=status):
        return lib.ivf_tracker_loop_consistency(h, p(kr), nK, p(start), p(conn), nconn, p(qk), nQ, p(cand), p(nc), mc, 3, p(gm), p(gs), p(gcnt), p(n), gc, mem,
                                                p(en), p(nen), p(pairs), p(sel), p(status), None)
    assert consistency() == _lib.IVF_OK
    for bad in (dict(h=None), dict(kr=None), dict(start=None), dict(conn=None), dict(qk=None), dict(cand=None), dict(nc=None), dict(gm=None), dict(gs=None),
                dict(gcnt=None), dict(n=None), dict(en=None), dict(nen=None), dict(pairs=None), dict(sel=None), dict(status=None), dict(mc=0), dict(gc=0),
                dict(mem=0), dict(mem=-2), dict(nK=-1), dict(nQ=-1), dict(nconn=-1)):
        assert consistency(**bad) == _lib.IVF_E_INVALID, bad
    torch.cuda.synchronize()


def test_reloc_candidates_before_and_after_a_loop_call_on_the_handle(iv):
    """the two queries share the handle's scratch: ivf_tracker_reloc_candidates on the neighbour scene of tests/reloc_db_scenes.py gives
    the same bytes before and after a loop call (which marks connected cells in that scratch) on the same handle"""
    rsc = D.neighbour_scene(0.9)
    V = vocabulary(iv, rsc["tree"])
    tr = make_tracker(iv, 256, 2)
    before = device_candidates(iv, tr, V, rsc, rsc["frame_vecs"])
    want = reloc_expected(rsc, rsc["frame_vecs"])
    for name in ("batch", "connected"):
        sc = dict([s for s in SCENES if s["name"] == name][0], nf=256)
        assert_equal(device_loop(iv, tr, sc), expected(sc)[0], CAND_KEYS + GROUP_KEYS, name)
        after = device_candidates(iv, tr, V, rsc, rsc["frame_vecs"])
        for k in want:
            assert before[k].tobytes() == after[k].tobytes() == want[k].tobytes(), (name, k)


def test_chain_bow_vectors_candidates_consistency_search_by_bow_keyframes(iv):
    """records -> bow_vectors (the database rows, the current keyframes among them) -> loop_candidates -> loop_consistency ->
    search_by_bow_keyframes with the produced pairs / select, on one stream with no host read in between.  Four keyframes: 0 and 1 the
    keyframes of two matcher scenes of tests/track_bow_scenes.py, 2 and 3 their frames, appended and queried with visible = their index;
    each query is connected to the other scene's keyframe (a low minScore).  The groups start with the two old keyframes at counter 0
    and th = 1, so a candidate is enough-consistent at once.  Everything equals the per-step restatements, the search equals the same
    table fed from the host, and keyframe 2 finds keyframe 0."""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    tree = S.TREES[3]; nf = S.NF
    scs = S.scenes(3)
    recs = S.records_of(scs[0]) + S.records_of(scs[2])                       # records 0: keyframe, 1: frame (main); 2: keyframe, 3: frame (wide nodes)
    kf_rec = [0, 2, 1, 3]; nK = 4; mc = 2; gc, mem = 4, 4
    V = vocabulary(iv, tree)
    tr = make_tracker(iv, nf, 2 * mc); ls = iv.LoopSearch(tr)
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    t = lambda a, dt=torch.int32: torch.tensor(a, dtype=dt, device=dev)
    conn_rows = [[], [], [1], [0]]
    sc = Z.scene("chain", [[]] * nK, [(2, 2, 1), (3, 3, 1)], conn={2: [1], 3: [0]}, kf_record=kf_rec, max_cand=mc, nf=nf, th=1, group_cap=gc, member_cap=mem)
    sc["groups"] = [({0}, 0), ({1}, 0)]
    start, conn = (torch.from_numpy(a).to(dev) for a in Z.csr(conn_rows))
    kw = torch.empty((nK, nf), dtype=torch.int32, device=dev); kv = torch.empty((nK, nf), dtype=torch.float64, device=dev); kn = torch.empty(nK, dtype=torch.int32, device=dev)
    neigh = torch.full((nK, 10), -1, dtype=torch.int32, device=dev)
    ms = torch.empty(2, dtype=torch.float32, device=dev); cand = torch.empty((2, mc), dtype=torch.int32, device=dev); nc = torch.empty(2, dtype=torch.int32, device=dev)
    member, size, count, ng = (torch.from_numpy(a).to(dev) for a in L.pack_state(sc["groups"], gc, mem))
    en = torch.empty((2, mc), dtype=torch.int32, device=dev); nen = torch.empty(2, dtype=torch.int32, device=dev)
    pairs = torch.empty((2, mc, 2), dtype=torch.int32, device=dev); sel = torch.empty((2, mc), dtype=torch.int32, device=dev); status = torch.empty(2, dtype=torch.int32, device=dev)
    m12 = torch.full((2 * mc, nf), -7, dtype=torch.int32, device=dev); nm = torch.full((2 * mc,), -7, dtype=torch.int32, device=dev)
    qk = t([2, 3])
    tr.bow_vectors(V, block, t(kf_rec), kw, kv, kn)
    ls.loop_candidates(kw, kv, kn, neigh, start, conn, qk, t([2, 3]), ms, cand, nc)
    ls.loop_consistency(t(kf_rec), start, conn, qk, cand, nc, member, size, count, ng, en, nen, pairs, sel, status, th=1)
    ls.search_by_bow_keyframes(V, block, pairs.view(-1, 2), m12, nm, levelsup=1, select=sel.view(-1))
    torch.cuda.synchronize()
    # the per-step restatements
    def vec_of(r):
        wid, _, wt = O.bow_transform(tree, recs[r]["desc"], 0)
        return R.bow_vector(wid, wt)
    sc["kf_vecs"] = [vec_of(r) for r in kf_rec]
    want, _ = expected(sc)
    got = dict(min_score=ms, cand=cand, ncand=nc, group_member=member, group_size=size, group_count=count, n_groups=ng, enough=en, nenough=nen, pairs=pairs,
               select=sel, status=status)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert_equal(got, want, tuple(got), "chain")
    m12h = torch.full((2 * mc, nf), -7, dtype=torch.int32, device=dev); nmh = torch.full((2 * mc,), -7, dtype=torch.int32, device=dev)
    ls.search_by_bow_keyframes(V, block, torch.from_numpy(want["pairs"].reshape(-1, 2)).to(dev), m12h, nmh, levelsup=1,
                               select=torch.from_numpy(want["select"].reshape(-1)).to(dev))
    torch.cuda.synchronize()
    nm = nm.cpu().numpy()
    assert nm.tobytes() == nmh.cpu().numpy().tobytes() and m12.cpu().numpy().tobytes() == m12h.cpu().numpy().tobytes()
    assert got["enough"][0, 0] == 0 and got["pairs"][0, 0].tolist() == [1, 0] and got["select"][0, 0] == 1 and nm[0] > 20, "keyframe 2 (record 1) finds keyframe 0 (record 0)"
    assert (nm[want["select"].reshape(-1) == 0] == -2).all()
