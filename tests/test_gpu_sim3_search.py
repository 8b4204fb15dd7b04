"""ivf_tracker_search_by_bow_keyframes (iv_slam_amd/csrc/ivf_track_bow.hip) and ivf_tracker_search_by_sim3 (ivf_track_sim3.hip) -- the two
searches of LoopClosing::ComputeSim3 around the batched Sim3Solver -- through iv_slam_amd.LoopSearch, against tests/sim3_search_ref.py on
the hand-made scenes of tests/sim3_search_scenes.py.  Both searches produce integers only: match12 / nmatches and matches / nfound /
match1 / match2 must be EQUAL to the restatement's on every scene, alone and all in one call, and to the per-call
ivf_search_by_bow_keyframes / ivf_search_by_sim3 fed with the same feature vectors / the restatement's projections.  They can be equal
because tests/test_sim3_search_cpu.py keeps every gate of every scene on its boundary bit for bit (exact scenes) or further from it than
64 x the f32 - f64 spread (generic scenes).  Outputs are pre-filled with sentinels: a pair left out or with a record outside the block
writes its count (-2 / -1) and nothing else.  nfeatures is sim3_scenes.NF = 128 except where a scene needs more keypoints than that (a
window or a node of 130): 256 there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_scenes as S
import sim3_search_scenes as SC
from test_gpu_track import iv  # noqa: F401  (the module fixture)
from test_sim3_search_cpu import BOW, SCENES, bow_ref, ref

pytestmark = pytest.mark.gpu
F = np.float32
FILL = -7
LP = SC.LOCAL_POINT_DTYPE
MAX_PAIRS = 8


def make_tracker(iv, cam, nf, max_pairs=MAX_PAIRS):
    return iv.BatchTracker(nf, SC.S.SCALE, float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam["bf"]), cam["bounds"], max_pairs=max_pairs)


_TRACKERS = {}


def tracker_for(iv, cam, nf):
    key = (float(cam["fx"]), nf)
    if key not in _TRACKERS:
        _TRACKERS[key] = make_tracker(iv, cam, nf)
    return _TRACKERS[key]


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def record_of(kf):
    n = kf["n"]
    return dict(kps=kf["kps"], desc=kf["desc"], uright=np.full(n, -1.0, F), depth=np.full(n, -1.0, F))


def run_sim3(iv, scs, tracker=None, stream=False, diag=True, order=None, bad=(), unselected=(), sim3_override=None, pose_override=None, th=None):
    """the scenes scs (one camera, one nf) as the pairs of ONE call -> dict of numpy outputs [n_pairs, ...]"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    order = list(range(len(scs))) if order is None else list(order)
    scs = [scs[k] for k in order]
    n, nf, cam = len(scs), scs[0]["nf"], scs[0]["cam"]
    recs = []; pairs = []
    poses = np.zeros((2 * n, 12), F); pts = np.zeros((2 * n, nf), LP); pts["flags"] = 1
    sim3 = np.zeros((n, 16), F); m12 = np.full((n, nf), -1, np.int32); inl = np.ones((n, nf), np.uint8)
    for j, sc in enumerate(scs):
        for side, kf in enumerate((sc["kf1"], sc["kf2"])):
            r = 2 * j + side
            recs.append(record_of(kf)); poses[r] = kf["pose"]; pts[r, :kf["n"]] = kf["points"]
            pts[r, kf["n"]:]["flags"] = 0; pts["pos"][r, kf["n"]:] = (0.0, 0.0, 8.0); pts["max_distance"][r, kf["n"]:] = 8.0   # a live point past the count: never read
        pairs.append((2 * j, 2 * n + 3 if sc["name"] in bad else 2 * j + 1))
        sim3[j] = sc["sim3"]; m12[j] = sc["match12"]
        if sc["inlier"] is not None:
            inl[j] = sc["inlier"]
    if sim3_override is not None:
        sim3[:] = sim3_override
    if pose_override is not None:
        poses[:] = pose_override
    sel = np.array([int(sc["name"] not in unselected) for sc in scs], np.int32)
    tr = tracker or tracker_for(iv, cam, nf)
    ls = iv.LoopSearch(tr)
    block = up(ivd.pack_records(recs, nf).reshape(-1))
    d = dict(matches=torch.full((n, nf), FILL, dtype=torch.int32, device=dev), nfound=torch.full((n,), FILL, dtype=torch.int32, device=dev),
             match1=torch.full((n, nf), FILL, dtype=torch.int32, device=dev), match2=torch.full((n, nf), FILL, dtype=torch.int32, device=dev))
    use_inl = any(sc["inlier"] is not None for sc in scs)
    st = torch.cuda.Stream() if stream else None
    args = (block, up(np.array(pairs, np.int32)), up(poses), up(pts.view(np.uint8).reshape(-1)), up(sim3), up(m12), d["matches"], d["nfound"])
    if st is not None:
        st.wait_stream(torch.cuda.current_stream())
    ls.search_by_sim3(*args, th=scs[0]["th"] if th is None else th, select=None if sel.all() else up(sel), inlier=up(inl) if use_inl else None,
                      match1=d["match1"] if diag else None, match2=d["match2"] if diag else None, stream_ptr=st.cuda_stream if st is not None else None)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    back = np.argsort(order)
    return {k: v[back] for k, v in out.items()}


def compare_sim3(sc, g, j, diag=True):
    o = ref(sc["name"])
    assert g["nfound"][j] == o["nfound"], "%s: nfound %d, the restatement %d" % (sc["name"], g["nfound"][j], o["nfound"])
    for key in ("matches", "match1", "match2") if diag else ("matches",):
        assert np.array_equal(g[key][j], o[key]), "%s: %s differs at %r" % (sc["name"], key, np.nonzero(g[key][j] != o[key])[0][:8])


def groups():
    g = {}
    for name in sorted(SCENES):
        g.setdefault((SCENES[name]["kind"], SCENES[name]["nf"]), []).append(name)
    return [v[i:i + MAX_PAIRS] for v in g.values() for i in range(0, len(v), MAX_PAIRS)]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_sim3_scene_alone(iv, name):
    """every scene of tests/sim3_search_scenes.py in a call of its own: the image edges, the sign of the depth, the range ends, the window's
    radius, the octaves, TH_HIGH, equal distances, the agreement check, the already-matched sets, the inlier filter, a bad point, a match
    past KF2's count, windows of 65 and 130 candidates, empty and full records, the planted similarities"""
    sc = SCENES[name]
    compare_sim3(sc, run_sim3(iv, [sc]), 0)


_GROUP = {}


def group_run(iv, names):
    key = tuple(names)
    if key not in _GROUP:
        _GROUP[key] = run_sim3(iv, [SCENES[n] for n in names])
    return _GROUP[key]


@pytest.mark.parametrize("names", groups(), ids=lambda g: g[0] + "+%d" % (len(g) - 1))
def test_sim3_scenes_in_one_call(iv, names):
    g = group_run(iv, names)
    for j, name in enumerate(names):
        compare_sim3(SCENES[name], g, j)


@pytest.mark.parametrize("name", sorted(n for n, s in SCENES.items() if s["kf1"]["n"] and s["kf2"]["n"]))      # the per-call search takes no empty keyframe
def test_sim3_equals_the_per_call_search_on_the_restatements_projections(iv, name):
    sc, o = SCENES[name], ref(name)
    k1, k2 = sc["kf1"], sc["kf2"]
    m, nfound = iv.ORBmatcher(0.75, True).SearchBySim3(k1["kps"], k1["desc"], sc["cam"]["bounds"], k2["kps"], k2["desc"], sc["cam"]["bounds"], o["q12"], o["q21"])
    g = run_sim3(iv, [sc])
    new = g["matches"][0][:k1["n"]].copy()
    new[o["m_in"] >= 0] = -1                                                # the per-call search returns the new matches only
    assert nfound == g["nfound"][0] and np.array_equal(m, new), name


def test_sim3_unselected_and_out_of_range_pairs_are_left_untouched(iv):
    names = groups()[0]
    g = run_sim3(iv, [SCENES[n] for n in names], bad=names[1:2], unselected=names[2:3])
    for j, name in enumerate(names):
        if j in (1, 2):
            assert g["nfound"][j] == (-1 if j == 1 else -2), name
            assert all((g[k][j] == FILL).all() for k in ("matches", "match1", "match2")), name
        else:
            compare_sim3(SCENES[name], g, j)


def test_sim3_runs_are_bit_identical_on_any_stream_in_any_pair_order_and_without_the_diagnostics(iv):
    for names in groups()[:2]:
        scs = [SCENES[n] for n in names]
        a = group_run(iv, names)
        tr = make_tracker(iv, scs[0]["cam"], scs[0]["nf"])
        b = run_sim3(iv, scs, tracker=tr)
        c = run_sim3(iv, scs, tracker=tr, stream=True)
        d = run_sim3(iv, scs, tracker=tr, order=list(range(len(scs)))[::-1])
        e = run_sim3(iv, scs, diag=False)
        for key in ("matches", "nfound", "match1", "match2"):
            assert a[key].tobytes() == b[key].tobytes(), "%s differs between two runs" % key
            assert a[key].tobytes() == c[key].tobytes(), "%s differs on a non-default stream" % key
            assert a[key].tobytes() == d[key].tobytes(), "%s differs under another pair order" % key
        assert a["matches"].tobytes() == e["matches"].tobytes() and a["nfound"].tobytes() == e["nfound"].tobytes()
        assert (e["match1"] == FILL).all() and (e["match2"] == FILL).all()


def test_sim3_nan_similarity_and_nan_pose_return_with_nothing_found(iv):
    sc = SCENES["planted"]
    nan16 = np.full(16, np.nan, F)
    for g in (run_sim3(iv, [sc], sim3_override=nan16), run_sim3(iv, [sc], pose_override=np.full(12, np.nan, F))):
        assert g["nfound"][0] == 0 and (g["matches"][0] == -1).all() and (g["match1"][0] == -1).all() and (g["match2"][0] == -1).all()


def test_sim3_arguments_are_checked(iv):
    import torch
    sc = SCENES["planted"]
    with pytest.raises(iv.IvfError):
        run_sim3(iv, [sc], th=0.0)
    with pytest.raises(iv.IvfError):
        run_sim3(iv, [sc, sc], tracker=make_tracker(iv, sc["cam"], sc["nf"], max_pairs=1))      # n_pairs > max_pairs
    tr = tracker_for(iv, sc["cam"], sc["nf"]); ls = iv.LoopSearch(tr)
    from iv_slam_amd import dist as ivd
    block = up(ivd.pack_records([record_of(sc["kf1"]), record_of(sc["kf2"])], sc["nf"]).reshape(-1))
    m = up(np.full((1, sc["nf"]), -1, np.int32)); nfd = torch.zeros(1, dtype=torch.int32, device=m.device)
    pts = up(np.zeros((2, sc["nf"]), LP).view(np.uint8).reshape(-1))
    with pytest.raises(iv.IvfError):                                                           # matches may not alias match12
        ls.search_by_sim3(block, up(np.array([[0, 1]], np.int32)), up(np.zeros((2, 12), F)), pts, up(np.zeros((1, 16), F)), m, m, nfd)


# ---- SearchByBoW(KF, KF) --------------------------------------------------------------------------------------------------------------
def run_bow(iv, scs, tracker=None, stream=False, order=None, bad=(), unselected=(), flags=True, nn_ratio=SC.NN_RATIO, check_orientation=True, levelsup=None):
    import torch
    from iv_slam_amd import dist as ivd
    from test_gpu_track_bow import vocabulary
    dev = torch.device("cuda:0")
    order = list(range(len(scs))) if order is None else list(order)
    scs = [scs[k] for k in order]
    n, nf = len(scs), SC.NF_BOW
    recs = []; pairs = []; fl = np.zeros((2 * n, nf), np.uint8)
    for j, sc in enumerate(scs):
        for side, kf in enumerate((sc["kf1"], sc["kf2"])):
            has = kf["has"]
            # bit 1 is not this call's; without flags a keypoint holds a point where it has a stereo depth
            fl[2 * j + side, :kf["n"]] = has | 2; fl[2 * j + side, kf["n"]:] = 1
            recs.append(dict(kps=kf["kps"], desc=kf["desc"], uright=np.full(kf["n"], -1.0, F), depth=np.where(has != 0, 8.0, -1.0).astype(F)))
        pairs.append((2 * j, 2 * n + 3 if sc["name"] in bad else 2 * j + 1))
    sel = np.array([int(sc["name"] not in unselected) for sc in scs], np.int32)
    tr = tracker or tracker_for(iv, SC.GENERIC_CAM, nf)
    V = vocabulary(iv, scs[0]["tree"])
    m12 = torch.full((n, nf), FILL, dtype=torch.int32, device=dev); nm = torch.full((n,), FILL, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream() if stream else None
    if st is not None:
        st.wait_stream(torch.cuda.current_stream())
    iv.LoopSearch(tr).search_by_bow_keyframes(V, up(ivd.pack_records(recs, nf).reshape(-1)), up(np.array(pairs, np.int32)), m12, nm,
                                              levelsup=scs[0]["levelsup"] if levelsup is None else levelsup, select=None if sel.all() else up(sel),
                                              point_flags=up(fl) if flags else None, nn_ratio=nn_ratio, check_orientation=check_orientation,
                                              stream_ptr=st.cuda_stream if st is not None else None)
    torch.cuda.synchronize()
    back = np.argsort(order)
    return m12.cpu().numpy()[back], nm.cpu().numpy()[back]


@pytest.mark.parametrize("check_orientation", [True, False])
@pytest.mark.parametrize("name", sorted(BOW))
def test_bow_scene_alone_equals_the_restatement_and_the_per_call_search(iv, name, check_orientation):
    """nodes of 1, 64, 65 and 130 features on either side, a node on one side only, bestDist1 49 and 50, the ratio on its edge, a KF2
    feature without a point, two KF1 features after one KF2 feature, a removed rotation bin, empty records; with flags and without"""
    sc = BOW[name]
    want, nm, _, _, (fv1, fv2) = bow_ref(name, check_orientation=check_orientation)
    for flags in (True, False):
        g, gn = run_bow(iv, [sc], flags=flags, check_orientation=check_orientation)
        assert gn[0] == nm and np.array_equal(g[0], want), "%s (flags %r): differs at %r" % (name, flags, np.nonzero(g[0] != want)[0][:8])
    k1, k2 = sc["kf1"], sc["kf2"]
    if k1["n"] and k2["n"]:
        V = __import__("test_gpu_track_bow").vocabulary(iv, sc["tree"])
        f1 = V.transform(k1["desc"], sc["levelsup"])[1]; f2 = V.transform(k2["desc"], sc["levelsup"])[1]
        assert {k: list(v) for k, v in f1.items()} == fv1 and {k: list(v) for k, v in f2.items()} == fv2, name
        m, n = iv.ORBmatcher(SC.NN_RATIO, check_orientation).SearchByBoWKeyFrames(k1["kps"], k1["desc"], k1["has"], f1, k2["kps"], k2["desc"], k2["has"], f2)
        assert n == nm and np.array_equal(m, want[:k1["n"]]), name


def test_bow_scenes_in_one_call_left_out_pairs_and_repeatability(iv):
    names = sorted(BOW)
    scs = [BOW[n] for n in names]
    a = run_bow(iv, scs)
    for j, name in enumerate(names):
        want, nm = bow_ref(name)[:2]
        assert a[1][j] == nm and np.array_equal(a[0][j], want), name
    tr = make_tracker(iv, SC.GENERIC_CAM, SC.NF_BOW)
    for other in (run_bow(iv, scs, tracker=tr), run_bow(iv, scs, tracker=tr, stream=True), run_bow(iv, scs, tracker=tr, order=list(range(len(scs)))[::-1])):
        assert a[0].tobytes() == other[0].tobytes() and a[1].tobytes() == other[1].tobytes()
    g, gn = run_bow(iv, scs, bad=names[1:2], unselected=names[2:3])
    assert gn[1] == -1 and gn[2] == -2 and (g[1] == FILL).all() and (g[2] == FILL).all()
    keep = [j for j in range(len(names)) if j not in (1, 2)]
    assert np.array_equal(g[keep], a[0][keep]) and np.array_equal(gn[keep], a[1][keep])
    # every feature in node 0 (levelsup = L): one long chain on both sides
    for name in ("bow_gates", "bow_wide_kf1"):
        sc = BOW[name]
        want, nm = SC_ref_at(sc, sc["tree"]["depth"])
        g, gn = run_bow(iv, [sc], levelsup=sc["tree"]["depth"])
        assert gn[0] == nm and np.array_equal(g[0], want), name


def SC_ref_at(sc, levelsup):
    import sim3_search_ref as R
    return R.search_by_bow_keyframes(sc["tree"], levelsup, sc["kf1"], sc["kf1"]["has"], sc["kf2"], sc["kf2"]["has"], SC.NN_RATIO, True, nf=sc["nf"])[:2]


def test_bow_arguments_are_checked(iv):
    sc = BOW["bow_gates"]
    for bad in (dict(nn_ratio=0.0), dict(levelsup=-1)):
        with pytest.raises(iv.IvfError):
            run_bow(iv, [sc], **bad)
    with pytest.raises(iv.IvfError):
        run_bow(iv, [sc, sc], tracker=make_tracker(iv, SC.GENERIC_CAM, SC.NF_BOW, max_pairs=1))


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def test_chain_search_by_bow_keyframes_solve_sim3_search_by_sim3_without_the_host(iv):
    """the chain of tests/test_gpu_sim3.py with both host steps replaced: LoopSearch.search_by_bow_keyframes -> solve_sim3 ->
    LoopSearch.search_by_sim3 on two synthetic keyframes related by a known similarity (s = 1.2, fix_scale 0); match12 stays on the device,
    select is (ninliers > 0) computed there; all 60 correspondences come out, with no .cpu() between the calls"""
    import torch
    from iv_slam_amd import dist as ivd, track
    from test_gpu_track_bow import vocabulary
    import track_bow_scenes as TB
    dev = torch.device("cuda:0")
    sc = SC.generic_scene("chain", 73)
    n, perm, nf = sc["kf1"]["n"], sc["perm"], SC.NF
    # descriptors the vocabulary sends to one node: two thirds of the points (the BoW search sees them), the others to a stopped word's leaf
    tree = TB.TREES[3]
    b = TB.Builder(tree, 5)
    known = np.arange(n) % 3 != 0
    stopped = TB.path_to(tree, tree["stopped"]); node = b.node()
    desc1 = np.stack([b.desc(node if known[i] else stopped, b.payload()) for i in range(n)])
    for kf, slot in ((sc["kf1"], np.arange(n)), (sc["kf2"], perm)):
        d = np.zeros((n, 32), np.uint8); d[slot] = desc1
        kf["desc"] = d; kf["points"]["desc"] = d
    tr = make_tracker(iv, SC.GENERIC_CAM, nf, max_pairs=1)
    ls = iv.LoopSearch(tr)
    block = up(ivd.pack_records([record_of(sc["kf1"]), record_of(sc["kf2"])], nf).reshape(-1))
    pairs = up(np.array([[0, 1]], np.int32))
    flags = np.zeros((2, nf), np.uint8); flags[:, :n] = 1
    xw = np.zeros((2, nf, 3), F); pts = np.zeros((2, nf), LP); pts["flags"] = 1
    for r, kf in enumerate((sc["kf1"], sc["kf2"])):
        xw[r, :n] = kf["points"]["pos"]; pts[r, :n] = kf["points"]
    poses = up(np.stack([sc["kf1"]["pose"], sc["kf2"]["pose"]]))
    dflags, dxw, dpts = up(flags), up(xw), up(pts.view(np.uint8).reshape(-1))
    draws = up(track.sim3_draws(1, 300, 4).view(np.int32))
    i32 = lambda *s: torch.full(s, FILL, dtype=torch.int32, device=dev)
    m12, nm, ninl, matches, nfound = i32(1, nf), i32(1), i32(1), i32(1, nf), i32(1)
    sim3 = torch.zeros((1, 16), dtype=torch.float32, device=dev); inl = torch.zeros((1, nf), dtype=torch.uint8, device=dev)
    ls.search_by_bow_keyframes(vocabulary(iv, tree), block, pairs, m12, nm, levelsup=1, point_flags=dflags)
    tr.solve_sim3(block, pairs, poses, dxw, dflags, m12, draws, sim3, inl, ninl, fix_scale=False)
    ls.search_by_sim3(block, pairs, poses, dpts, sim3, m12, matches, nfound, select=(ninl > 0).to(torch.int32), inlier=inl)
    torch.cuda.synchronize()
    m12, nm, ninl, matches, nfound = (x.cpu().numpy() for x in (m12, nm, ninl, matches, nfound))
    print("chain: %d BoW matches, %d inliers, %d found by SearchBySim3" % (nm[0], ninl[0], nfound[0]))
    assert nm[0] == known.sum() and np.array_equal(m12[0, :n][known], perm[known]) and (m12[0, :n][~known] == -1).all()
    assert ninl[0] == known.sum()
    assert nfound[0] == (~known).sum() and np.array_equal(matches[0, :n], perm) and (matches[0, n:] == -1).all()
