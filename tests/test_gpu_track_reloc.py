"""ivf_tracker_search_reloc / ivf_tracker_filter_assign (iv_slam_amd/csrc/ivf_track_reloc.hip) -- ORBmatcher::SearchByProjection(CurrentFrame,
pKF, sAlreadyFound, th, ORBdist) (ORB/src/ORBmatcher.cc:1520-1652) and the set bookkeeping of Tracking::Relocalization around it
(ORB/src/Tracking.cc:2351-2404), batched on the tracker handle.  Bar: d_assign, d_nmatches and the quality arrays IDENTICAL to
oracle/projection_oracle.py:search_reloc around the C oracle, element for element, on the hand-made scenes of tests/reloc_scenes.py, on a seeded
random sweep with overflowing windows, and at every search of the relocalization chain run without a host synchronisation between its steps."""
import os
import sys
import types

import numpy as np
import pytest

import oracle_lib as O
import reloc_scenes as S
from test_gpu_track import iv  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
F = np.float32
SCENES = S.scenes()
FILL = -7


def groups(scenes):
    out = {}
    for sc in scenes:
        out.setdefault(sc.group, []).append(sc)
    return list(out.values())


def make_tracker(iv, cam, max_pairs):
    return iv.BatchTracker(cam["nf"], cam["scale"], float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam["bf"]),
                           cam["bounds"], max_pairs=max_pairs, b=float(cam["b"]))


def pad(a, nf, fill):
    out = np.full(nf, fill, np.asarray(a).dtype)
    out[:len(a)] = a
    return out


def found_mask(sc, nf):
    m = np.zeros(nf, np.uint8)
    m[sorted(sc.found)] = 1
    return m


def run_scenes(iv, scs, quality=None, poses=True, tracker=None, stream=False):
    """the scenes as the pairs of one call per entry of their (shared) call list: per call (assign [n, nf], nmatches [n]) and, with
    quality = (point_q, key_q) [n, nf], the two arrays after the last call"""
    import torch
    from iv_slam_amd import _lib, dist as ivd
    cam, nf, n = scs[0].cam, scs[0].cam["nf"], len(scs)
    dev = torch.device("cuda:0")
    recs = [r for sc in scs for r in (sc.rec_kf, sc.rec_cur)]
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    tr = tracker or make_tracker(iv, cam, n)
    dp = torch.tensor([(2 * k, 2 * k + 1) for k in range(n)], dtype=torch.int32, device=dev)
    pts = np.zeros((2 * n, nf), _lib.LOCAL_POINT_DTYPE); pts["flags"] = 1
    for k, sc in enumerate(scs):
        pts[2 * k] = S.kf_points(sc, nf, _lib.LOCAL_POINT_DTYPE)
    dpts = torch.from_numpy(pts.view(np.uint8).reshape(-1)).to(dev)
    dposes = torch.from_numpy(np.stack([sc.T[:3, :4].reshape(12) for sc in scs]).astype(F)).to(dev) if poses else None
    assign = torch.from_numpy(np.stack([pad(sc.assign0, nf, FILL) for sc in scs])).to(dev)
    dfound = torch.from_numpy(np.stack([found_mask(sc, nf) for sc in scs])).to(dev)
    dpq = dkq = None
    if quality is not None:
        dpq = torch.from_numpy(np.ascontiguousarray(quality[0], F)).to(dev); dkq = torch.from_numpy(np.ascontiguousarray(quality[1], F)).to(dev)
    st = torch.cuda.Stream() if stream else None
    if st is not None:
        st.wait_stream(torch.cuda.current_stream())
    out = []
    for c in scs[0].calls:
        nm = torch.full((n,), FILL, dtype=torch.int32, device=dev)
        tr.search_reloc(block, dp, dpts, assign, nm, th=float(c["th"]), orb_dist=c["orb_dist"], poses=dposes, found=dfound if c["given"] else None,
                        check_orientation=scs[0].ori, point_quality=dpq, key_quality=dkq, stream_ptr=None if st is None else st.cuda_stream)
        if st is not None:
            torch.cuda.current_stream().wait_stream(st)
        out.append((assign.clone(), nm))
        if st is not None:
            st.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = [(a.cpu().numpy(), m.cpu().numpy()) for a, m in out]
    if quality is not None:
        return out, dpq.cpu().numpy(), dkq.cpu().numpy()
    return out


def check_scene(sc, got, k, how):
    """got: per call (assign [n, nf], nmatches [n]); pair k is scene sc"""
    import projection_oracle as PO
    nC = len(sc.rec_cur["kps"])
    ref = S.run_calls(O, PO, sc, S.oracle_call)
    w = S.run_calls(O, PO, sc, S.walk)
    for c in range(len(sc.calls)):
        a, nm = got[c][0][k], int(got[c][1][k])
        assert np.array_equal(a[:nC], ref[c][1]), "scene %s, call %d (%s): device differs from the oracle\n%s" % (
            sc.name, c, how, S.explain(a[:nC], ref[c][1], w[c][2], w[c][3]))
        assert nm == ref[c][0], "scene %s, call %d (%s): nmatches %d, oracle %d" % (sc.name, c, how, nm, ref[c][0])
        assert (a[nC:] == FILL).all(), "entries past the record's count were written"
    return ref


@pytest.mark.parametrize("scs", groups(SCENES), ids=lambda g: "%s%s" % (g[0].name, "_and_%d_more" % (len(g) - 1) if len(g) > 1 else ""))
def test_scenes_as_the_pairs_of_one_call(iv, scs):
    got = run_scenes(iv, scs)
    for k, sc in enumerate(scs):
        check_scene(sc, got, k, "pair %d of %d" % (k, len(scs)))


def test_scenes_one_call_each_without_poses(iv):
    """every scene alone; the scenes' poses are the identity, so NULL poses must give the same"""
    for sc in SCENES:
        if sc.cam["nf"] > S.NF:
            continue
        assert np.array_equal(sc.T, S.I4)
        check_scene(sc, run_scenes(iv, [sc], poses=False), 0, "alone, d_poses NULL")


@pytest.mark.parametrize("scs", groups(SCENES), ids=lambda g: g[0].name)
def test_scenes_with_quality_arrays(iv, scs):
    """UpdateQualityScores(CurrentFrame) (ORBmatcher.cc:1647-1649, :1108-1121) at the end of every call, over every keypoint that holds a point
    -- those held on entry included; scores on a 0.004 lattice, so differences fall on both sides of the 0.01 write-back threshold"""
    import projection_oracle as PO
    nf = scs[0].cam["nf"]
    rng = np.random.default_rng(31)
    pq = (rng.integers(0, 250, (len(scs), nf)) * F(0.004)).astype(F); kq = (rng.integers(0, 250, (len(scs), nf)) * F(0.004)).astype(F)
    got, gpq, gkq = run_scenes(iv, scs, quality=(pq, kq))
    for k, sc in enumerate(scs):
        ref = check_scene(sc, got, k, "with quality arrays")
        nC = len(sc.rec_cur["kps"])
        ekq, epq = kq[k, :nC].copy(), pq[k].copy()
        for c in range(len(sc.calls)):
            ekq, epq = PO.update_quality_scores([int(v) for v in ref[c][1]], ekq, epq)
        assert gkq[k, :nC].tobytes() == ekq.tobytes() and gpq[k].tobytes() == epq.tobytes(), sc.name
        assert np.array_equal(gkq[k, nC:], kq[k, nC:])
        assert (ekq != kq[k, :nC]).any() or not (ref[-1][1] >= 0).any()


def test_quality_write_back_rule(iv):
    """a point's score is written back only when it moves by more than 0.01 (ORBmatcher.cc:1116-1118); the keypoint's always"""
    sc = [s for s in SCENES if s.name == "skip_rules"][0]
    nf = sc.cam["nf"]
    pq = np.full((1, nf), 0.5, F); kq = np.full((1, nf), 0.5, F)
    kq[0, 0] = F(0.495)                                                          # keypoint 0 takes keyframe keypoint 0: 0.005 below its score
    got, gpq, gkq = run_scenes(iv, [sc], quality=(pq, kq))
    assert got[0][0][0, 0] == 0 and gpq[0, 0] == F(0.5) and gkq[0, 0] == F(0.495)
    kq[0, 0] = F(0.4)
    got, gpq, gkq = run_scenes(iv, [sc], quality=(pq, kq))
    assert gpq[0, 0] == F(0.4) and gkq[0, 0] == F(0.4) and (gpq[0, 1:] == F(0.5)).all()


def test_two_runs_are_bit_identical_on_any_stream(iv):
    scs = max(groups(SCENES), key=len)
    tr = make_tracker(iv, scs[0].cam, len(scs))
    a = run_scenes(iv, scs)
    b = run_scenes(iv, scs, tracker=tr)
    c = run_scenes(iv, scs, tracker=tr, stream=True)
    for x in (b, c):
        for (a0, n0), (a1, n1) in zip(a, x):
            assert a0.tobytes() == a1.tobytes() and n0.tobytes() == n1.tobytes()


def test_select_and_record_indices_outside_the_block(iv):
    """d_select 0 gives -2, a record index of -1 or n_records gives -1; neither pair's d_assign is touched"""
    import torch
    from iv_slam_amd import _lib, dist as ivd
    sc = [s for s in SCENES if s.name == "acceptance_and_ties"][0]
    nf, dev = sc.cam["nf"], torch.device("cuda:0")
    block = torch.from_numpy(ivd.pack_records([sc.rec_kf, sc.rec_cur], nf).reshape(-1)).to(dev)
    pts = np.zeros((2, nf), _lib.LOCAL_POINT_DTYPE); pts[0] = S.kf_points(sc, nf, _lib.LOCAL_POINT_DTYPE); pts[1]["flags"] = 1
    dpts = torch.from_numpy(pts.view(np.uint8).reshape(-1)).to(dev)
    pairs = [(0, 1), (0, 1), (-1, 1), (0, 2), (2, 1), (0, -1), (0, 1)]
    sel = [1, 0, 1, 1, 1, 1, 5]
    tr = make_tracker(iv, sc.cam, len(pairs))
    a0 = np.stack([pad(sc.assign0, nf, FILL)] * len(pairs))
    assign = torch.from_numpy(a0).to(dev); nm = torch.full((len(pairs),), FILL, dtype=torch.int32, device=dev)
    c = sc.calls[0]
    tr.search_reloc(block, torch.tensor(pairs, dtype=torch.int32, device=dev), dpts, assign, nm, th=float(c["th"]), orb_dist=c["orb_dist"],
                    select=torch.tensor(sel, dtype=torch.int32, device=dev), found=torch.from_numpy(np.stack([found_mask(sc, nf)] * len(pairs))).to(dev))
    torch.cuda.synchronize()
    a, nm = assign.cpu().numpy(), nm.cpu().numpy()
    assert nm.tolist()[1:6] == [-2, -1, -1, -1, -1] and nm[0] == nm[6] == 4
    assert np.array_equal(a[1:6], a0[1:6]) and np.array_equal(a[0], a[6]) and not np.array_equal(a[0], a0[0])


# ---- a seeded random sweep ----------------------------------------------------------------------------------------------------------
def random_case(rng, nf, quality_safe):
    """clustered current keypoints (windows of well over 64 candidates), keyframe points un-projected from them under a random pose with a
    perturbation, a descriptor some bits away, random levels, angles from a few values, random occupancy and found sets"""
    W, H = 640.0, 240.0
    nC = int(rng.integers(nf // 2, nf + 1)); nK = int(rng.integers(nf // 2, nf + 1))
    centres = rng.uniform([40, 40], [W - 40, H - 40], (3, 2))
    xy = centres[rng.integers(0, 3, nC)] + rng.normal(0, 5.0, (nC, 2))
    cur = np.zeros(nC, S.KP_DTYPE)
    cur["x"] = np.clip(xy[:, 0], 1, W - 1); cur["y"] = np.clip(xy[:, 1], 1, H - 1); cur["octave"] = rng.integers(0, 4, nC); cur["size"] = 31
    cur["angle"] = rng.choice([0.0, 45.0, 200.0], nC)
    cdesc = rng.integers(0, 256, (nC, 32)).astype(np.uint8)
    cdesc[:, 8:] = cdesc[0, 8:]                                                    # descriptors differ in 64 bits only: many candidates below ORBdist
    from test_gpu_track import pose
    T = pose(float(rng.uniform(-3, 3)), rng.uniform(-0.3, 0.3, 3), float(rng.uniform(-2, 2)))
    Rm, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    kf = np.zeros(nK, S.KP_DTYPE); kf["size"] = 31; kf["angle"] = rng.choice([0.0, 45.0, 90.0, 200.0, 300.0], nK, p=[0.5, 0.2, 0.1, 0.1, 0.1])
    points = []
    for i in range(nK):
        if rng.uniform() < 0.15:
            points.append(None)
            continue
        j = int(rng.integers(0, nC))
        z = float(rng.uniform(2, 20)) * (-1 if rng.uniform() < 0.05 else 1)
        u = cur["x"][j] + rng.normal(0, 3); v = cur["y"][j] + rng.normal(0, 3)
        pc = np.array([(u - 320.0) * z / 256.0, (v - 120.0) * z / 256.0, z])
        xw = (Rm.T @ (pc - t)).astype(F)
        dist = float(np.linalg.norm(pc))
        maxd = dist * 1.2 ** (int(cur["octave"][j]) - 0.5 + rng.uniform(-1.2, 1.2))
        mind = maxd / 3.6 if rng.uniform() < 0.9 else dist * rng.uniform(1.0, 1.4)
        points.append(dict(pos=xw, minDist=F(mind), maxDist=F(maxd), desc=S.at_distance(cdesc[j], int(rng.integers(0, 90)), shift=int(rng.integers(0, 64))),
                           bad=bool(rng.uniform() < 0.05)))
    assign0 = np.where(rng.uniform(size=nC) < 0.2, rng.integers(0, nK, nC), -1).astype(np.int32)
    found = set(int(i) for i in np.nonzero(rng.uniform(size=nK) < 0.2)[0])
    if quality_safe:
        found |= set(int(a) for a in assign0 if a >= 0)                          # as in the reference: sAlreadyFound contains what the frame holds
        _, first = np.unique(np.where(assign0 >= 0, assign0, -np.arange(1, nC + 1)), return_index=True)
        keep = np.zeros(nC, bool); keep[first] = True
        assign0 = np.where(keep, assign0, -1).astype(np.int32)                    # and a point sits on one keypoint
    sc = types.SimpleNamespace(name="random", ori=True, T=T, cam=S.cam(nf=nf), points=points, found=found, assign0=assign0,
                               rec_kf=dict(kps=kf, desc=rng.integers(0, 256, (nK, 32)).astype(np.uint8), uright=np.full(nK, -1, F), depth=np.full(nK, -1, F)),
                               rec_cur=dict(kps=cur, desc=cdesc, uright=np.full(nC, -1, F), depth=np.full(nC, -1, F)))
    return sc


@pytest.mark.parametrize("seed,nf,th,orb_dist,ori", [(1, 512, 10.0, 100, True), (2, 300, 3.0, 64, True), (3, 64, 10.0, 100, True), (4, 512, 15.0, 40, False),
                                                     (5, 200, 10.0, 255, True), (6, 512, 10.0, 0, True)])
def test_random_sweep_against_the_oracle(iv, seed, nf, th, orb_dist, ori):
    """six calls of four pairs: 24 cases.  Pairs 0 and 1 carry quality arrays' preconditions (found covers the entries), 2 and 3 arbitrary sets."""
    import projection_oracle as PO
    rng = np.random.default_rng(seed)
    scs = [random_case(rng, nf, k < 2) for k in range(4)]
    for sc in scs:
        sc.ori = ori
        sc.calls = [dict(th=F(th), orb_dist=orb_dist, given=True)]
    got = run_scenes(iv, scs)
    overflow = rotated = 0
    for k, sc in enumerate(scs):
        nC = len(sc.rec_cur["kps"])
        nm, ref = S.oracle_search(O, PO, sc, sc.assign0, sc.T, sc.found, th, orb_dist)
        a = got[0][0][k]
        bad = np.nonzero(a[:nC] != ref)[0]
        assert bad.size == 0, "seed %d pair %d: %d keypoints differ, first %d: device %d, oracle %d" % (seed, k, bad.size, bad[0], a[bad[0]], ref[bad[0]])
        assert int(got[0][1][k]) == nm and (a[nC:] == FILL).all()
        w = S.walk(O, PO, sc, sc.assign0, 0)
        assert w[0] == nm and np.array_equal(w[1], ref)
        overflow += sum(1 for i in w[3] if i.get("n_window", 0) > 64)
        rotated += w[2].count(S.ROTATED_OUT)
    print("seed %d: %d overflowing windows, %d matches taken back by the rotation filter" % (seed, overflow, rotated))
    if seed == 1:
        assert overflow > 0 and rotated > 0
    if nf == 512 and orb_dist == 100:
        pq = (rng.integers(0, 250, (4, nf)) * F(0.004)).astype(F); kq = (rng.integers(0, 250, (4, nf)) * F(0.004)).astype(F)
        got2, gpq, gkq = run_scenes(iv, scs[:2], quality=(pq[:2], kq[:2]))
        for k, sc in enumerate(scs[:2]):
            nC = len(sc.rec_cur["kps"])
            assert np.array_equal(got2[0][0][k], got[0][0][k])
            ekq, epq = PO.update_quality_scores([int(v) for v in got[0][0][k][:nC]], kq[k, :nC], pq[k])
            assert gkq[k, :nC].tobytes() == ekq.tobytes() and gpq[k].tobytes() == epq.tobytes()


# ---- filter_assign, argument checks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("use_found", [False, True])
def test_filter_assign_against_numpy(iv, use_mask, keep, use_found):
    import torch
    nf, n = 300, 3
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    a0 = np.where(rng.uniform(size=(n, nf)) < 0.5, rng.integers(0, nf, (n, nf)), -1).astype(np.int32)
    mask = (rng.integers(0, 3, (n, nf)) % 2 * rng.integers(1, 255, (n, nf))).astype(np.uint8)
    exp = a0.copy()
    if use_mask:
        exp[(mask != 0) != keep] = -1
    efound = np.zeros((n, nf), np.uint8)
    for f in range(n):
        efound[f, exp[f][exp[f] >= 0]] = 1
    tr = make_tracker(iv, S.cam(nf=nf), n)
    a = torch.from_numpy(a0).to(dev); found = torch.full((n, nf), 9, dtype=torch.uint8, device=dev)
    tr.filter_assign(a, mask=torch.from_numpy(mask).to(dev) if use_mask else None, keep_when_set=keep, found=found if use_found else None)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), exp)
    assert np.array_equal(found.cpu().numpy(), efound if use_found else np.full((n, nf), 9, np.uint8))


def test_arguments_are_checked(iv):
    import torch
    from iv_slam_amd import _lib
    sc = SCENES[0]
    ok = dict(th=10.0, orb_dist=100)
    for bad in (dict(orb_dist=-1), dict(orb_dist=256), dict(th=0.0), dict(th=-1.0), dict(th=float("nan")), dict(pairs=2), dict(quality=1), dict(null="assign"),
                dict(null="kf_points"), dict(null="nmatches")):
        dev = torch.device("cuda:0")
        nf = sc.cam["nf"]
        n = bad.get("pairs", 1)
        tr = make_tracker(iv, sc.cam, 1)
        from iv_slam_amd import dist as ivd
        block = torch.from_numpy(ivd.pack_records([sc.rec_kf, sc.rec_cur], nf).reshape(-1)).to(dev)
        dpts = torch.zeros(2 * nf * 80, dtype=torch.uint8, device=dev)
        assign = torch.full((n, nf), -1, dtype=torch.int32, device=dev); nm = torch.zeros(n, dtype=torch.int32, device=dev)
        dp = torch.tensor([(0, 1)] * n, dtype=torch.int32, device=dev)
        kw = dict(ok, **{k: v for k, v in bad.items() if k in ok})
        if "null" in bad:
            args = dict(assign=assign.data_ptr(), kf_points=dpts.data_ptr(), nmatches=nm.data_ptr())
            args[bad["null"]] = None
            rc = tr._lib.ivf_tracker_search_reloc(tr._h, block.data_ptr(), tr.record_bytes, 2, dp.data_ptr(), n, None, None, args["kf_points"], None, 10.0, 100, 1,
                                                  None, None, args["assign"], args["nmatches"], None)
            assert rc == _lib.IVF_E_INVALID, bad
            continue
        with pytest.raises(iv.IvfError) as e:
            tr.search_reloc(block, dp, dpts, assign, nm, point_quality=torch.zeros((n, nf), device=dev) if "quality" in bad else None, **kw)
        assert e.value.code == _lib.IVF_E_INVALID, bad
        if "pairs" in bad:
            with pytest.raises(iv.IvfError):
                tr.filter_assign(assign)
    torch.cuda.synchronize()
    assert (assign.cpu().numpy() == -1).all()


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def test_relocalization_chain_without_leaving_the_device(iv):
    """Tracking.cc:2351-2404 on tests/reloc_scenes.py:Chain, enqueued without a host synchronisation: filter_assign (sFound) ->
    points_from_keyframe -> optimize_pose -> filter_assign (outliers) -> search_reloc(10, 100) -> points_from_keyframe -> optimize_pose ->
    filter_assign -> search_reloc(3, 64, found = NULL) -> points_from_keyframe -> optimize_pose -> filter_assign; the masks that decide who
    searches are torch comparisons of the device's own counts.  Pair 1 is the same frame already holding 63 true matches: it is left out
    of both searches.  Every search equals the oracle on the fetched inputs of that step; every optimised pose is within 4 float quanta of
    tests/pose_opt_ref.py fed the same inputs; the chain ends with at least 50 inliers."""
    import torch
    import projection_oracle as PO
    import pose_opt_ref as PR
    from iv_slam_amd import _lib, dist as ivd
    ch = S.Chain()
    ch2 = S.Chain(n_entry=63)
    nf, nC, dev = S.CHAIN_NF, ch.nC, torch.device("cuda:0")
    tr = make_tracker(iv, ch.cam, 2)
    block = torch.from_numpy(ivd.pack_records([ch.rec_kf, ch.rec_cur], nf).reshape(-1)).to(dev)
    dp = torch.tensor([(0, 1), (0, 1)], dtype=torch.int32, device=dev)
    cur = dp[:, 1].contiguous()
    pts = np.zeros((2, nf), _lib.LOCAL_POINT_DTYPE); pts[0] = S.kf_points(ch, nf, _lib.LOCAL_POINT_DTYPE); pts[1]["flags"] = 1
    dpts = torch.from_numpy(pts.view(np.uint8).reshape(-1)).to(dev)
    kxw = np.zeros((2, nf, 3), F); kxw[0] = ch.kf_xw
    dkxw = torch.from_numpy(kxw).to(dev)
    assign = torch.from_numpy(np.stack([pad(ch.assign0, nf, -1), pad(ch2.assign0, nf, -1)])).to(dev)
    poses = torch.from_numpy(np.stack([ch.pose_in, ch.pose_in]).astype(F)).to(dev)
    found = torch.full((2, nf), 9, dtype=torch.uint8, device=dev)
    xw = torch.zeros((2, nf, 3), dtype=torch.float32, device=dev); has = torch.zeros((2, nf), dtype=torch.uint8, device=dev)
    outl = torch.zeros((2, nf), dtype=torch.uint8, device=dev)
    snap = {}

    def optimise(tag):
        tr.points_from_keyframe(dp, dkxw, assign, xw, has)
        ninl = torch.full((2,), FILL, dtype=torch.int32, device=dev)
        snap[tag + "_in"] = (xw.clone(), has.clone(), poses.clone())
        tr.optimize_pose(block, cur, xw, has, poses, outl, ninl)
        snap[tag + "_out"] = (poses.clone(), outl.clone(), ninl)
        tr.filter_assign(assign, mask=outl, keep_when_set=False)                  # :2368-2370, :2398-2400
        return ninl

    def search(tag, sel, th, orb_dist, fnd):
        nm = torch.full((2,), FILL, dtype=torch.int32, device=dev)
        snap[tag + "_in"] = (assign.clone(), poses.clone(), None if fnd is None else fnd.clone(), sel.clone())
        tr.search_reloc(block, dp, dpts, assign, nm, th=th, orb_dist=orb_dist, select=sel, poses=poses, found=fnd)
        snap[tag + "_out"] = (assign.clone(), nm)
        return nm

    tr.filter_assign(assign, found=found)                                         # :2351-2361 (the entries are PnP's inliers already)
    good1 = optimise("opt1")
    sel1 = ((good1 >= 10) & (good1 < 50)).to(torch.int32)                         # :2366, :2374
    add1 = search("search1", sel1, 10.0, 100, found)
    good2 = optimise("opt2")                                                      # :2379
    sel2 = (sel1.bool() & (add1 + good1 >= 50) & (good2 > 30) & (good2 < 50)).to(torch.int32)     # :2378, :2385
    add2 = search("search2", sel2, 3.0, 64, None)
    good3 = optimise("opt3")                                                      # :2395
    torch.cuda.synchronize()

    cpu = {k: tuple(None if t is None else t.cpu().numpy() for t in v) for k, v in snap.items()}
    ref = S.chain_reference(O, PO, PR, ch)
    q = float(np.sqrt(3.0) * 2.0 ** -23)
    for tag in ("opt1", "opt2", "opt3"):
        (ixw, ihas, ipose), (opose, ooutl, oninl) = cpu[tag + "_in"], cpu[tag + "_out"]
        c = ch.cam
        r = PR.pose_optimization(ch.rec_cur["kps"], nC, ch.rec_cur["uright"], ch.INV_SIGMA2, c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], ixw[0][:nC], ihas[0][:nC],
                                 None, 4, ipose[0])
        rot, trn = PR.pose_difference(opose[0], r["pose"])
        print("%s: %d edges, %d inliers (restatement %d); pose vs restatement %.3g rad %.3g" % (tag, ihas[0].sum(), oninl[0], r["ninliers"], rot, trn))
        assert rot <= 4 * q and trn <= 4 * q
        assert np.array_equal(ooutl[0, :nC], r["outlier"][:nC]) and oninl[0] == r["ninliers"]
    for tag, th, od in (("search1", 10.0, 100), ("search2", 3.0, 64)):
        (ia, ipose, ifound, isel), (oa, onm) = cpu[tag + "_in"], cpu[tag + "_out"]
        assert isel.tolist() == [1, 0]
        fnd = set(np.nonzero(ifound[0])[0].tolist()) if ifound is not None else set(int(v) for v in ia[0] if v >= 0)
        nm, ea = S.oracle_search(O, PO, ch, ia[0][:nC], ipose[0].reshape(3, 4), fnd, th, od)
        assert np.array_equal(oa[0][:nC], ea) and onm[0] == nm and (oa[0][nC:] == -1).all(), tag
        assert onm[1] == -2 and np.array_equal(oa[1], ia[1])                      # the pair that needs no search is left alone
        print("%s: %d additional matches" % (tag, nm))
    g1, g2, g3 = (int(cpu[t + "_out"][2][0]) for t in ("opt1", "opt2", "opt3"))
    a1, a2 = int(cpu["search1_out"][1][0]), int(cpu["search2_out"][1][0])
    assert cpu["opt1_out"][2][1] >= 50
    assert 10 <= g1 < 50 and a1 + g1 >= 50 and 30 < g2 < 50 and a2 + g2 >= 50 and g3 >= 50
    assert (g1, a1, g2, a2, g3) == (ref["nGood1"], ref["nadd1"], ref["nGood2"], ref["nadd2"], ref["nGood3"])
    # sFound after the first filter_assign: the 33 entries
    f0 = cpu["search1_in"][2][0]
    assert set(np.nonzero(f0)[0].tolist()) == set(int(v) for v in ch.assign0 if v >= 0) and set(np.unique(f0).tolist()) <= {0, 1}
    final = assign.cpu().numpy()[0]
    assert (final[:nC] >= 0).sum() == g3 and np.array_equal(final[:nC], ref["assign3"])
