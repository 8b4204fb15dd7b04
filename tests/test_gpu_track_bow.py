"""ivf_tracker_search_by_bow / ivf_tracker_points_from_keyframe (iv_slam_amd/csrc/ivf_track_bow.hip, ivf_track_points.hip) -- the matcher part of
Tracking::TrackReferenceKeyFrame (ORB/src/Tracking.cc:1159-1176) for many (keyframe, current frame) pairs on the device -- against the C
oracle's SearchByBoW on feature vectors built from its own transform, and against the per-call ivf_bow_transform + ivf_bow_vectors +
ivf_search_by_bow path on the same data.  Every comparison is bit for bit (integers, and the min of floats in the quality update)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O
import pose_opt_ref as PR
import pose_opt_scenes as PS
import track_bow_ref as R
import track_bow_scenes as S
from test_gpu_track import extracted_sequence, scale_table, iv  # noqa: F401  (iv: the module fixture)

pytestmark = pytest.mark.gpu
F = np.float32
NF = S.NF


def vocabulary(iv, tree):
    return iv.ORBVocabulary(tree["child_start"], tree["child"], tree["desc"], tree["word"], tree["weight"], tree["depth"])


def make_tracker(iv, nf, max_pairs, cam=None, bounds=S.BOUNDS):
    c = cam or S.CAM
    return iv.BatchTracker(nf, scale_table(), float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), float(c["bf"]), bounds, max_pairs=max_pairs)


def run_bow(iv, tr, V, levelsup, recs, pairs, nf, select=None, flags=None, check_orientation=True, quality=None, nn_ratio=0.7, block=None):
    """-> (assign [n_pairs, nf], nmatches [n_pairs][, point quality, key quality]) from the device"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    if block is None:
        block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    n = len(pairs)
    dp = torch.tensor(pairs, dtype=torch.int32, device=dev).reshape(-1, 2)
    assign = torch.full((n, nf), -7, dtype=torch.int32, device=dev); nm = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dsel = None if select is None else torch.tensor(select, dtype=torch.int32, device=dev)
    dfl = None if flags is None else torch.from_numpy(np.ascontiguousarray(flags, np.uint8)).to(dev)
    dpq = dkq = None
    if quality is not None:
        dpq = torch.from_numpy(np.ascontiguousarray(quality[0], F)).to(dev); dkq = torch.from_numpy(np.ascontiguousarray(quality[1], F)).to(dev)
    tr.search_by_bow(V, block, dp, assign, nm, levelsup=levelsup, select=dsel, point_flags=dfl, nn_ratio=nn_ratio, check_orientation=check_orientation,
                     point_quality=dpq, key_quality=dkq)
    torch.cuda.synchronize()
    if quality is not None:
        return assign.cpu().numpy(), nm.cpu().numpy(), dpq.cpu().numpy(), dkq.cpu().numpy()
    return assign.cpu().numpy(), nm.cpu().numpy()


_BLOCKS = {}


def scene_block(depth):
    """every scene as two records (keyframe 2k, frame 2k + 1) and one pair each, plus the main scene's keyframe against the frame of
    another scene: that record is the keyframe of two pairs.  Built once per tree and shared."""
    if depth not in _BLOCKS:
        scs = S.scenes(depth)
        recs = []; pairs = []; items = []
        for k, sc in enumerate(scs):
            recs.extend(S.records_of(sc)); pairs.append((2 * k, 2 * k + 1)); items.append(sc)
        cross = dict(name="main_x_wide", tree=scs[0]["tree"], levelsup=scs[0]["levelsup"], kf=scs[0]["kf"], f=scs[2]["f"])
        pairs.append((0, 5)); items.append(cross)
        _BLOCKS[depth] = (scs[0]["tree"], recs, pairs, items)
    return _BLOCKS[depth]


def point_flags(recs, items, pairs, mode):
    """mode 0: no flags (a keyframe keypoint holds a point where it has a stereo depth); 1: flags that differ from the depth pattern"""
    if not mode:
        return None, [sc["kf"]["has"] for sc in items]
    fl = np.zeros((len(recs), NF), np.uint8)
    for r, rec in enumerate(recs):
        h = (rec["depth"] > 0).astype(np.uint8)
        h[::7] ^= 1
        fl[r, :len(h)] = h | 2 * (np.arange(len(h)) % 2).astype(np.uint8)       # bit 1 is not this call's
    return fl, [fl[a, :len(sc["kf"]["kps"])] & 1 for sc, (a, b) in zip(items, pairs)]


def check_against_oracle(items, has, assign, nm, levelsup, check_orientation, what):
    total = 0
    for k, sc in enumerate(items):
        om, onm = S.oracle(O, sc, levelsup, 0.7, check_orientation, has=has[k])
        nF = len(sc["f"]["kps"])
        assert nm[k] == onm, "%s %s: nmatches %d vs oracle %d" % (what, sc["name"], nm[k], onm)
        assert np.array_equal(assign[k, :nF], om), "%s %s: assignment differs at %r" % (what, sc["name"], np.nonzero(assign[k, :nF] != om)[0][:8])
        assert (assign[k, nF:] == -1).all()
        total += onm
    return total


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("check_orientation", [True, False])
@pytest.mark.parametrize("with_flags", [0, 1])
def test_scenes_through_the_abi(iv, depth, check_orientation, with_flags):
    """every hand-made scene as one pair of one call: nodes at level 2, and every feature in node 0 (levelsup = L and L + 2); equal to
    the oracle and to the per-call path; a second run is byte-identical"""
    tree, recs, pairs, items = scene_block(depth)
    V = vocabulary(iv, tree)
    tr = make_tracker(iv, NF, len(pairs))
    fl, has = point_flags(recs, items, pairs, with_flags)
    for ls in (depth - 2, depth, depth + 2):
        assign, nm = run_bow(iv, tr, V, ls, recs, pairs, NF, flags=fl, check_orientation=check_orientation)
        tot = check_against_oracle(items, has, assign, nm, ls, check_orientation, "levelsup %d" % ls)
        assert tot > 60
        again = run_bow(iv, tr, V, ls, recs, pairs, NF, flags=fl, check_orientation=check_orientation)
        assert again[0].tobytes() == assign.tobytes() and again[1].tobytes() == nm.tobytes()
    # the per-call path of the same library on the same data
    m = iv.ORBmatcher(0.7, check_orientation)
    ls = depth - 2
    assign, nm = run_bow(iv, tr, V, ls, recs, pairs, NF, flags=fl, check_orientation=check_orientation)
    for k, sc in enumerate(items):
        nK, nF = len(sc["kf"]["kps"]), len(sc["f"]["kps"])
        if nK == 0 or nF == 0:
            assert nm[k] == 0 and (assign[k] == -1).all()
            continue
        _, kfv = V.transform(sc["kf"]["desc"], ls); _, ffv = V.transform(sc["f"]["desc"], ls)
        gm, gn = m.SearchByBoW(sc["kf"]["kps"], sc["kf"]["desc"], has[k], kfv, sc["f"]["kps"], sc["f"]["desc"], ffv)
        assert gn == nm[k] and np.array_equal(gm, assign[k, :nF]), sc["name"]


def test_select_mask_and_record_index_outside_the_block(iv):
    tree, recs, pairs, items = scene_block(3)
    V = vocabulary(iv, tree)
    tr = make_tracker(iv, NF, len(pairs))
    has = [sc["kf"]["has"] for sc in items]
    full_a, full_n = run_bow(iv, tr, V, 1, recs, pairs, NF)
    sel = [k % 2 for k in range(len(pairs))]
    a, n = run_bow(iv, tr, V, 1, recs, pairs, NF, select=sel)
    for k in range(len(pairs)):
        if sel[k]:
            assert n[k] == full_n[k] and a[k].tobytes() == full_a[k].tobytes()
        else:
            assert n[k] == -2 and (a[k] == -1).all()
    bad = list(pairs); bad[1] = (len(recs) + 3, 3); bad[4] = (8, -1)
    a, n = run_bow(iv, tr, V, 1, recs, bad, NF)
    for k in range(len(pairs)):
        if k in (1, 4):
            assert n[k] == -1 and (a[k] == -1).all()
        else:
            assert n[k] == full_n[k] and a[k].tobytes() == full_a[k].tobytes()
    check_against_oracle(items, has, full_a, full_n, 1, True, "unmasked")
    a, n = run_bow(iv, tr, V, 1, recs, bad, NF, select=[0] * len(pairs))          # left out wins over a bad index: nothing is read
    assert (n == -2).all() and (a == -1).all()


def test_batch_sizes_and_consecutive_calls_on_one_handle(iv):
    """n_pairs = 1, 3 and max_pairs give the same per-pair results; two calls on one handle with different pair tables (the second
    reverses the first: every scratch slot holds another record's feature vector) do not see each other's feature vectors"""
    tree, recs, pairs, items = scene_block(3)
    V = vocabulary(iv, tree)
    tr = make_tracker(iv, NF, len(pairs))
    full_a, full_n = run_bow(iv, tr, V, 1, recs, pairs, NF)
    for k in range(len(pairs)):
        assert full_n[k] == S.oracle(O, items[k], 1)[1]
    a1, n1 = run_bow(iv, tr, V, 1, recs, pairs[:1], NF)
    assert n1[0] == full_n[0] and a1[0].tobytes() == full_a[0].tobytes()
    a3, n3 = run_bow(iv, tr, V, 1, recs, pairs[3:6], NF)
    assert n3.tobytes() == full_n[3:6].tobytes() and a3.tobytes() == full_a[3:6].tobytes()
    rev = pairs[::-1]
    ar, nr = run_bow(iv, tr, V, 1, recs, rev, NF)
    assert nr.tobytes() == full_n[::-1].tobytes() and ar.tobytes() == np.ascontiguousarray(full_a[::-1]).tobytes()
    a2, n2 = run_bow(iv, tr, V, 1, recs, pairs, NF)
    assert n2.tobytes() == full_n.tobytes() and a2.tobytes() == full_a.tobytes()
    with pytest.raises(iv.IvfError):
        run_bow(iv, tr, V, 1, recs, pairs + pairs[:1], NF)                     # n_pairs > max_pairs
    with pytest.raises(iv.IvfError):
        run_bow(iv, tr, V, -1, recs, pairs, NF)                                # levelsup < 0


def test_extracted_frames_at_1000_features(iv):
    """8 synthetic stereo frames from the front end, 1000 features each; a ragged tree whose node descriptors are descriptors of those
    frames, with stopped words; 7 consecutive pairs and a frame against itself; nodes of ~25 and of > 64 features (levelsup 1 and 2)"""
    import torch
    cam, recs, block, fe = extracted_sequence(iv, 1242, 375, 1000, 8, seed=93)
    rng = np.random.default_rng(8)
    tree = O.make_vocabulary(6, 3, seed=21, early_leaf_frac=0.1, stop_frac=0.05)
    pool = np.concatenate([r["desc"] for r in recs])
    tree["desc"][1:] = pool[rng.permutation(len(pool))[:len(tree["desc"]) - 1]]
    V = vocabulary(iv, tree)
    pairs = [(k - 1, k) for k in range(1, 8)] + [(3, 3)]
    tr = iv.BatchTracker(1000, cam["scale"], float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam["bf"]), cam["bounds"],
                         max_pairs=len(pairs), b=float(cam["b"]))
    for ls in (1, 2):
        assign, nm = run_bow(iv, tr, V, ls, recs, pairs, 1000, block=block)
        widest = 0
        for k, (a, b) in enumerate(pairs):
            sc = dict(name="pair %d" % k, tree=tree, levelsup=ls, kf=dict(kps=recs[a]["kps"], desc=recs[a]["desc"], has=(recs[a]["depth"] > 0).astype(np.uint8)),
                      f=dict(kps=recs[b]["kps"], desc=recs[b]["desc"]))
            kfv, ffv = S.node_ids(O, sc, ls)
            widest = max(widest, max(len(v) for v in ffv.values()))
            om, onm = O.search_by_bow(sc["kf"]["kps"], sc["kf"]["desc"], sc["kf"]["has"], kfv, sc["f"]["kps"], sc["f"]["desc"], ffv, 0.7, True)
            nF = len(sc["f"]["kps"])
            assert nm[k] == onm and np.array_equal(assign[k, :nF], om) and (assign[k, nF:] == -1).all(), (ls, k, nm[k], onm)
            assert onm >= 15
        print("levelsup %d: matches %r, widest node %d features" % (ls, nm.tolist(), widest))
        assert widest > 64 or ls == 1


def test_quality_scores_on_the_device(iv):
    tree, recs, pairs, items = scene_block(3)
    V = vocabulary(iv, tree)
    tr = make_tracker(iv, NF, len(pairs))
    rng = np.random.default_rng(12)
    pq = rng.uniform(0, 1, (len(pairs), NF)).astype(F); kq = rng.uniform(0, 1, (len(pairs), NF)).astype(F)
    kq[:, ::3] = pq[:, ::3] - F(0.005)                                          # changes below the 0.01 threshold, where they meet
    assign, nm, gpq, gkq = run_bow(iv, tr, V, 1, recs, pairs, NF, quality=(pq, kq))
    changed = 0
    for k, sc in enumerate(items):
        om, onm = S.oracle(O, sc, 1)
        full = np.full(NF, -1, np.int32); full[:len(om)] = om
        ek, em = kq[k].copy(), pq[k].copy()
        O.lib.orc_update_quality_scores(O.ptr(full), NF, O.ptr(ek), O.ptr(em))
        assert np.array_equal(assign[k], full) and gkq[k].tobytes() == ek.tobytes() and gpq[k].tobytes() == em.tobytes(), sc["name"]
        changed += int((em != pq[k]).sum())
    assert changed > 20


def test_chain_search_by_bow_points_optimize_pose(iv):
    """search_by_bow -> points_from_keyframe -> optimize_pose without leaving the device, on a current frame that observes known world
    points (tests/pose_opt_scenes.py) and a keyframe whose keypoints hold those points in shuffled order: d_xw / d_has_point equal a numpy
    gather of the oracle's assignment, the pose / flags / inlier count agree with tests/pose_opt_ref.py fed with that gather as
    tests/test_gpu_pose_opt.py's chain does (pose within 4 float quanta of the output, flags and count equal)"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    tree = S.TREES[3]
    V = vocabulary(iv, tree)
    fr = PS.make_frame(77, 200, 200, "mixed", noise=0.5, n_outliers=6)
    b = S.Builder(tree, 9)
    n = fr["n"]
    perm = b.rng.permutation(n)
    pay = [b.payload() for _ in range(n)]
    node = [b.nodes[i % len(b.nodes)] for i in range(n)]
    fdesc = np.stack([b.desc(node[i], pay[i]) for i in range(n)])
    kdesc = np.zeros((n, 32), np.uint8); kxw = np.zeros((3, NF, 3), F)
    for i in range(n):
        kdesc[perm[i]] = b.desc(node[i], b.flipped(pay[i], b.pick(2)))
        kxw[1, perm[i]] = fr["xw"][i]                                       # the keyframe is record 1
    kf = dict(kps=fr["kps"][perm.argsort()], desc=kdesc, has=(np.arange(n) % 10 != 3).astype(np.uint8))
    sc = dict(name="chain", tree=tree, levelsup=1, kf=kf, f=dict(kps=fr["kps"], desc=fdesc))
    recK, _ = S.records_of(sc)
    recF = dict(kps=fr["kps"], desc=fdesc, uright=fr["uright"], depth=fr["depth"])
    recs = [recF, recK, recF]
    pairs = [(1, 0), (7, 2), (1, 2)]                                        # the middle pair's keyframe is outside the block
    tr = iv.BatchTracker(NF, PS.SCALE, float(PS.CAM["fx"]), float(PS.CAM["fy"]), float(PS.CAM["cx"]), float(PS.CAM["cy"]), float(PS.CAM["bf"]), PS.BOUNDS, max_pairs=3)
    block = torch.from_numpy(ivd.pack_records(recs, NF).reshape(-1)).to(dev)
    dp = torch.tensor(pairs, dtype=torch.int32, device=dev)
    assign = torch.full((3, NF), -7, dtype=torch.int32, device=dev); nm = torch.full((3,), -7, dtype=torch.int32, device=dev)
    xw = torch.full((3, NF, 3), 7.0, dtype=torch.float32, device=dev); has = torch.full((3, NF), 7, dtype=torch.uint8, device=dev)
    cur = dp[:, 1].contiguous()
    poses = torch.from_numpy(np.stack([fr["pose_in"]] * 3).astype(F)).to(dev)
    outl = torch.full((3, NF), 9, dtype=torch.uint8, device=dev); ninl = torch.full((3,), -7, dtype=torch.int32, device=dev)
    tr.search_by_bow(V, block, dp, assign, nm, levelsup=1)
    tr.points_from_keyframe(dp, torch.from_numpy(kxw).to(dev), assign, xw, has)
    tr.optimize_pose(block, cur, xw, has, poses, outl, ninl)
    torch.cuda.synchronize()
    assign = assign.cpu().numpy(); nm = nm.cpu().numpy(); xw = xw.cpu().numpy(); has = has.cpu().numpy()
    poses = poses.cpu().numpy(); outl = outl.cpu().numpy(); ninl = ninl.cpu().numpy()
    om, onm = S.oracle(O, sc, 1)
    assert onm > 150 and nm.tolist() == [onm, -1, onm]
    exw = np.zeros((NF, 3), F); ehas = np.zeros(NF, np.uint8)
    for i in range(n):
        if om[i] >= 0:
            exw[i] = kxw[1, om[i]]; ehas[i] = 1
    ref = PR.pose_optimization(fr["kps"], n, fr["uright"], PS.INV_SIGMA2, PS.CAM["fx"], PS.CAM["fy"], PS.CAM["cx"], PS.CAM["cy"], PS.CAM["bf"], exw[:n], ehas[:n],
                               None, 4, fr["pose_in"])
    q = float(np.sqrt(3.0) * 2.0 ** -23)                                     # the float quantum of the output pose (tests/test_pose_opt_cpu.py)
    for p in (0, 2):
        assert np.array_equal(assign[p, :n], om) and (assign[p, n:] == -1).all()
        assert has[p].tobytes() == ehas.tobytes() and xw[p].tobytes() == exw.tobytes(), "points_from_keyframe is a gather"
        rot, trn = PR.pose_difference(poses[p], ref["pose"])
        print("chain pair %d: %d matches, %d inliers (restatement %d), pose vs restatement %.3g rad %.3g" % (p, nm[p], ninl[p], ref["ninliers"], rot, trn))
        assert rot <= 4 * q and trn <= 4 * q
        assert np.array_equal(outl[p, :n], ref["outlier"][:n]) and ninl[p] == ref["ninliers"] and ninl[p] > 100
    assert (assign[1] == -1).all() and not has[1].any() and not xw[1].any() and ninl[1] == 0 and poses[1].tobytes() == fr["pose_in"].astype(F).tobytes()
