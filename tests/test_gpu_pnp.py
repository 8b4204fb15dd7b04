"""ivf_tracker_solve_pnp (iv_slam_amd/csrc/ivf_pnp.hip) -- PnPsolver (ORB/src/PnPsolver.cc) as Tracking::Relocalization runs it, batched on
the device -- against tests/pnp_ref.py, the f64 restatement, on the scenes of tests/pnp_scenes.py.

The POSE of a 4-point hypothesis is not comparable between implementations (its MtM has a four-dimensional null space whose basis
rounding chooses, see tests/pnp_ref.py); what a hypothesis computes before and after that basis is, and tests/test_gpu_pnp_hyp.py compares
it through the taps of ivf_test_pnp_hypotheses (sample, control points, the basis as a basis, the three candidates, the choice, the
inlier count), taking only the basis as given.  Here the
device's own hypotheses (hyp_poses, hyp_ninliers) are taken as given and everything after them is replayed: CheckInliers of every
hypothesis pose in numpy, the bookkeeping of PnPsolver.cc:213-259 over those masks with the restatement's Refine, and the result compared.
Tolerance of the Refine pose: 4 x the floor committed in tests/golden/pnp_noise.json (the restatement's spread over its two SVD back ends
and 8 summation orders, not below the float quantum of the output; tests/test_pnp_cpu.py), the margin tests/test_gpu_pose_opt.py uses for
the same reason: a different but fixed summation order.

hyp_poses leaves the device as float, the device counted inliers under the double pose.  A point whose error2 lies closer to mvMaxError
than that narrowing can move it (band(), a bound worked out from the float format) may be counted either way: hyp_ninliers must lie
between the count without and with those points and equal the count where there are none, and where such a point belongs to a hypothesis
that raises mnBestInliers the replay follows every inlier set consistent with the device's count.

The sampler (draws -> indices) is not exposed by the call: the restatement's is checked on the CPU (tests/test_pnp_cpu.py, against a
transcription of :192-205), the device's on a scene whose NaN-tagged world points name the sample of every iteration (sampler_scene),
and directly, index by index, in tests/test_gpu_pnp_hyp.py."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ref as R
import pnp_scenes as S
import pose_opt_ref as PR
import ransac_ref as RR
from test_gpu_track import iv  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NOISE = json.load(open(os.path.join(ROOT, "tests", "golden", "pnp_noise.json")))
SCENARIOS = S.scenarios()
POSE_FILL, FLAG_FILL, INT_FILL = 7.0, 9, -7


def make_tracker(iv, nf, max_pairs):
    c = S.CAM
    return iv.BatchTracker(nf, S.SCALE, float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), float(c["bf"]), S.BOUNDS, max_pairs=max_pairs)


def run_pnp(iv, sc, order=None, stream=False, tracker=None, hyp=True):
    """-> dict of device results as numpy, indexed by frame (not by slot): slot j of the call holds frame order[j]"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    frames, nf, p = sc["frames"], sc["nf"], sc["params"]
    n = len(frames); mi = p["max_iterations"]
    order = list(range(n)) if order is None else list(order)
    block = torch.from_numpy(ivd.pack_records([dict(kps=f["kps"], desc=f["desc"], uright=f["uright"], depth=f["depth"]) for f in frames], nf).reshape(-1)).to(dev)
    tr = tracker or make_tracker(iv, nf, sc["max_pairs"])
    xw = np.zeros((n, nf, 3), F); has = np.zeros((n, nf), np.uint8)
    draws = sc["draws"] if "draws" in sc else S.R_draws(sc["seed"], n, mi)
    for j, k in enumerate(order):
        f = frames[k]
        xw[j, :f["n"]] = f["xw"]; has[j, :f["n"]] = f["has"]
        if f["kind"] == "tail":
            has[j, f["n"]:] = 1; xw[j, f["n"]:] = (0.0, 0.0, 10.0)
    idx = [(n + 5 if k in sc["bad"] else k) for k in order]
    d = dict(pose=torch.full((n, 12), POSE_FILL, dtype=torch.float32, device=dev), inlier=torch.full((n, nf), FLAG_FILL, dtype=torch.uint8, device=dev),
             ninl=torch.full((n,), INT_FILL, dtype=torch.int32, device=dev), its=torch.full((n,), INT_FILL, dtype=torch.int32, device=dev),
             hyp_pose=torch.full((n, mi, 12), POSE_FILL, dtype=torch.float32, device=dev), hyp_n=torch.full((n, mi), INT_FILL, dtype=torch.int32, device=dev))
    ddraws = torch.from_numpy(np.ascontiguousarray(draws[order]).view(np.int32)).to(dev)
    st = torch.cuda.Stream() if stream else None
    if st is not None:
        st.wait_stream(torch.cuda.current_stream())
    tr.solve_pnp(block, torch.tensor(idx, dtype=torch.int32, device=dev), torch.from_numpy(xw).to(dev), torch.from_numpy(has).to(dev), ddraws,
                 d["pose"], d["inlier"], d["ninl"], max_iterations=mi, probability=p["probability"], min_inliers=p["min_inliers"], epsilon=p["epsilon"],
                 th2=p["th2"], iterations=d["its"], hyp_poses=d["hyp_pose"] if hyp else None, hyp_ninliers=d["hyp_n"] if hyp else None,
                 stream_ptr=st.cuda_stream if st is not None else None)
    torch.cuda.synchronize()
    inv = np.argsort(order)
    return {k: v.cpu().numpy()[inv] for k, v in d.items()}


_RUNS = {}


def device_run(iv, name):
    """the device's answer on a scenario, computed once and shared among the tests"""
    if name not in _RUNS:
        _RUNS[name] = run_pnp(iv, SCENARIOS[name])
    return _RUNS[name]


def band(pose12, X, uv, e2):
    """how far error2 of each point can move when the double pose is narrowed to float: every entry of R and t moves by at most 2^-24 of its
    magnitude (|R| <= 1), so a camera coordinate moves by d <= 2^-24 (|X|_1 + |t|_inf), and as much again in the float rounding of Xc, Yc,
    invZc; a pixel coordinate by dp <= fx d (1 + |Xc / Zc|) / |Zc| per axis; error2 by 2 sqrt(2 error2) dp + 2 dp^2, plus its own rounding.
    A factor 4 on d covers the three coordinates and the roundings."""
    T = np.asarray(pose12, np.float64).reshape(3, 4)
    Xd = X.astype(np.float64)
    with np.errstate(all="ignore"):
        Pc = Xd @ T[:, :3].T + T[:, 3]
        d = 4 * 2.0 ** -24 * (np.abs(Xd).sum(1) + np.abs(T[:, 3]).max() + np.abs(Pc).max(1))
        dp = float(S.CAM["fx"]) * d * (1 + np.abs(Pc[:, 0] / Pc[:, 2]) + np.abs(Pc[:, 1] / Pc[:, 2])) / np.abs(Pc[:, 2])
        e = e2.astype(np.float64)
        return 2 * np.sqrt(2 * e) * dp + 2 * dp * dp + 4 * np.spacing(e2).astype(np.float64)


def hypotheses(got, k, its, X, uv, me):
    """per iteration: (mask without the banded points, indices of the banded points, device count)"""
    out = []
    for it in range(its):
        pose = got["hyp_pose"][k, it]
        T = pose.astype(np.float64).reshape(3, 4)
        mask, e2 = R.check_inliers(T[:, :3], T[:, 3], X, uv, me, S.CAM)
        with np.errstate(all="ignore"):
            near = np.abs(e2.astype(np.float64) - me.astype(np.float64)) <= band(pose, X, uv, e2)
        near &= np.isfinite(e2)
        lo = int((mask & ~near).sum()); hi = int((mask | near).sum()); cnt = int(got["hyp_n"][k, it])
        assert lo <= cnt <= hi, "iteration %d: the device counted %d inliers, numpy %d..%d on its pose" % (it, cnt, lo, hi)
        out.append((mask & ~near, np.nonzero(near)[0], cnt))
    return out


def outcomes(hyps, got, k, X, uv, me, n_min, its):
    """every result the bookkeeping of :213-259 can reach over the device's hypotheses (one, unless a banded point sits in a hypothesis that
    raises mnBestInliers)"""
    res = []

    def walk(it0, best, best_it, best_mask):
        for it in range(it0, its):
            base, near, cnt = hyps[it]
            if cnt >= n_min and cnt > best:
                need = cnt - int(base.sum())
                assert len(near) <= 8
                for extra in R.subsets(list(near), need):
                    m = base.copy(); m[list(extra)] = True
                    ok, Rr, tr, mask, c = R.refine(X, uv, me, S.CAM, m, n_min)
                    if ok:
                        res.append(dict(pose=R.pose12(Rr, tr), mask=mask, ninliers=c, iterations=it + 1, refined=True, best_it=it))
                    else:
                        walk(it + 1, cnt, it, m)
                return
        if best_it >= 0:
            res.append(dict(pose=got["hyp_pose"][k, best_it], mask=best_mask, ninliers=best, iterations=its, refined=False, best_it=best_it))
        else:
            res.append(dict(pose=None, mask=np.zeros(len(X), bool), ninliers=0, iterations=its, refined=False, best_it=-1))
    walk(0, 0, -1, None)
    return res


def flags_of(fr, nf, idx, mask):
    f = np.zeros(nf, np.uint8)
    f[idx[mask]] = 1
    return f


def check_frame(name, k, fr, sc, got, g):
    nf = sc["nf"]
    idx, X, uv, s2 = S.correspondences(fr)
    me = R.max_error(s2, sc["params"]["th2"])
    n_min, its, _ = R.ransac_parameters(len(X), **{q: sc["params"][q] for q in ("probability", "min_inliers", "max_iterations", "epsilon")})
    assert (n_min, its) == (fr["n_min"], fr["max_its"])
    untouched = np.full(12, POSE_FILL, F).tobytes()
    if its == 0:                                                           # N < mRansacMinInliers (:177-181)
        assert got["ninl"][k] == 0 and got["its"][k] == 0 and got["pose"][k].tobytes() == untouched and not got["inlier"][k].any()
        assert (got["hyp_n"][k] == INT_FILL).all()
        return
    assert (got["hyp_n"][k, its:] == INT_FILL).all() and (got["hyp_pose"][k, its:] == POSE_FILL).all(), "a hypothesis past mRansacMaxIts was written"
    hyps = hypotheses(got, k, its, X, uv, me)
    outs = outcomes(hyps, got, k, X, uv, me, n_min, its)
    floor_rot, floor_trans = g["floor_rot"], g["floor_trans"]
    borderline = set(g["borderline"].get(str(k), []))
    fails = []
    for o in outs:
        why = None
        if got["ninl"][k] != o["ninliers"] and not borderline:
            why = "ninliers %d vs %d" % (got["ninl"][k], o["ninliers"])
        elif abs(int(got["ninl"][k]) - o["ninliers"]) > len(borderline):
            why = "ninliers"
        elif got["its"][k] != o["iterations"]:
            why = "iterations %d vs %d" % (got["its"][k], o["iterations"])
        elif o["pose"] is None:
            if got["pose"][k].tobytes() != untouched or got["inlier"][k].any():
                why = "no pose, but something was written"
        else:
            diff = np.nonzero(got["inlier"][k] != flags_of(fr, nf, idx, o["mask"]))[0]
            if not set(int(i) for i in diff) <= borderline:
                why = "flags differ at %r" % diff[:8]
            elif o["refined"]:
                rot, trn = PR.pose_difference(got["pose"][k], o["pose"])
                print("%s frame %d: N %d, %d iterations of %d, %d inliers, Refine pose vs replay %.3g rad %.3g (bound %.3g / %.3g)" %
                      (name, k, len(X), got["its"][k], its, got["ninl"][k], rot, trn, 4 * floor_rot, 4 * floor_trans))
                if not (rot <= 4 * floor_rot and trn <= 4 * floor_trans):
                    why = "pose %.3g rad %.3g off the replay's" % (rot, trn)
            elif got["pose"][k].tobytes() != got["hyp_pose"][k, o["best_it"]].tobytes():
                why = "the unrefined pose is not the best hypothesis's"
        if why is None:
            break
        fails.append(why)
    else:
        raise AssertionError("%s frame %d: %r" % (name, k, fails))
    if o["pose"] is None:
        print("%s frame %d: N %d, %d iterations, no pose" % (name, k, len(X), its))
    # planted truth
    if o["refined"] and fr["share"] >= 0.7 and fr["kind"] in (None, "tail"):
        assert np.array_equal(got["inlier"][k], flags_of(fr, nf, idx, fr["planted"][idx])), (name, k)
        gt = PR.pose_difference(o["pose"], fr["pose_gt"])                      # the replay's Refine solved on the same inlier set
        grot, gtr = PR.pose_difference(got["pose"][k], fr["pose_gt"])
        assert grot <= gt[0] + 4 * floor_rot and gtr <= gt[1] + 4 * floor_trans, (name, k, grot, gtr, gt)


@pytest.mark.parametrize("name", sorted(n for n, s in SCENARIOS.items() if not s["degenerate"]))
def test_scenario_replayed_on_the_restatement(iv, name):
    """N = 0 / 3 / 9 (no pose, nothing but the count written) / 10 (one iteration, Refine cannot succeed: the pose is the hypothesis's, to the
    bit) / 11 / 15 / 64 / 65 / 257 / 1000, nfeatures 1000 and 4096, n_frames 1 / 3 / max_pairs, inlier shares 1.0 / 0.7 / 0.4 (with and without
    a pose), a bad record index (-1, nothing of the frame written), has_point set past the record's count; planted truth for shares >= 0.7"""
    sc = SCENARIOS[name]
    g = NOISE[name]
    assert sum(len(v) for v in g["borderline"].values()) <= 0.01 * g["n_points"]
    got = device_run(iv, name)
    for k, fr in enumerate(sc["frames"]):
        if k in sc["bad"]:
            assert got["ninl"][k] == -1 and got["its"][k] == INT_FILL and got["pose"][k].tobytes() == np.full(12, POSE_FILL, F).tobytes()
            assert (got["inlier"][k] == FLAG_FILL).all() and (got["hyp_n"][k] == INT_FILL).all(), "a bad record index leaves the frame untouched"
            continue
        check_frame(name, k, fr, sc, got, g)


def test_degenerate_scenes_return_and_are_self_consistent(iv):
    """a plane, points behind the camera, NaN world points: the call returns; each frame has no pose or a finite one whose flags are a numpy
    CheckInliers of that pose, outside a 1e-3 relative band of the threshold (termination and self-consistency, not agreement)"""
    sc = SCENARIOS["degenerate"]
    got = device_run(iv, "degenerate")
    for k, fr in enumerate(sc["frames"]):
        idx, X, uv, s2 = S.correspondences(fr)
        me = R.max_error(s2, sc["params"]["th2"])
        print("degenerate frame %d (%s): %d inliers after %d iterations" % (k, fr["kind"], got["ninl"][k], got["its"][k]))
        if got["ninl"][k] == 0:
            assert got["pose"][k].tobytes() == np.full(12, POSE_FILL, F).tobytes() and not got["inlier"][k].any()
            continue
        assert got["ninl"][k] >= fr["n_min"] and np.isfinite(got["pose"][k]).all()
        T = got["pose"][k].astype(np.float64).reshape(3, 4)
        mask, e2 = R.check_inliers(T[:, :3], T[:, 3], X, uv, me, S.CAM)
        with np.errstate(all="ignore"):
            clear = np.isfinite(e2) & (np.abs(e2.astype(np.float64) - me) > 1e-3 * me)
        assert np.array_equal(got["inlier"][k][idx][clear], mask[clear].astype(np.uint8))
        assert not got["inlier"][k][idx][~np.isfinite(e2)].any() and got["inlier"][k].sum() == got["ninl"][k]
        assert not np.delete(got["inlier"][k], idx).any()


def test_runs_are_bit_identical_on_any_stream_and_in_any_frame_order(iv):
    name = "share_07"
    sc = SCENARIOS[name]
    a = device_run(iv, name)
    tr = make_tracker(iv, sc["nf"], sc["max_pairs"])
    b = run_pnp(iv, sc, tracker=tr)
    c = run_pnp(iv, sc, stream=True, tracker=tr)
    d = run_pnp(iv, sc, order=[2, 0, 1], tracker=tr)
    e = run_pnp(iv, sc, hyp=False)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), "%s differs between two runs" % key
        assert a[key].tobytes() == c[key].tobytes(), "%s differs on a non-default stream" % key
        assert a[key].tobytes() == d[key].tobytes(), "%s differs under another frame order" % key
        if not key.startswith("hyp"):
            assert a[key].tobytes() == e[key].tobytes(), "%s differs without the hypothesis outputs" % key


def test_sampler_draws_the_four_points_of_the_restatement(iv):
    """tests/pnp_scenes.py:sampler_scene: frame 1 + j carries a NaN in the world point of correspondence j, so the frames whose hypothesis
    `it` is non-finite are the four points k_pnp_hyp sampled in iteration `it` (tests/test_pnp_cpu.py shows that compute_pose behaves so and
    that the no_swap and the stride-3 misreadings give other sets).  Every iteration, the planted rows among them: the back drawn first,
    positions an earlier removal rewrote, all-0 and all-RAND_MAX rows, bit 31 set"""
    sc = S.sampler_scene()
    got = run_pnp(iv, sc)
    N, its, draws = sc["frames"][0]["N"], sc["frames"][0]["max_its"], sc["draws"][0]
    bad = ~np.isfinite(got["hyp_pose"][:, :its]).all(2)                        # [13, its]
    assert not bad[0].any(), "the clean frame has a finite pose in every iteration"
    for it in range(its):
        want = set(RR.sample_indices(N, draws[it], 4))
        tagged = set(int(j) for j in np.nonzero(bad[1:, it])[0])
        name = sc["rows"][it][0] if it < len(sc["rows"]) else "random"
        assert tagged == want, "iteration %d (%s): the device sampled %r, the restatement %r" % (it, name, sorted(tagged), sorted(want))
    assert (got["hyp_n"][:, :its][bad] == 0).all(), "a non-finite hypothesis has no inlier"


def test_arguments_are_checked(iv):
    sc = dict(SCENARIOS["has_past_count"])
    for bad in (dict(max_iterations=0), dict(max_iterations=301), dict(probability=1.0), dict(epsilon=1.5), dict(th2=0.0)):
        with pytest.raises(iv.IvfError):
            run_pnp(iv, dict(sc, params=dict(sc["params"], **bad)))
    with pytest.raises(iv.IvfError):
        run_pnp(iv, dict(sc, frames=sc["frames"] * 2))                      # n_frames > max_pairs


def test_chain_search_by_bow_points_solve_pnp_optimize_pose(iv):
    """the relocalization chain without leaving the device, on the construction of tests/test_gpu_track_bow.py's chain test (a current frame
    that observes known world points, a keyframe that holds them in shuffled order): search_by_bow -> points_from_keyframe -> solve_pnp ->
    has_point & inlier -> optimize_pose, the pose buffer starting from ZERO instead of the keyframe's pose.  solve_pnp finds >= 10 inliers on
    every pair whose search found >= 15 matches; the optimised pose agrees with tests/pose_opt_ref.py fed with the same inputs within the 4
    float quanta that file's chain uses (its distance to the truth is printed next to that of the optimisation started from the keyframe's pose)."""
    import torch
    from iv_slam_amd import dist as ivd
    import oracle_lib as O
    import pose_opt_scenes as PS
    import track_bow_scenes as TS
    from test_gpu_track_bow import vocabulary, NF
    dev = torch.device("cuda:0")
    tree = TS.TREES[3]
    V = vocabulary(iv, tree)
    fr = PS.make_frame(77, 200, 200, "mixed", noise=0.5, n_outliers=6)
    b = TS.Builder(tree, 9)
    n = fr["n"]
    perm = b.rng.permutation(n)
    pay = [b.payload() for _ in range(n)]
    node = [b.nodes[i % len(b.nodes)] for i in range(n)]
    fdesc = np.stack([b.desc(node[i], pay[i]) for i in range(n)])
    kdesc = np.zeros((n, 32), np.uint8); kxw = np.zeros((3, NF, 3), F)
    for i in range(n):
        kdesc[perm[i]] = b.desc(node[i], b.flipped(pay[i], b.pick(2)))
        kxw[1, perm[i]] = fr["xw"][i]
    kf = dict(kps=fr["kps"][perm.argsort()], desc=kdesc, has=(np.arange(n) % 10 != 3).astype(np.uint8))
    sc = dict(name="chain", tree=tree, levelsup=1, kf=kf, f=dict(kps=fr["kps"], desc=fdesc))
    recK, _ = TS.records_of(sc)
    recF = dict(kps=fr["kps"], desc=fdesc, uright=fr["uright"], depth=fr["depth"])
    recs = [recF, recK, recF]
    pairs = [(1, 0), (7, 2), (1, 2)]
    tr = iv.BatchTracker(NF, PS.SCALE, float(PS.CAM["fx"]), float(PS.CAM["fy"]), float(PS.CAM["cx"]), float(PS.CAM["cy"]), float(PS.CAM["bf"]), PS.BOUNDS, max_pairs=3)
    block = torch.from_numpy(ivd.pack_records(recs, NF).reshape(-1)).to(dev)
    dp = torch.tensor(pairs, dtype=torch.int32, device=dev)
    assign = torch.full((3, NF), -7, dtype=torch.int32, device=dev); nm = torch.full((3,), -7, dtype=torch.int32, device=dev)
    xw = torch.full((3, NF, 3), 7.0, dtype=torch.float32, device=dev); has = torch.full((3, NF), 7, dtype=torch.uint8, device=dev)
    cur = dp[:, 1].contiguous()
    poses = torch.zeros((3, 12), dtype=torch.float32, device=dev)
    inl = torch.full((3, NF), 9, dtype=torch.uint8, device=dev); npnp = torch.full((3,), -7, dtype=torch.int32, device=dev)
    outl = torch.full((3, NF), 9, dtype=torch.uint8, device=dev); ninl = torch.full((3,), -7, dtype=torch.int32, device=dev)
    from iv_slam_amd import track
    draws = torch.from_numpy(track.pnp_draws(3, 300, 5).view(np.int32)).to(dev)
    tr.search_by_bow(V, block, dp, assign, nm, levelsup=1)
    tr.points_from_keyframe(dp, torch.from_numpy(kxw).to(dev), assign, xw, has)
    tr.solve_pnp(block, cur, xw, has, draws, poses, inl, npnp)
    pnp_pose = poses.clone()
    has2 = has & inl
    tr.optimize_pose(block, cur, xw, has2, poses, outl, ninl)
    torch.cuda.synchronize()
    nm = nm.cpu().numpy(); npnp = npnp.cpu().numpy(); xw = xw.cpu().numpy(); has2 = has2.cpu().numpy(); pnp_pose = pnp_pose.cpu().numpy()
    poses = poses.cpu().numpy(); outl = outl.cpu().numpy(); ninl = ninl.cpu().numpy()
    assert nm[0] >= 15 and nm[2] >= 15 and nm[1] == -1
    q = float(np.sqrt(3.0) * 2.0 ** -23)
    ref_kf = PR.pose_optimization(fr["kps"], n, fr["uright"], PS.INV_SIGMA2, PS.CAM["fx"], PS.CAM["fy"], PS.CAM["cx"], PS.CAM["cy"], PS.CAM["bf"], xw[0][:n],
                                  (xw[0][:n] != 0).any(1).astype(np.uint8), None, 4, fr["pose_in"])
    kf_rot, kf_tr = PR.pose_difference(ref_kf["pose"], fr["pose_gt"])
    for p in (0, 2):
        assert npnp[p] >= 10, "solve_pnp found %d inliers on %d matches" % (npnp[p], nm[p])
        ref = PR.pose_optimization(fr["kps"], n, fr["uright"], PS.INV_SIGMA2, PS.CAM["fx"], PS.CAM["fy"], PS.CAM["cx"], PS.CAM["cy"], PS.CAM["bf"], xw[p][:n], has2[p][:n],
                                   None, 4, pnp_pose[p])
        rot, trn = PR.pose_difference(poses[p], ref["pose"])
        grot, gtr = PR.pose_difference(poses[p], fr["pose_gt"])
        print("chain pair %d: %d matches, PnP %d inliers, optimised %d; vs restatement %.3g rad %.3g; vs truth %.3g rad %.3g (from the keyframe's pose: %.3g %.3g)" %
              (p, nm[p], npnp[p], ninl[p], rot, trn, grot, gtr, kf_rot, kf_tr))
        assert rot <= 4 * q and trn <= 4 * q
        assert np.array_equal(outl[p, :n], ref["outlier"][:n]) and ninl[p] == ref["ninliers"] and ninl[p] > 100
    assert npnp[1] == 0 and ninl[1] == 0 and not poses[1].any()
