"""ivf_tracker_optimize_pose (iv_slam_amd/csrc/ivf_pose.hip) -- Optimizer::PoseOptimization (ORB/src/Optimizer.cc:251-503) with the
quality-scaled Huber kernels, one workgroup per frame -- against tests/pose_opt_ref.py, the f64 restatement (g2o cannot be built here),
on the scenarios of tests/pose_opt_scenes.py.

Tolerance: the pose agrees with the restatement within 4 x the floor committed in tests/golden/pose_opt_noise.json (the restatement's own
spread under 8 random summation orders, not below the float quantum of the output pose; see tests/test_pose_opt_cpu.py); mvbOutlier and
the inlier count are equal except on the edges that file lists as borderline (none, for the seeds chosen).  Noise-free scenarios: the
flags are the planted set and the pose is within (the restatement's distance to the truth + 4 x floor) of the truth."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O
import pose_opt_ref as PR
import pose_opt_scenes as S
from test_gpu_track import extracted_sequence, frame_dict, run_tracker, iv  # noqa: F401  (iv: the module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
F = np.float32
NOISE = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_opt_noise.json")))
SCENARIOS = S.scenarios()
_REF = {}


def reference(name):
    """the restatement of every frame of a scenario, computed once and shared"""
    if name not in _REF:
        sc = SCENARIOS[name]
        _REF[name] = [S.reference(fr, sc["n_rounds"]) for fr in sc["frames"]]
    return _REF[name]


def make_tracker(iv, nf, max_pairs, cam=None):
    c = cam or dict(S.CAM, scale=S.SCALE, bounds=S.BOUNDS)
    return iv.BatchTracker(nf, c["scale"], float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), float(c["bf"]), c["bounds"], max_pairs=max_pairs)


def run_optimize(iv, frames, nf, n_rounds, max_pairs, bad=(), with_quality=None, tracker=None):
    """frames: list of scene dicts -> dict of device results as numpy; slots in `bad` get a record index outside the block; a frame with
    has_tail = 1 gets has_point = 1 and a point 10 m ahead on every slot past its record's count"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    n = len(frames)
    block = torch.from_numpy(ivd.pack_records([dict(kps=f["kps"], desc=f["desc"], uright=f["uright"], depth=f["depth"]) for f in frames], nf).reshape(-1)).to(dev)
    tr = tracker or make_tracker(iv, nf, max_pairs)
    idx = [(n + 5 if k in bad else k) for k in range(n)]
    xw = np.zeros((n, nf, 3), F); has = np.zeros((n, nf), np.uint8); q = np.ones((n, nf), F); poses = np.zeros((n, 12), F)
    for k, f in enumerate(frames):
        xw[k, :f["n"]] = f["xw"]; has[k, :f["n"]] = f["has"]; poses[k] = f["pose_in"]
        if f["quality"] is not None:
            q[k, :f["n"]] = f["quality"]
        if f.get("has_tail"):
            has[k, f["n"]:] = 1; xw[k, f["n"]:] = (0.0, 0.0, 10.0)
    use_q = with_quality if with_quality is not None else any(f["quality"] is not None for f in frames)
    d = dict(frames=torch.tensor(idx, dtype=torch.int32, device=dev), xw=torch.from_numpy(xw).to(dev), has=torch.from_numpy(has).to(dev),
             q=torch.from_numpy(q).to(dev) if use_q else None, poses=torch.from_numpy(poses).to(dev),
             outlier=torch.full((n, nf), 9, dtype=torch.uint8, device=dev), ninl=torch.full((n,), -7, dtype=torch.int32, device=dev),
             chi2=torch.full((n, nf), -3.0, dtype=torch.float32, device=dev))
    tr.optimize_pose(block, d["frames"], d["xw"], d["has"], d["poses"], d["outlier"], d["ninl"], quality=d["q"], n_rounds=n_rounds, chi2=d["chi2"])
    torch.cuda.synchronize()
    return dict(pose=d["poses"].cpu().numpy(), outlier=d["outlier"].cpu().numpy(), ninl=d["ninl"].cpu().numpy(), chi2=d["chi2"].cpu().numpy())


def check_frame(name, k, fr, ref, got, floor_rot, floor_trans, borderline):
    ne = len(ref["edges"])
    rot, tr = PR.pose_difference(got["pose"][k], ref["pose"])
    print("%s frame %d: %d edges, pose vs restatement %.3g rad %.3g (bound %.3g / %.3g), inliers %d vs %d" %
          (name, k, ne, rot, tr, 4 * floor_rot, 4 * floor_trans, got["ninl"][k], ref["ninliers"]))
    if ne < 3:
        assert got["ninl"][k] == 0 and got["pose"][k].tobytes() == fr["pose_in"].tobytes() and not got["outlier"][k].any()
        return
    assert rot <= 4 * floor_rot and tr <= 4 * floor_trans, (name, k, rot, tr)
    n = fr["n"]
    diff = np.nonzero(got["outlier"][k, :n] != ref["outlier"][:n])[0]
    assert set(int(i) for i in diff) <= set(borderline), "%s frame %d: mvbOutlier differs at %r" % (name, k, diff[:8])
    assert not got["outlier"][k, n:].any() and not got["outlier"][k, :n][fr["has"] == 0].any()
    assert not got["chi2"][k, n:].any(), "chi2 logged on a slot past the record's count"
    assert abs(int(got["ninl"][k]) - ref["ninliers"]) <= len(borderline) and (len(diff) > 0 or got["ninl"][k] == ref["ninliers"])
    if ref["chi2"] is not None:
        c = got["chi2"][k, :n]
        e = ref["edges"]
        assert not c[fr["has"] == 0].any()
        with np.errstate(all="ignore"):
            # chi2 = invSigma2 * |e|^2 (invSigma2 <= 1) moves with the pose: a pose within 4 x floor of the restatement's moves a residual by
            # at most de = 4 x floor x (fx + bf) px, and chi2 by 2 sqrt(chi2) de + de^2; plus the float rounding of the output
            de = 4 * (floor_rot + floor_trans) * (float(S.CAM["fx"]) + float(S.CAM["bf"]))
            r64 = ref["chi2"][e].astype(np.float64)
            tol = 2 * np.sqrt(r64) * de + de * de + 4 * np.spacing(ref["chi2"][e]).astype(np.float64)
        assert (np.abs(c[e].astype(np.float64) - ref["chi2"][e]) <= tol).all(), (name, k)
    if fr["noise_free"]:
        assert np.array_equal(got["outlier"][k, :n], fr["planted"]), (name, k)
        g = NOISE[name]
        grot, gtr = PR.pose_difference(got["pose"][k], fr["pose_gt"])
        assert grot <= g["gt_rot"] + 4 * floor_rot and gtr <= g["gt_trans"] + 4 * floor_trans, (name, k, grot, gtr)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_against_the_restatement(iv, name):
    """edge counts 0 / 2 / 3 / 9 / 10 / 63 / 64 / 65 / 257 / 1000 of 4096, mono / stereo / mixed, n_rounds 1..4, n_frames 1 / 3 /
    max_pairs, every quality mode, one bad record index; rotations of 119..180 degrees and exact axis permutations (every case of
    Quaterniond(Matrix3d), the sign flip of normalizeRotation), points behind the camera, negative quality (failed solves, the pose
    stays), has_point set past the record's count; and a second run is bit-identical to the first"""
    sc = SCENARIOS[name]
    g = NOISE[name]
    assert sum(len(v) for v in g["borderline"].values()) <= 0.01 * g["n_edges"]
    refs = reference(name)
    got = run_optimize(iv, sc["frames"], sc["nf"], sc["n_rounds"], sc["max_pairs"], bad=sc["bad"])
    for k, fr in enumerate(sc["frames"]):
        if k in sc["bad"]:
            assert got["ninl"][k] == -1 and got["pose"][k].tobytes() == fr["pose_in"].tobytes(), "a bad record index leaves the pose untouched"
            continue
        check_frame(name, k, fr, refs[k], got, g["floor_rot"], g["floor_trans"], g["borderline"].get(str(k), []))
    again = run_optimize(iv, sc["frames"], sc["nf"], sc["n_rounds"], sc["max_pairs"], bad=sc["bad"])
    for key in ("pose", "outlier", "ninl", "chi2"):
        assert got[key].tobytes() == again[key].tobytes(), "%s: %s differs between two runs" % (name, key)


def test_quality_of_one_is_no_quality_and_rounds_are_checked(iv):
    sc = SCENARIOS["quality_None"]
    a = run_optimize(iv, sc["frames"], 64, 4, 1, with_quality=False); b = run_optimize(iv, sc["frames"], 64, 4, 1, with_quality=True)
    for key in ("pose", "outlier", "ninl", "chi2"):
        assert a[key].tobytes() == b[key].tobytes()
    for r in (0, 5):
        with pytest.raises(iv.IvfError):
            run_optimize(iv, sc["frames"], 64, r, 1)
    with pytest.raises(iv.IvfError):
        run_optimize(iv, sc["frames"] * 2, 64, 4, 1)                       # n_frames > max_pairs


def test_conversion_only_is_the_restatement_to_the_bit(iv):
    """the scenario in which nothing is optimised (quality 0, one round): the device pose is Converter::toCvMat(Converter::toSE3Quat(input)),
    a few dozen double operations with no sum over edges in them, so it equals the restatement's bit for bit -- each hand-written case of
    Quaterniond(Matrix3d) compared directly, not through a Levenberg-Marquardt that would repair a wrong start.  sqrt and the divisions
    are correctly rounded in double on both sides and nothing is fused (-ffp-contract=off)."""
    sc = SCENARIOS["conversion_only"]
    refs = reference("conversion_only")
    got = run_optimize(iv, sc["frames"], sc["nf"], sc["n_rounds"], sc["max_pairs"])
    for k, fr in enumerate(sc["frames"]):
        q, t = PR.se3_from_pose(fr["pose_in"])
        assert refs[k]["pose"].tobytes() == PR.pose_from_se3(q, t).tobytes()
        assert got["pose"][k].tobytes() == refs[k]["pose"].tobytes(), (k, got["pose"][k], refs[k]["pose"])
        assert np.array_equal(got["outlier"][k], refs[k]["outlier"]) and got["ninl"][k] == refs[k]["ninliers"]
        assert got["chi2"][k].tobytes() == refs[k]["chi2"].tobytes(), k


def zero_depth_frame():
    """a scene moved into its camera's frame (input pose = identity, world points = their camera coordinates narrowed to float), 40 edges,
    one of them with z = 0.0f: the identity quaternion maps a point to itself exactly, so P[2] is exactly 0"""
    fr = S.make_frame(901, 64, 40, "mixed", 1.0, 0, prior=(0, 0))
    T = fr["pose_gt"].reshape(3, 4)
    fr["xw"] = (fr["xw"].astype(np.float64) @ T[:, :3].T + T[:, 3]).astype(F)
    fr["pose_in"] = np.eye(4, dtype=F)[:3].reshape(12).copy()
    fr["pose_gt"] = fr["pose_in"].astype(np.float64)
    k = int(np.nonzero(fr["has"])[0][17])
    fr["xw"][k, 2] = F(0.0)
    return fr, k


def test_zero_depth_point_is_contained(iv):
    """the kernel's claim "NaN input cannot spin the kernel", once: frame A holds a point with z = 0.0f exactly at the identity input pose.
    Its invz is infinite, its Huber weight 0, every entry of H is 0 * inf = NaN, the solve returns NaN, every trial pose and every chi2 at it
    is NaN; NaN compares false everywhere (levenberg.cpp:134, :149, :151, :155; Optimizer.cc:432, :469), so no trial is accepted, no edge is
    an outlier and the estimate never moves.  Expected, from the restatement: the pose has the input's bits, no outliers, ninliers == nE,
    chi2 NaN where the restatement's is.  Frame B, an ordinary frame in the same launch, agrees with its restatement as ever; a second
    run is bit-identical.  Not a scenario: spread_and_borderline marks every edge of a frame with non-finite chi2 borderline."""
    A, kz = zero_depth_frame()
    sc = SCENARIOS["quality_None"]
    B = sc["frames"][0]
    with np.errstate(all="ignore"):
        refA = S.reference(A, 4)
    ne = int(A["has"].sum())
    assert ne == 40 and A["xw"][kz, 2] == 0 and A["has"][kz] == 1
    assert refA["pose"].tobytes() == A["pose_in"].tobytes() and not refA["outlier"].any() and refA["ninliers"] == ne
    assert np.isnan(refA["chi2"][kz]) and not np.isnan(refA["chi2"][A["has"] == 0]).any()
    got = run_optimize(iv, [A, B], 64, 4, 2)
    print("zero depth: device inliers %d, NaN chi2 on %d edges (restatement %d), pose %r" %
          (got["ninl"][0], int(np.isnan(got["chi2"][0]).sum()), int(np.isnan(refA["chi2"]).sum()), got["pose"][0]))
    assert got["pose"][0].tobytes() == A["pose_in"].tobytes()
    assert not got["outlier"][0].any() and got["ninl"][0] == ne
    assert np.array_equal(np.isnan(got["chi2"][0]), np.isnan(refA["chi2"]))
    assert np.isnan(refA["chi2"][A["has"] != 0]).all() and not got["chi2"][0][A["has"] == 0].any()      # all 40 edges; 0 where there is no point
    g = NOISE["quality_None"]
    check_frame("zero depth, frame B", 1, B, reference("quality_None")[0], got, g["floor_rot"], g["floor_trans"], g["borderline"].get("0", []))
    again = run_optimize(iv, [A, B], 64, 4, 2)
    for key in ("pose", "outlier", "ninl", "chi2"):
        assert got[key].tobytes() == again[key].tobytes(), key


def test_points_from_pairs_edges(iv):
    """ivf_tracker_points_from_pairs on its own, nf = 70 (not a multiple of the block), poses = NULL (identity): a last-record index outside
    the block, assign = -1 / exactly the last record's count / past it / past nf, last keypoints with depth -1 and 0.  The last records hold
    keypoints with depth on every slot, also past their count.  Bit-exact against projection_oracle.unproject_stereo with T = I; has == 0
    and xw == 0 everywhere else."""
    import torch
    import projection_oracle as PO
    from iv_slam_amd import dist as ivd
    nf = 70
    dev = torch.device("cuda:0")
    counts = [60, 70, 33]
    recs = []
    for k in range(3):
        fr = S.make_frame(910 + k, nf, nf, "stereo")
        recs.append(dict(kps=fr["kps"], desc=fr["desc"], uright=fr["uright"], depth=fr["depth"].copy()))
    recs[0]["depth"][[5, 6]] = (-1.0, 0.0); recs[1]["depth"][[0, 69]] = (0.0, -1.0)
    raw = ivd.pack_records(recs, nf)
    for k, c in enumerate(counts):
        raw[k, :4] = np.array([c], np.int32).view(np.uint8)                       # the slots from the count on keep their keypoints and depth
    pairs = [(0, 1), (5, 2), (1, 0)]                                             # (last, current); record 5 does not exist
    rng = np.random.default_rng(4)
    assign = rng.integers(-1, nf + 3, (3, nf)).astype(np.int32)
    assign[0, :8] = (-1, 60, 61, 69, 70, 1 << 30, 5, 6); assign[0, 69] = 59
    assign[2, :6] = (0, 69, 70, -1, -(1 << 31), 68)
    tr = make_tracker(iv, nf, 3)
    xw = torch.full((3, nf, 3), 7.0, dtype=torch.float32, device=dev); has = torch.full((3, nf), 7, dtype=torch.uint8, device=dev)
    tr.points_from_pairs(torch.from_numpy(raw.reshape(-1)).to(dev), torch.tensor(pairs, dtype=torch.int32, device=dev), torch.from_numpy(assign).to(dev),
                         xw, has, poses=None)
    torch.cuda.synchronize()
    xw = xw.cpu().numpy(); has = has.cpu().numpy()
    exw = np.zeros((3, nf, 3), F); ehas = np.zeros((3, nf), np.uint8)
    for p, (a, b) in enumerate(pairs):
        if not 0 <= a < 3:
            continue
        last = dict(kps=recs[a]["kps"], depth=recs[a]["depth"], T=np.eye(4, dtype=F), **{k: S.CAM[k] for k in ("fx", "fy", "cx", "cy")})
        for i in range(nf):
            j = int(assign[p, i])
            if 0 <= j < counts[a] and last["depth"][j] > 0:
                exw[p, i] = PO.unproject_stereo(last, j); ehas[p, i] = 1
    assert ehas[0].sum() > 20 and ehas[2].sum() > 20 and not ehas[1].any() and ehas[0, 69] == 1 and not ehas[0, :8].any() and ehas[2, :6].tolist() == [0, 0, 0, 0, 0, 1]
    assert has.tobytes() == ehas.tobytes()
    assert xw.tobytes() == exw.tobytes()


def test_points_from_local_is_exact(iv):
    import torch
    from iv_slam_amd._lib import LOCAL_POINT_DTYPE
    rng = np.random.default_rng(3)
    nf, n_frames = 70, 3
    dev = torch.device("cuda:0")
    off = np.array([0, 40, 40, 130], np.int32)
    pts = np.zeros(130, LOCAL_POINT_DTYPE); pts["pos"] = rng.normal(size=(130, 3)).astype(F)
    assign = np.full((n_frames, nf), -1, np.int32)
    for f in range(n_frames):
        m = off[f + 1] - off[f]
        if m:
            sel = rng.permutation(nf)[:30]; assign[f, sel] = rng.integers(0, m, 30)
    assign[2, 0] = 90                                                        # past the frame's range: no point
    tr = make_tracker(iv, nf, n_frames)
    xw = torch.full((n_frames, nf, 3), 7.0, dtype=torch.float32, device=dev); has = torch.full((n_frames, nf), 7, dtype=torch.uint8, device=dev)
    tr.points_from_local(torch.from_numpy(pts.view(np.uint8).reshape(-1)).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(assign).to(dev), xw, has)
    torch.cuda.synchronize()
    xw = xw.cpu().numpy(); has = has.cpu().numpy()
    for f in range(n_frames):
        for i in range(nf):
            a = assign[f, i]
            ok = 0 <= a < off[f + 1] - off[f]
            assert has[f, i] == (1 if ok else 0)
            assert xw[f, i].tobytes() == (pts["pos"][off[f] + a] if ok else np.zeros(3, F)).tobytes()


def test_chain_run_points_optimize_search_local(iv):
    """run -> points_from_pairs -> optimize_pose -> search_local at the optimised pose on 2 pairs of 500 features, never leaving the device,
    against the same chain through oracle/projection_oracle.py and the restatement.  points_from_pairs is bit-exact against
    projection_oracle.unproject_stereo.  The oracle's SearchLocalPoints runs at the pose the device produced, which the assertion before it
    ties to the restatement's within the noise floor."""
    import torch
    import projection_oracle as PO
    from iv_slam_amd import dist as ivd
    from test_gpu_track_local import check_local, map_points_from, pack_points
    cam, recs, _, _ = extracted_sequence(iv, 640, 240, 500, 3, seed=97, shift=3)
    nf = 500
    dev = torch.device("cuda:0")
    pairs = [(0, 1), (1, 2)]
    Tl = [PO_pose(0.4, [0.05, -0.02, 0.3]), PO_pose(-0.3, [0.0, 0.03, -0.2])]     # the last frames' poses; the prior of cur = the same (zero motion)
    pp = [(Tl[0], Tl[0]), (Tl[1], Tl[1])]
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    tr = iv.BatchTracker(nf, cam["scale"], float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam["bf"]), cam["bounds"],
                         max_pairs=2, b=float(cam["b"]))
    dp = torch.tensor(pairs, dtype=torch.int32, device=dev)
    dposes = torch.from_numpy(np.stack([np.stack([a[:3, :4].reshape(12), b[:3, :4].reshape(12)]) for a, b in pp]).astype(F)).to(dev)
    assign = torch.full((2, nf), -7, dtype=torch.int32, device=dev); nm = torch.full((2,), -7, dtype=torch.int32, device=dev)
    xw = torch.full((2, nf, 3), 7.0, dtype=torch.float32, device=dev); has = torch.full((2, nf), 7, dtype=torch.uint8, device=dev)
    cur = dp[:, 1].contiguous()
    opt = dposes[:, 1].contiguous().clone()
    outl = torch.full((2, nf), 9, dtype=torch.uint8, device=dev); ninl = torch.full((2,), -7, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(5)
    per_frame = [map_points_from(cam, recs[a], Tl[k], rng) for k, (a, b) in enumerate(pairs)]
    pts, off = pack_points(iv, per_frame)
    M = max(len(p) for p in per_frame)
    dpts = torch.from_numpy(pts.view(np.uint8).reshape(-1)).to(dev); doff = torch.from_numpy(off).to(dev)
    la = torch.full((2, nf), -7, dtype=torch.int32, device=dev); lnm = torch.full((2,), -7, dtype=torch.int32, device=dev)
    # ---- the chain: four calls, no synchronisation and no host copy between them
    tr.run(block, dp, assign, nm, poses=dposes)
    tr.points_from_pairs(block, dp, assign, xw, has, poses=dposes)
    tr.optimize_pose(block, cur, xw, has, opt, outl, ninl)
    tr.search_local(block, cur, dpts, doff, M, la, lnm, poses=opt, th=3.0)
    torch.cuda.synchronize()
    assign = assign.cpu().numpy(); xw = xw.cpu().numpy(); has = has.cpu().numpy(); opt = opt.cpu().numpy(); outl = outl.cpu().numpy(); ninl = ninl.cpu().numpy()
    inv_s2 = PR.inv_level_sigma2(cam["scale"])
    for k, (a, b) in enumerate(pairs):
        last = frame_dict(recs[a], pp[k][0], cam); curf = frame_dict(recs[b], pp[k][1], cam)
        n_or, exp = PO.track_with_motion_model_matches(O, curf, last, F(7.0), F(14.0), 20, True, 0.0, True, None)
        nC = len(curf["kps"])
        assert np.array_equal(assign[k, :nC], exp) and n_or > 50
        exw = np.zeros((nf, 3), F); ehas = np.zeros(nf, np.uint8)
        for i2 in range(nC):
            if exp[i2] >= 0 and last["depth"][exp[i2]] > 0:
                exw[i2] = PO.unproject_stereo(last, int(exp[i2])); ehas[i2] = 1
        assert has[k].tobytes() == ehas.tobytes() and xw[k].tobytes() == exw.tobytes(), "points_from_pairs is bit-exact"
        fr = dict(kps=recs[b]["kps"], n=nC, uright=recs[b]["uright"], xw=exw[:nC], has=ehas[:nC], quality=None, pose_in=pp[k][1][:3, :4].reshape(12).astype(F))
        ref = PR.pose_optimization(fr["kps"], nC, fr["uright"], inv_s2, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], fr["xw"], fr["has"], None, 4, fr["pose_in"])
        rot, trn = PR.pose_difference(opt[k], ref["pose"])
        q = float(np.sqrt(3.0) * 2.0 ** -23)                                 # the float quantum of the output pose (tests/test_pose_opt_cpu.py)
        print("chain pair %d: %d matches, %d edges, %d inliers (restatement %d), pose vs restatement %.3g rad %.3g" % (k, n_or, int(ehas.sum()), ninl[k], ref["ninliers"], rot, trn))
        assert rot <= 4 * q and trn <= 4 * q
        assert np.array_equal(outl[k, :nC], ref["outlier"][:nC]) and ninl[k] == ref["ninliers"] and ninl[k] > 30
    poses_by_record = {b: np.vstack([opt[k].reshape(3, 4), [[0, 0, 0, 1]]]).astype(F) for k, (a, b) in enumerate(pairs)}
    tot = check_local(cam, recs, [b for a, b in pairs], per_frame, poses_by_record, None, 3.0, 0.8, la.cpu().numpy(), lnm.cpu().numpy(), what="chain")
    assert tot > 50


def PO_pose(deg_y, t):
    from test_gpu_track import pose
    return pose(deg_y, t)
