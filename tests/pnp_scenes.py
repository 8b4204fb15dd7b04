"""pnp_scenes.py -- the seeded synthetic scenes of the PnPsolver tests (test infrastructure only), shared by tests/test_pnp_cpu.py (the
restatement tests/pnp_ref.py against itself and the planted truth, the noise floor in tests/golden/pnp_noise.json) and
tests/test_gpu_pnp.py (ivf_tracker_solve_pnp against the restatement), on the camera of tests/pose_opt_scenes.py.

A frame: nk keypoints, N of them hold a map point.  A known pose; world points at 3..40 m spread over the image (non-planar); planted
inliers observe their point with at most 0.5 px of noise per axis (error2 <= 0.5 against mvMaxError >= 5.991), planted outliers are moved
by 30..60 px (error2 >= 900 against mvMaxError <= 5.991 * 1.2^14 = 77): every point is at least 20 % away from its threshold."""
import math

import numpy as np

import pnp_ref as R
import pose_opt_scenes as PS

F = np.float32
CAM, SCALE, BOUNDS, KP_DTYPE, W, H = PS.CAM, PS.SCALE, PS.BOUNDS, PS.KP_DTYPE, PS.W, PS.H
SIGMA2 = R.level_sigma2(SCALE)
DEFAULTS = dict(probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991)


def make_frame(seed, nk, N, share=1.0, kind=None, params=None):
    """kind: None, "planar" (every world point on one plane), "behind" (a fifth of the points mirrored behind the camera), "nan" (three
    world points are NaN), "tail" (has_point = 1 and a point on the slots past the record's count)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (np.float64(CAM[k]) for k in ("fx", "fy", "cx", "cy"))
    Rg = PS.rot(rng.normal(size=3), rng.uniform(0, 25)); tg = rng.uniform(-2, 2, 3)
    u = rng.uniform(20, W - 20, nk); v = rng.uniform(20, H - 20, nk); z = rng.uniform(3, 40, nk)
    if kind == "planar":
        z = 12.0 + 0.004 * (u - cx) + 0.002 * (v - cy)                 # a plane in the camera frame
    octv = rng.integers(0, 8, nk)
    Pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    Xw = ((Pc - tg) @ Rg).astype(F)
    Pc = Xw.astype(np.float64) @ Rg.T + tg
    u = fx * Pc[:, 0] / Pc[:, 2] + cx; v = fy * Pc[:, 1] / Pc[:, 2] + cy
    u = u + rng.uniform(-0.5, 0.5, nk); v = v + rng.uniform(-0.5, 0.5, nk)
    has = np.zeros(nk, np.uint8)
    pts = np.sort(rng.permutation(nk)[:N])
    has[pts] = 1
    n_in = int(round(share * N))
    out = rng.permutation(pts)[:N - n_in]
    ang = rng.uniform(0, 2 * math.pi, len(out)); mag = rng.uniform(30, 60, len(out))
    u[out] += mag * np.cos(ang); v[out] += mag * np.sin(ang)
    planted = has.astype(bool); planted[out] = False
    if kind == "behind":
        sel = rng.permutation(pts)[:max(1, N // 5)]
        Pm = Xw[sel].astype(np.float64) @ Rg.T + tg; Pm[:, 2] = -Pm[:, 2]
        Xw[sel] = ((Pm - tg) @ Rg).astype(F)
        planted[sel] = False
    if kind == "nan":
        Xw[rng.permutation(pts)[:3], rng.integers(0, 3, 3)] = np.nan
    kp = np.zeros(nk, KP_DTYPE)
    kp["x"] = u.astype(F); kp["y"] = v.astype(F); kp["octave"] = octv; kp["size"] = 31
    Tgt = np.zeros((3, 4)); Tgt[:, :3] = Rg; Tgt[:, 3] = tg
    p = dict(DEFAULTS, **(params or {}))
    n_min, its, x = R.ransac_parameters(N, p["probability"], p["min_inliers"], p["max_iterations"], p["epsilon"])
    assert x is None or abs(x - round(x)) > 1e-6, "N = %d: log(1 - p) / log(1 - eps^3) = %r is too close to an integer" % (N, x)
    return dict(kps=kp, n=nk, uright=np.full(nk, -1.0, F), depth=np.full(nk, -1.0, F), desc=np.zeros((nk, 32), np.uint8), xw=Xw, has=has,
                planted=planted, pose_gt=Tgt.reshape(12), N=N, share=share, kind=kind, seed=seed, n_min=n_min, max_its=its)


def correspondences(fr):
    """what the constructor collects (:71-114): -> (keypoint indices, X [N,3], uv [N,2], sigma2 [N])"""
    idx = np.nonzero(fr["has"][:fr["n"]])[0]
    kp = fr["kps"][idx]
    return idx, fr["xw"][idx], np.stack([kp["x"], kp["y"]], 1), SIGMA2[kp["octave"]]


def R_draws(seed, n_frames, max_iterations):
    """the same array iv_slam_amd.track.pnp_draws returns (checked in tests/test_pnp_cpu.py)"""
    from iv_slam_amd import track
    return track.ransac_draws(n_frames, max_iterations, 4, seed)


def sampler_scene():
    """The scene that shows WHICH four points a hypothesis drew, without comparing poses: 13 frames with the same 12 correspondences and
    the same draws; frame 0 is clean, frame 1 + j has one coordinate of correspondence j's world point set to NaN.  compute_pose on a sample
    that holds the NaN point returns a non-finite pose and on any other a finite one, so the frames whose hypothesis `it` is non-finite name
    the sample of iteration `it`.  epsilon = 0.1 and min_inliers = 4 give mRansacMinInliers = 4, eps = 4 / 12 and 123 iterations, capped by
    max_iterations = 64.  The first rows of the draws are planted (`rows`: name, the draws, whether a draw reads a position an earlier
    removal rewrote), the rest come from ransac_draws.
    -> the scenario dict of scenarios() with draws [13, 64, 4], rows, and the sample a row was planted for (None: raw values)"""
    from iv_slam_amd import track
    N, RM = 12, R.RAND_MAX
    p = dict(DEFAULTS, epsilon=0.1, min_inliers=4, max_iterations=64)
    base = make_frame(701, 40, N, 1.0, params=p)
    idx = np.nonzero(base["has"])[0]
    frames = [base]
    for j in range(N):
        fr = dict(base, xw=base["xw"].copy())
        fr["xw"][idx[j], j % 3] = np.nan
        frames.append(fr)
    wanted = [("back_then_zero", [11, 0, 5, 7], False),                # the back first (it replaces itself), then index 0
              ("second_on_first", [2, 11, 4, 6], True),                # position 2 holds 11 after the first removal
              ("third_on_first", [2, 5, 11, 6], True),
              ("fourth_on_first", [2, 5, 7, 11], True),
              ("third_on_second", [2, 5, 10, 6], True),                # position 5 holds 10 after the second removal
              ("fourth_on_second", [2, 5, 7, 10], True),
              ("fourth_on_third", [2, 5, 7, 9], True),                 # position 7 holds 9 after the third removal
              ("last_after_rewrite", [9, 0, 11, 10], True),            # position 9 holds 11 and is the last one when the third draw reads it
              ("rewritten_back_moves", [10, 3, 11, 9], True)]          # position 10 holds 11, which the second removal moves on to position 3
    rows = [(name, R.draws_for(N, w), rew, w) for name, w, rew in wanted]
    rows += [("all_zero", np.zeros(4, np.uint32), True, None), ("all_rand_max", np.full(4, RM, np.uint32), False, None)]
    plain = R.draws_for(N, [3, 9, 0, 6])
    rows += [("bit31_clear", plain, False, [3, 9, 0, 6]), ("bit31_set", plain | np.uint32(0x80000000), False, [3, 9, 0, 6])]
    draws = track.ransac_draws(1, p["max_iterations"], 4, 18)[0]
    for it, row in enumerate(rows):
        draws[it] = row[1]
    assert base["max_its"] >= len(rows) + 36, "mRansacMaxIts covers the planted rows and three dozen random ones"
    return dict(nf=64, max_pairs=N + 1, bad=[], seed=18, params=p, degenerate=True, frames=frames, rows=rows,
                draws=np.repeat(draws[None], N + 1, 0))


def scenarios():
    """name -> dict(nf, max_pairs, frames, bad = slots given a record index outside the block, params, seed (of the draws),
    degenerate = termination and self-consistency only)"""
    S = {}
    counts = [0, 3, 9, 10, 11, 15, 64, 65]
    # every count around the early refusal (9 < min_inliers), mRansacMinInliers == N (10), the first Refine-able sizes, one wave and one
    # more; all inliers; one slot with a bad record index
    S["counts_all_inliers"] = dict(nf=1000, max_pairs=12, bad=[4], seed=11, params=dict(DEFAULTS), degenerate=False,
                                   frames=[make_frame(100 + k, 1000 if k % 2 else 700, c) for k, c in enumerate(counts[:4])] +
                                          [make_frame(150, 800, 40)] +
                                          [make_frame(100 + k, 1000 if k % 2 else 700, c) for k, c in enumerate(counts) if k >= 4])
    # 30 % outliers: several hypotheses before the first all-inlier sample; more than one point per lane, every slot of the record used
    S["share_07"] = dict(nf=1000, max_pairs=3, bad=[], seed=12, params=dict(DEFAULTS), degenerate=False,
                         frames=[make_frame(201, 900, 65, 0.7), make_frame(202, 1000, 257, 0.7), make_frame(203, 1000, 1000, 0.7)])
    # the largest record, sparsely filled; n_frames == max_pairs == 1
    S["sparse4096"] = dict(nf=4096, max_pairs=1, bad=[], seed=13, params=dict(DEFAULTS), degenerate=False,
                           frames=[make_frame(301, 4096, 1000, 0.7)])
    # 40 % inliers.  Under the default epsilon = 0.5 no hypothesis can reach mRansacMinInliers = N / 2: no pose, whatever the draws
    S["share_04_default"] = dict(nf=1000, max_pairs=2, bad=[], seed=14, params=dict(DEFAULTS), degenerate=False,
                                 frames=[make_frame(401, 1000, 64, 0.4), make_frame(402, 1000, 257, 0.4)])
    # ... and under epsilon = 0.3 with 40 iterations an all-inlier sample (0.4^4 = 2.6 % each) comes for some seeds and not for others;
    # tests/test_pnp_cpu.py checks that both kinds are present
    p = dict(DEFAULTS, epsilon=0.3, max_iterations=40)
    S["share_04_eps03"] = dict(nf=1000, max_pairs=6, bad=[], seed=15, params=p, degenerate=False,
                               frames=[make_frame(410 + k, 1000, 65 if k % 2 else 257, 0.4, params=p) for k in range(6)])
    # termination and self-consistency only: a plane, points behind the camera, NaN world points, has_point past the record's count
    S["degenerate"] = dict(nf=1000, max_pairs=4, bad=[], seed=16, params=dict(DEFAULTS), degenerate=True,
                           frames=[make_frame(501, 1000, 64, 1.0, "planar"), make_frame(502, 1000, 65, 1.0, "behind"),
                                   make_frame(503, 1000, 64, 1.0, "nan"), make_frame(504, 1000, 1000, 0.7, "nan")])
    S["has_past_count"] = dict(nf=1000, max_pairs=1, bad=[], seed=17, params=dict(DEFAULTS), degenerate=False,
                               frames=[make_frame(601, 800, 64, 0.7, "tail")])
    return S


def refine_spread(fr, n_perm=8, seed=7):
    """the noise floor of one frame, on the reference side only: compute_pose on the planted inliers (what Refine solves once RANSAC has
    found them) under both back ends and n_perm random summation orders -> (base R, t, largest rotation / translation difference of the
    float poses to the base, borderline keypoints: those whose error2 comes within the spread of error2 over the runs, times 4, plus
    4 float ulps, of mvMaxError)"""
    import pose_opt_ref as PR
    idx, X, uv, s2 = correspondences(fr)
    keep = fr["planted"][idx]
    me = R.max_error(s2, DEFAULTS["th2"])
    rng = np.random.default_rng(seed)
    n = int(keep.sum())
    runs = []
    for backend in ("numpy", "jacobi"):
        runs.append(R.compute_pose(X[keep], uv[keep], CAM, backend))
        for _ in range(n_perm if backend == "numpy" else 1):
            runs.append(R.compute_pose(X[keep], uv[keep], CAM, backend, perm=rng.permutation(n)))
    base = runs[0]
    b12 = R.pose12(base[0], base[1])
    rot_s = max(PR.pose_difference(R.pose12(r[0], r[1]), b12)[0] for r in runs)
    tr_s = max(PR.pose_difference(R.pose12(r[0], r[1]), b12)[1] for r in runs)
    e2 = np.stack([R.check_inliers(r[0], r[1], X, uv, me, CAM)[1].astype(np.float64) for r in runs])
    margin = 4 * (e2.max(0) - e2.min(0)) + 4 * np.spacing(me).astype(np.float64)
    near = (np.abs(e2 - me.astype(np.float64)) <= margin).any(0) | ~np.isfinite(e2).all(0)
    return base, rot_s, tr_s, sorted(int(i) for i in idx[near])
