"""pose_opt_scenes.py -- the synthetic scenarios of the PoseOptimization tests (test infrastructure only), shared by
tests/test_pose_opt_cpu.py (the restatement against ground truth, the noise floor in tests/golden/pose_opt_noise.json) and
tests/test_gpu_pose_opt.py (ivf_tracker_optimize_pose against the restatement).  Everything is drawn from fixed seeds.

A frame: a KITTI-like camera at a ground-truth pose, map points spread over the image at 4..40 m, observations = the projection of the
FLOAT world point through the ground-truth pose (plus noise / planted gross outliers), narrowed to float like mvKeysUn / mvuRight."""
import math

import numpy as np

import pose_opt_ref as PR

F = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])   # ivf_keypoint
W, H = 1241.0, 376.0
CAM = dict(fx=F(718.856), fy=F(718.856), cx=F(607.1928), cy=F(185.2157), bf=F(386.1448))
BOUNDS = (0.0, 0.0, W, H)


def scale_table(nlevels=8, sf=1.2):
    s = [F(1.0)]
    for _ in range(1, nlevels):
        s.append(F(np.float64(s[-1]) * np.float64(F(sf))))
    return np.array(s, F)


SCALE = scale_table()
INV_SIGMA2 = PR.inv_level_sigma2(SCALE)


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def make_frame(seed, nk, n_edges, kind="mixed", noise=0.0, n_outliers=0, prior=(0.02, 0.3), quality=None, biased=0, rot_gt=None, behind=0):
    """nk keypoints, n_edges of them hold a map point.  kind: mono / stereo / mixed; noise: sigma in px at level 0 (times the level's
    scale factor); n_outliers: edges whose observation is moved 25..60 px; prior = (metres, degrees) the input pose is off the truth;
    quality: None, "ones", "random" (uniform [0.2, 1]), "zero" (0 on a fifth of the edges, 1 elsewhere); biased: that many edges get
    +2.5 px in x and quality 0.2 when quality == "biased"; quality == "negative": -1 on three quarters of the edges, 1 elsewhere;
    "all_zero": 0 everywhere.
    rot_gt: the ground-truth rotation, a 3x3 matrix or (axis, degrees), in place of the drawn 0..8 degrees; prior == (0, 0): the input
    pose is the truth narrowed to float; behind: that many edges get their world point mirrored through the camera's principal plane
    at the true pose (z -> -z in the camera frame) and are marked planted.  Both consume no draw that an older argument list made."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = (np.float64(CAM[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    Rg = rot(rng.normal(size=3), rng.uniform(0, 8)); tg = rng.uniform(-2, 2, 3)
    if rot_gt is not None:
        Rg = rot(*rot_gt) if len(rot_gt) == 2 else np.array(rot_gt, np.float64).reshape(3, 3)
    kp = np.zeros(nk, KP_DTYPE)
    u = rng.uniform(20, W - 20, nk); v = rng.uniform(20, H - 20, nk); z = rng.uniform(4, 40, nk)
    octv = rng.integers(0, 8, nk)
    Pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    Xw = ((Pc - tg) @ Rg).astype(F)                                            # R^T (Pc - t), narrowed: GetWorldPos() is float
    Pc = Xw.astype(np.float64) @ Rg.T + tg
    u = fx * Pc[:, 0] / Pc[:, 2] + cx; v = fy * Pc[:, 1] / Pc[:, 2] + cy
    ur = u - bf / Pc[:, 2]
    stereo = {"mono": np.zeros(nk, bool), "stereo": np.ones(nk, bool), "mixed": rng.uniform(size=nk) < 0.6}[kind]
    sig = noise * SCALE[octv].astype(np.float64)
    u = u + rng.normal(size=nk) * sig; v = v + rng.normal(size=nk) * sig; ur = ur + rng.normal(size=nk) * sig
    has = np.zeros(nk, np.uint8)
    edges = np.sort(rng.permutation(nk)[:n_edges])
    has[edges] = 1
    planted = np.zeros(nk, np.uint8)
    out = rng.permutation(edges)[:n_outliers]
    ang = rng.uniform(0, 2 * math.pi, len(out)); mag = rng.uniform(25, 60, len(out))
    u[out] += mag * np.cos(ang); v[out] += mag * np.sin(ang); ur[out] += mag * np.cos(ang) + rng.uniform(-20, 20, len(out))
    planted[out] = 1
    q = None
    if quality == "ones":
        q = np.ones(nk, F)
    elif quality == "random":
        q = rng.uniform(0.2, 1.0, nk).astype(F)
    elif quality == "zero":
        q = np.ones(nk, F); q[rng.permutation(edges)[:max(1, n_edges // 5)]] = 0
    elif quality == "all_zero":
        q = np.zeros(nk, F)
    elif quality == "negative":
        q = np.ones(nk, F); q[rng.permutation(edges)[:(3 * n_edges) // 4]] = -1
    if biased:
        sel = rng.permutation(edges)[:biased]
        u[sel] += 2.5; ur[sel] += 2.5
        if quality == "biased":
            q = np.ones(nk, F); q[sel] = F(0.2)
    kp["x"] = u.astype(F); kp["y"] = v.astype(F); kp["octave"] = octv; kp["size"] = 31
    uright = np.where(stereo, ur, -1.0).astype(F)
    depth = np.where(stereo, Pc[:, 2], -1.0).astype(F)
    # the input pose: the truth moved by `prior`
    dR = rot(rng.normal(size=3), prior[1]); dt = rng.normal(size=3); dt = dt / np.linalg.norm(dt) * prior[0]
    Tin = np.zeros((3, 4)); Tin[:, :3] = dR @ Rg; Tin[:, 3] = dR @ tg + dt
    if tuple(prior) == (0, 0):
        Tin[:, :3] = Rg; Tin[:, 3] = tg                                          # not dR @ Rg with dR = I + 0 * K: the exact matrix
    if behind:
        sel = rng.permutation(edges)[:behind]
        Pm = Xw[sel].astype(np.float64) @ Rg.T + tg; Pm[:, 2] = -Pm[:, 2]
        Xw[sel] = ((Pm - tg) @ Rg).astype(F)
        planted[sel] = 1
    Tgt = np.zeros((3, 4)); Tgt[:, :3] = Rg; Tgt[:, 3] = tg
    return dict(kps=kp, n=nk, uright=uright, depth=depth, desc=np.zeros((nk, 32), np.uint8), xw=Xw, has=has, quality=q,
                pose_in=Tin.astype(F).reshape(12), pose_gt=Tgt.reshape(12), planted=planted, noise_free=noise == 0.0 and not biased)


def reference(fr, n_rounds, perm=None):
    return PR.pose_optimization(fr["kps"], fr["n"], fr["uright"], INV_SIGMA2, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["bf"], fr["xw"],
                                fr["has"], fr["quality"], n_rounds, fr["pose_in"], perm=perm)


def scenarios():
    """name -> dict(nf, n_rounds, frames, max_pairs, bad = frame slots that get a record index outside the block)"""
    S = {}
    # edge counts around the early returns, the < 10 break and one wave; noise-free with planted outliers; one bad record index;
    # n_frames == max_pairs with a different edge count per frame
    counts = [0, 2, 3, 9, 10, 63, 64]
    S["counts64_clean"] = dict(nf=64, n_rounds=4, max_pairs=8, bad=[3],
                               frames=[make_frame(100 + k, 64, c, "mixed", 0.0, n_outliers=(c // 6 if c >= 10 else 0)) for k, c in enumerate(counts[:3])] +
                                      [make_frame(199, 64, 40, "mixed", 0.0, 5)] +
                                      [make_frame(100 + k, 64, c, "mixed", 0.0, n_outliers=(c // 6 if c >= 10 else 0)) for k, c in enumerate(counts) if k >= 3])
    # a wave plus one edge, more than one edge per lane; pixel noise, the prior 0.2 m / 3 degrees off
    S["over_a_wave_noisy"] = dict(nf=320, n_rounds=4, max_pairs=4, bad=[],
                                  frames=[make_frame(201, 320, 65, "mixed", 1.0, 6, prior=(0.2, 3.0)), make_frame(202, 300, 257, "mixed", 1.0, 25, prior=(0.2, 3.0)),
                                          make_frame(203, 320, 257, "stereo", 0.0, 30, prior=(0.2, 3.0))])
    # a sparse has_point over the largest record; quality drawn from [0.2, 1]
    S["sparse4096"] = dict(nf=4096, n_rounds=4, max_pairs=1, bad=[],
                           frames=[make_frame(301, 4096, 1000, "mixed", 1.0, 80, prior=(0.2, 3.0), quality="random")])
    # all-mono, all-stereo and mixed frames under every round count
    for r in (1, 2, 3, 4):
        S["kinds_rounds%d" % r] = dict(nf=64, n_rounds=r, max_pairs=3, bad=[],
                                       frames=[make_frame(400 + 10 * r + k, 64, 64, kind, 1.0, 6, prior=(0.2, 3.0)) for k, kind in enumerate(("mono", "stereo", "mixed"))])
    # the quality score: absent, 1 (the same thing), random, 0 on a subset
    for qn in (None, "ones", "random", "zero"):
        S["quality_%s" % qn] = dict(nf=64, n_rounds=4, max_pairs=1, bad=[], frames=[make_frame(500, 64, 60, "mixed", 1.0, 6, prior=(0.1, 1.5), quality=qn)])
    # ---- rotations far from the identity: Quaterniond(Matrix3d) leaves its trace > 0 branch at 120 degrees, normalizeRotation flips the sign
    turns = [((1, 0, 0), 179.0), ((0, 1, 0), 179.0), ((0, 0, 1), 179.0), ((0, 1, 0), -178.0), ((1, 0, 0), -179.5), ((0, 0, 1), -177.0),
             ((1, 2, 3), 170.0), ((3, -1, 2), -175.0)]
    for label, noise in (("clean", 0.0), ("noisy", 1.0)):
        S["half_turn_%s" % label] = dict(nf=80, n_rounds=4, max_pairs=len(turns), bad=[],
                                         frames=[make_frame(800 + (10 if noise else 0) + k, 80, 60, "mixed", noise, 8, prior=(0.2, 3.0), rot_gt=t) for k, t in enumerate(turns)])
    # both sides of trace == 0, the input pose 3 degrees off
    S["branch_boundary"] = dict(nf=72, n_rounds=4, max_pairs=3, bad=[],
                                frames=[make_frame(830 + k, 72, 60, "mixed", 1.0, 6, prior=(0.2, 3.0), rot_gt=((0, 1, 0), d)) for k, d in enumerate((119.0, 120.0, 121.0))])
    # the input pose is an exact float matrix: trace exactly 0 and exactly -1, ties on the diagonal, w == 0 before the sign test
    cyc = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
    exact = [cyc, [list(r) for r in zip(*cyc)], [[0, -1, 0], [0, 0, -1], [1, 0, 0]], [[1, 0, 0], [0, -1, 0], [0, 0, -1]], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]],
             [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]]
    S["exact_axis_poses"] = dict(nf=64, n_rounds=4, max_pairs=2 * len(exact), bad=[],
                                 frames=[make_frame(840 + 2 * k + j, 64, 48, kind, 1.0, 5, prior=(0, 0), rot_gt=m) for k, m in enumerate(exact) for j, kind in enumerate(("mono", "stereo"))])
    # the conversions alone.  Quality 0 on every edge and one round (the kernels are never dropped): every weight is 0, H = b = 0, the
    # step is 0, rho == 0 terminates, and the pose that leaves is toRotationMatrix(normalizeRotation(Quaterniond(input))), with no sum
    # over edges in it: compared to the bit.  An optimiser that converges hides a wrong quaternion of the input pose behind the same
    # optimum (a flipped w at 179 degrees is a start 2 degrees off); here nothing moves.  Rotations about one axis at 130 / -135 degrees
    # (|w| ~ 0.4), and for each of i = 0, 1, 2 a generic axis with that component largest and the other two well away from 0
    conv = [((1, 0, 0), 130.0), ((0, 1, 0), 130.0), ((0, 0, 1), 130.0), ((1, 0, 0), -135.0), ((0, 1, 0), -135.0), ((0, 0, 1), -135.0),
            ((3, 2, 1), 150.0), ((1, 3, 2), -150.0), ((2, 1, 3), 145.0), ((3, -1, 2), -140.0), ((-2, 3, 1), 160.0), ((1, -2, 3), -155.0),
            ((0, 1, 0), 90.0), ((1, 1, 1), -100.0)]
    S["conversion_only"] = dict(nf=64, n_rounds=1, max_pairs=len(conv), bad=[],
                                frames=[make_frame(850 + k, 64, 48, "mixed", 1.0, 5, quality="all_zero", rot_gt=t) for k, t in enumerate(conv)])
    # six world points mirrored through the camera's principal plane: z < 0 in the camera frame, negative invz
    S["behind_camera"] = dict(nf=96, n_rounds=4, max_pairs=1, bad=[], frames=[make_frame(870, 96, 80, "mixed", 0.0, 0, behind=6)])
    # negative Huber widths make H + lambda I non-positive: failed solves, ten trials exhausted, the pose stays
    S["negative_quality"] = dict(nf=64, n_rounds=4, max_pairs=1, bad=[], frames=[make_frame(880, 64, 40, "mixed", 1.0, 4, prior=(0.1, 1.5), quality="negative")])
    # a record of 50 keypoints in 64 slots, has_point = 1 (and a point) on the 14 slots past the record's count
    S["has_past_count"] = dict(nf=64, n_rounds=4, max_pairs=1, bad=[], frames=[dict(make_frame(890, 50, 44, "mixed", 1.0, 4, prior=(0.2, 3.0)), has_tail=1)])
    return S


def spread_and_borderline(fr, n_rounds, n_perm=8, seed=7):
    """the restatement of one frame under the identity and n_perm random edge orders -> (base result, largest rotation / translation
    difference of the float poses to the base, keypoint indices of the borderline edges).  An edge is borderline when, in any round of
    any run, its chi2 lies within 4 x (its own spread over the runs) + 4 float ulps of the threshold it is compared with."""
    base = reference(fr, n_rounds)
    ne = len(base["edges"])
    rng = np.random.default_rng(seed)
    runs = [base] + [reference(fr, n_rounds, perm=rng.permutation(ne)) for _ in range(n_perm)] if ne >= 3 else [base]
    rot_s = max(PR.pose_difference(r["pose"], base["pose"])[0] for r in runs)
    tr_s = max(PR.pose_difference(r["pose"], base["pose"])[1] for r in runs)
    border = set()
    if ne >= 3:
        thr = base["thr"].astype(np.float64)
        rounds = min(len(r["chi2_rounds"]) for r in runs)
        if any(len(r["chi2_rounds"]) != rounds for r in runs):
            border |= set(int(i) for i in base["edges"])                         # the runs did not even agree on the number of rounds
        for k in range(rounds):
            chi = np.stack([r["chi2_rounds"][k] for r in runs])
            with np.errstate(all="ignore"):
                margin = 4 * (chi.max(0) - chi.min(0)) + 4 * np.spacing(base["thr"]).astype(np.float64)
                near = (np.abs(chi - thr) <= margin).any(0) | ~np.isfinite(chi).all(0)
            border |= set(int(i) for i in base["edges"][near])
        for r in runs:
            border |= set(int(i) for i in np.nonzero(r["outlier"] != base["outlier"])[0])
    return base, rot_s, tr_s, sorted(border)
