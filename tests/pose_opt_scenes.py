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


def make_frame(seed, nk, n_edges, kind="mixed", noise=0.0, n_outliers=0, prior=(0.02, 0.3), quality=None, biased=0):
    """nk keypoints, n_edges of them hold a map point.  kind: mono / stereo / mixed; noise: sigma in px at level 0 (times the level's
    scale factor); n_outliers: edges whose observation is moved 25..60 px; prior = (metres, degrees) the input pose is off the truth;
    quality: None, "ones", "random" (uniform [0.2, 1]), "zero" (0 on a fifth of the edges, 1 elsewhere); biased: that many edges get
    +2.5 px in x and quality 0.2 when quality == "biased"."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = (np.float64(CAM[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    Rg = rot(rng.normal(size=3), rng.uniform(0, 8)); tg = rng.uniform(-2, 2, 3)
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
