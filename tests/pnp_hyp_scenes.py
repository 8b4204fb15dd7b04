"""pnp_hyp_scenes.py -- the seeded scenes of the EPnP hypothesis tests (test infrastructure only), shared by tests/test_pnp_hyp_cpu.py (the
tail of tests/pnp_ref.py against itself: its spread, the power over its misreadings) and tests/test_gpu_pnp_hyp.py (the taps of
ivf_test_pnp_hypotheses against that tail), on the camera of tests/pose_opt_scenes.py.

Small on purpose: nfeatures 64 and the RANSAC parameters of tests/pnp_scenes.py:sampler_scene (epsilon 0.1, min_inliers 4,
max_iterations 64), under which N = 12 .. 40 correspondences give mRansacMaxIts = 64, N = 5 gives 7 and N = 4 gives 1.  Every iteration
of every frame is one 4-point hypothesis; the first rows of a frame's draws are planted with ransac_ref.draws_for where the frame is
about a kind of sample, the rest come from iv_slam_amd.track.ransac_draws.

scenarios() -> name -> dict(nf, max_pairs, bad, params, degenerate, frames, names, draws [n_frames, 64, 4]) in the layout of
tests/pnp_scenes.py:scenarios(), so that tests/test_gpu_pnp.py:run_pnp takes it.
  "hyp"         the comparable frames: clean / noise / outliers / near / turned / five / four, and one slot with a bad record index
  "degenerate"  termination and self-consistency only: four coplanar points, three collinear points plus one, a sample with a NaN point"""
import math

import numpy as np

import pnp_ref as R
import pnp_scenes as S
import pose_opt_scenes as PS

F = np.float32
CAM, SCALE, BOUNDS, KP_DTYPE, W, H = PS.CAM, PS.SCALE, PS.BOUNDS, PS.KP_DTYPE, PS.W, PS.H
NF = 64
PARAMS = dict(S.DEFAULTS, epsilon=0.1, min_inliers=4, max_iterations=64)


def make_frame(seed, nk, N, noise=0.0, share=1.0, depth=(3.0, 40.0), angle=None):
    """nk keypoints, the first N of a seeded choice hold a map point.  noise: uniform +- that many px per axis on every observation;
    share: the planted inlier share, the others are moved by 30 .. 60 px; depth: the range of camera-frame depths in metres; angle: the
    rotation of the pose in degrees (None: uniform 0 .. 25)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (np.float64(CAM[k]) for k in ("fx", "fy", "cx", "cy"))
    Rg = PS.rot(rng.normal(size=3), rng.uniform(0, 25) if angle is None else angle); tg = rng.uniform(-2, 2, 3)
    u = rng.uniform(20, W - 20, nk); v = rng.uniform(20, H - 20, nk); z = rng.uniform(depth[0], depth[1], nk)
    Pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    Xw = ((Pc - tg) @ Rg).astype(F)
    Pc = Xw.astype(np.float64) @ Rg.T + tg
    u = fx * Pc[:, 0] / Pc[:, 2] + cx; v = fy * Pc[:, 1] / Pc[:, 2] + cy
    u = u + rng.uniform(-1, 1, nk) * noise; v = v + rng.uniform(-1, 1, nk) * noise
    has = np.zeros(nk, np.uint8)
    pts = np.sort(rng.permutation(nk)[:N])
    has[pts] = 1
    out = rng.permutation(pts)[:N - int(round(share * N))]
    ang = rng.uniform(0, 2 * math.pi, len(out)); mag = rng.uniform(30, 60, len(out))
    u[out] += mag * np.cos(ang); v[out] += mag * np.sin(ang)
    planted = has.astype(bool); planted[out] = False
    kp = np.zeros(nk, KP_DTYPE)
    kp["x"] = u.astype(F); kp["y"] = v.astype(F); kp["octave"] = rng.integers(0, 8, nk); kp["size"] = 31
    Tgt = np.zeros((3, 4)); Tgt[:, :3] = Rg; Tgt[:, 3] = tg
    n_min, its, _ = R.ransac_parameters(N, PARAMS["probability"], PARAMS["min_inliers"], PARAMS["max_iterations"], PARAMS["epsilon"])
    return dict(kps=kp, n=nk, uright=np.full(nk, -1.0, F), depth=np.full(nk, -1.0, F), desc=np.zeros((nk, 32), np.uint8), xw=Xw, has=has,
                planted=planted, pose_gt=Tgt.reshape(12), N=N, share=share, kind=None, seed=seed, n_min=n_min, max_its=its)


def _draws(seed, frames, planted):
    """ransac_draws for every frame, the first rows of frame k replaced by draws_for(planted[k][j])"""
    from iv_slam_amd import track
    d = track.ransac_draws(len(frames), PARAMS["max_iterations"], 4, seed)
    for k, rows in planted.items():
        for j, wanted in enumerate(rows):
            d[k, j] = R.draws_for(frames[k]["N"], wanted)
    return d


def mixed_samples(fr):
    """for the outlier frame: samples (as indices into the frame's correspondences) of 4, 3, 2, 1 and 0 planted inliers"""
    idx = np.nonzero(fr["has"])[0]
    good = [j for j, i in enumerate(idx) if fr["planted"][i]]; bad = [j for j, i in enumerate(idx) if not fr["planted"][i]]
    return [good[:4 - k] + bad[:k] for k in range(5)] + [bad[2:4] + good[5:7]]


def scenarios():
    out = {}
    frames = [make_frame(901, 64, 12),                                    # clean: the planted pose is reachable
              make_frame(902, 50, 20, noise=0.5),
              make_frame(903, 64, 40, noise=0.5, share=0.7),              # samples mix inliers and outliers
              make_frame(904, 40, 16, noise=0.5, depth=(0.5, 2.0)),       # near only
              make_frame(905, 33, 13, noise=0.5, angle=120.0),            # a large rotation
              make_frame(906, 64, 12),                                    # the slot that gets a bad record index
              make_frame(907, 64, 5, noise=0.5),                          # mRansacMaxIts = 7 < max_iterations
              make_frame(908, 9, 4, noise=0.5)]                           # mRansacMinInliers == N: one iteration
    names = ["clean", "noise", "outliers", "near", "turned", "bad_record", "five", "four"]
    assert [f["max_its"] for f in frames] == [64, 64, 64, 64, 64, 64, 7, 1]
    out["hyp"] = dict(nf=NF, max_pairs=len(frames), bad=[5], seed=31, params=dict(PARAMS), degenerate=False, frames=frames, names=names,
                      draws=_draws(31, frames, {2: mixed_samples(frames[2])}))
    # ---- termination and self-consistency only
    base = make_frame(911, 64, 12)
    idx = np.nonzero(base["has"])[0]
    fx, fy, cx, cy = (np.float64(CAM[k]) for k in ("fx", "fy", "cx", "cy"))
    T = base["pose_gt"].reshape(3, 4); Rg, tg = T[:, :3], T[:, 3]

    def with_camera_points(sel, Pc):
        """the frame whose correspondences sel sit at the camera-frame points Pc and are observed exactly"""
        fr = dict(base, xw=base["xw"].copy(), kps=base["kps"].copy())
        fr["xw"][idx[sel]] = ((Pc - tg) @ Rg).astype(F)
        Pq = fr["xw"][idx[sel]].astype(np.float64) @ Rg.T + tg
        fr["kps"]["x"][idx[sel]] = (fx * Pq[:, 0] / Pq[:, 2] + cx).astype(F); fr["kps"]["y"][idx[sel]] = (fy * Pq[:, 1] / Pq[:, 2] + cy).astype(F)
        return fr
    sel = [0, 1, 2, 3]
    plane = np.array([[-2.0, -1.0, 10.0], [2.0, -1.0, 10.5], [2.0, 1.0, 11.0], [-2.0, 1.0, 10.5]])       # z = 10.25 + x / 8 + y / 4 ... a plane
    plane[:, 2] = 10.0 + 0.125 * plane[:, 0] + 0.25 * plane[:, 1]
    line = np.array([[-1.0, -0.5, 8.0], [0.0, 0.0, 9.0], [1.0, 0.5, 10.0], [0.5, -1.0, 12.0]])           # the first three on one line
    nan = dict(base, xw=base["xw"].copy())
    nan["xw"][idx[2], 1] = np.nan
    dframes = [with_camera_points(sel, plane), with_camera_points(sel, line), nan]
    planted = {0: [[0, 1, 2, 3], [3, 1, 0, 2]], 1: [[0, 1, 2, 3], [3, 2, 1, 0]], 2: [[2, 5, 7, 9], [0, 1, 2, 3], [4, 6, 8, 2]]}
    out["degenerate"] = dict(nf=NF, max_pairs=3, bad=[], seed=32, params=dict(PARAMS), degenerate=True, frames=dframes,
                             names=["coplanar", "collinear", "nan_point"], draws=_draws(32, dframes, planted), planted=planted)
    return out


def samples(sc):
    """every (frame slot, iteration, sample) of a scenario that the device runs: iterations below mRansacMaxIts of the frames whose record
    index is good"""
    for k, fr in enumerate(sc["frames"]):
        if k in sc["bad"]:
            continue
        for it in range(fr["max_its"]):
            yield k, it, R.sample_indices(fr["N"], sc["draws"][k, it])


# ---- how two results of pnp_ref.pose_tail are compared ------------------------------------------------------------------------------------
QUANTITIES = ("betas0", "betas1", "R", "t", "err")


def tail_difference(a, b, uv):
    """-> [3, 5]: per candidate and quantity of QUANTITIES the largest difference of b to a relative to the quantity's own size in a (its
    largest magnitude: the betas as a 4-vector, R as a matrix, t as a 3-vector; err relative to the larger of err and the largest image
    coordinate in uv, the sample's observations: err is a mean of distances between image coordinates and rounds as they do).  inf where
    one side is not finite and the other is or the non-finite patterns differ, 0 where both hold the same values, finite or not."""
    out = np.zeros((3, len(QUANTITIES)))
    pixel = float(np.abs(np.asarray(uv, np.float64)).max())
    with np.errstate(all="ignore"):
        for q, name in enumerate(QUANTITIES):
            for c in range(3):
                x = np.asarray(a[name][c], np.float64).reshape(-1); y = np.asarray(b[name][c], np.float64).reshape(-1)
                if not (np.isfinite(x).all() and np.isfinite(y).all()):
                    out[c, q] = 0.0 if np.array_equal(x, y, equal_nan=True) else np.inf
                    continue
                scale = max(np.abs(x).max(), pixel) if name == "err" else np.abs(x).max()
                d = np.abs(x - y).max()
                out[c, q] = 0.0 if d == 0 else (d / scale if scale > 0 else np.inf)
    return out


def perturbed(vv, seed):
    """the basis moved by one ulp per entry, up or down by a seeded coin"""
    rng = np.random.default_rng(seed)
    vv = np.asarray(vv, np.float64)
    return vv + np.spacing(np.abs(vv)) * rng.choice([-1.0, 1.0], vv.shape)
