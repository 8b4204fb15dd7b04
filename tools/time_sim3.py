#!/usr/bin/env python3
"""Time per pair of ivf_tracker_solve_sim3 at 128 keyframe pairs of 1000 features with about 150 correspondences per pair (70 % obey the
planted similarity, the others are other points altogether; LoopClosing.cc:280's parameters 0.99 / 20 / 300, so mRansacMaxIts = 300 and all
300 hypotheses of a pair are computed, whichever iteration succeeds first), and of ivf_tracker_solve_pnp on the same batch in the same run
(the first keyframe of every pair against its own 150 points, 70 % inliers) as a yardstick.

  python tools/time_sim3.py [--pairs 128] [--features 1000] [--corr 150] [--reps 5] [--out profiles/sim3_latency.json]

Every call is timed with device events around one call after a warm-up; the median over `reps` calls is reported.  The file also records
the largest difference between the device and the restatement (tests/sim3_ref.py) over sim3 and hyp_sim3 on the scenes of
tests/sim3_scenes.py, next to the bound tests/test_gpu_sim3.py holds it to.  There is no bar on the times: they are recorded, not asserted."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32


def rot(rng, max_deg):
    a = rng.normal(size=3); a /= np.linalg.norm(a); th = math.radians(rng.uniform(0, max_deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def make_batch(rng, n_pairs, nf, n_corr, cam, share=0.7):
    """-> records (2 per pair), poses [2n,12], kf_xw [2n,nf,3], flags [2n,nf], match12 [n,nf], and for the PnP yardstick has [n,nf]"""
    from iv_slam_amd._lib import KP_DTYPE
    fx, fy, cx, cy, bf = cam
    W, H = 1241.0, 376.0
    recs = []; poses = np.zeros((2 * n_pairs, 12), F); xw = np.zeros((2 * n_pairs, nf, 3), F); flags = np.zeros((2 * n_pairs, nf), np.uint8)
    m12 = np.full((n_pairs, nf), -1, np.int32)
    for p in range(n_pairs):
        R12 = rot(rng, 15); t12 = rng.uniform(-0.5, 0.5, 3)
        u = rng.uniform(30, W - 30, nf); v = rng.uniform(30, H - 30, nf); z = rng.uniform(3, 40, nf)
        X1 = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        X2 = (X1 - t12) @ R12
        sel = np.sort(rng.permutation(nf)[:n_corr])
        out = rng.permutation(sel)[:n_corr - int(round(share * n_corr))]
        X2[out] += rng.uniform(2, 4, (len(out), 3)) * rng.choice([-1.0, 1.0], (len(out), 3))
        perm = rng.permutation(nf)
        for side, X in enumerate((X1, X2)):
            Rk = rot(rng, 25); tk = rng.uniform(-2, 2, 3)
            T = np.zeros((3, 4)); T[:, :3] = Rk; T[:, 3] = tk
            r = 2 * p + side
            poses[r] = T.reshape(12)
            slot = np.arange(nf) if side == 0 else perm
            xw[r, slot] = ((X - tk) @ Rk).astype(F)
            flags[r] = 1
            kp = np.zeros(nf, KP_DTYPE)
            uu = fx * X[:, 0] / X[:, 2] + cx + rng.uniform(-0.5, 0.5, nf); vv = fy * X[:, 1] / X[:, 2] + cy + rng.uniform(-0.5, 0.5, nf)
            if side == 0:                                                     # the yardstick's outliers: the keypoint is somewhere else
                ang = rng.uniform(0, 2 * math.pi, len(out)); mag = rng.uniform(30, 60, len(out))
                uu[out] += mag * np.cos(ang); vv[out] += mag * np.sin(ang)
            kp["x"][slot] = uu.astype(F); kp["y"][slot] = vv.astype(F); kp["octave"] = rng.integers(0, 8, nf); kp["size"] = 31
            recs.append(dict(kps=kp, desc=np.zeros((nf, 32), np.uint8), uright=np.full(nf, -1.0, F), depth=np.full(nf, -1.0, F)))
        m12[p, sel] = perm[sel]
    return recs, poses, xw, flags, m12


def device_vs_restatement():
    """the scenes of the suite through the suite's own runner: -> (largest difference seen, the bound)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import iv_slam_amd as iv
    import test_gpu_sim3 as T
    for names in T.groups():
        for i0 in range(0, len(names), 8):
            got = T.run_calls(iv, names[i0:i0 + 8])
            for name in names[i0:i0 + 8]:
                for k, (o, g) in enumerate(zip(T.ref_runs(name), got[name])):
                    T.compare(T.SCENES[name], k, o, g)
    return T.WORST[0], T.TOL


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=128); ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--corr", type=int, default=150); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib, dist as ivd, track
    dev = torch.device("cuda:0")
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    n, nf = a.pairs, a.features
    sc = iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors()
    tr = iv.BatchTracker(nf, sc, *cam, (0.0, 0.0, 1241.0, 376.0), max_pairs=n)
    recs, poses, xw, flags, m12 = make_batch(np.random.default_rng(1), n, nf, min(a.corr, nf), cam)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    block = up(ivd.pack_records(recs, nf).reshape(-1))
    pairs = up(np.stack([2 * np.arange(n), 2 * np.arange(n) + 1], 1).astype(np.int32))
    dposes, dxw, dflags, dm12 = up(poses), up(xw), up(flags), up(m12)
    draws3 = up(track.sim3_draws(n, 300, 1).view(np.int32)); draws4 = up(track.pnp_draws(n, 300, 1).view(np.int32))
    sim3 = torch.zeros((n, 16), dtype=torch.float32, device=dev); inl = torch.empty((n, nf), dtype=torch.uint8, device=dev)
    ninl = torch.empty(n, dtype=torch.int32, device=dev); its = torch.empty(n, dtype=torch.int32, device=dev)
    # the yardstick: solve_pnp of every first keyframe on the points of the same correspondences
    frames = pairs[:, 0].contiguous()
    pxw = dxw[0::2].contiguous(); phas = up((m12 >= 0).astype(np.uint8))
    ppose = torch.zeros((n, 12), dtype=torch.float32, device=dev); pinl = torch.empty((n, nf), dtype=torch.uint8, device=dev)
    pninl = torch.empty(n, dtype=torch.int32, device=dev); pits = torch.empty(n, dtype=torch.int32, device=dev)

    def call_sim3():
        tr.solve_sim3(block, pairs, dposes, dxw, dflags, dm12, draws3, sim3, inl, ninl, iterations=its)

    def call_pnp():
        tr.solve_pnp(block, frames, pxw, phas, draws4, ppose, pinl, pninl, iterations=pits)

    def timed(call):
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(np.min(ts))
    s_med, s_min = timed(call_sim3)
    p_med, p_min = timed(call_pnp)
    worst, bound = device_vs_restatement()
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), pairs=n, features=nf, correspondences=a.corr,
               max_iterations=300, reps=a.reps, solve_sim3_ms_median=s_med, solve_sim3_ms_min=s_min, solve_sim3_us_per_pair=s_med * 1e3 / n,
               pairs_with_transform=int((ninl > 0).sum().item()), inliers_per_pair_mean=float(ninl.float().mean().item()),
               iterations_per_pair_mean=float(its.float().mean().item()),
               solve_pnp_ms_median=p_med, solve_pnp_ms_min=p_min, solve_pnp_us_per_frame=p_med * 1e3 / n,
               pnp_frames_with_pose=int((pninl > 0).sum().item()), pnp_iterations_per_frame_mean=float(pits.float().mean().item()),
               worst_device_minus_restatement=worst, bound_8x_spread=bound)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
