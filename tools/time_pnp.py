#!/usr/bin/env python3
"""Time per frame of ivf_tracker_solve_pnp at 128 frames of 1000 features for 20 / 100 / 1000 correspondences per frame (70 % inliers with
0.5 px of noise, the outliers moved by 30..60 px; max_iterations = 300 and Tracking.cc:2317's other parameters, so mRansacMaxIts = 35).

  python tools/time_pnp.py [--frames 128] [--features 1000] [--reps 20] [--out profiles/pnp_latency.json]

Every call is timed with device events around one call after a warm-up; the median over `reps` calls is reported, with the mean number of
RANSAC iterations a frame ran before Refine succeeded.  There is no bar on these numbers: they are recorded, not asserted."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32


def make_frames(rng, n_frames, nf, n_corr, cam, share=0.7):
    from iv_slam_amd._lib import KP_DTYPE
    fx, fy, cx, cy, bf = cam
    W, H = 1241.0, 376.0
    recs = []; xw = np.zeros((n_frames, nf, 3), F); has = np.zeros((n_frames, nf), np.uint8)
    for k in range(n_frames):
        u = rng.uniform(30, W - 30, nf); v = rng.uniform(30, H - 30, nf); z = rng.uniform(3, 40, nf)
        Pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        a = rng.normal(size=3); a /= np.linalg.norm(a); th = math.radians(rng.uniform(0, 20))
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        Rg = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K); tg = rng.uniform(-2, 2, 3)
        xw[k] = ((Pc - tg) @ Rg).astype(F)
        pts = rng.permutation(nf)[:n_corr]
        has[k, pts] = 1
        u = u + rng.uniform(-0.5, 0.5, nf); v = v + rng.uniform(-0.5, 0.5, nf)
        out = pts[:n_corr - int(round(share * n_corr))]
        ang = rng.uniform(0, 2 * math.pi, len(out)); mag = rng.uniform(30, 60, len(out))
        u[out] += mag * np.cos(ang); v[out] += mag * np.sin(ang)
        kp = np.zeros(nf, KP_DTYPE)
        kp["x"] = u.astype(F); kp["y"] = v.astype(F); kp["octave"] = rng.integers(0, 8, nf); kp["size"] = 31
        recs.append(dict(kps=kp, desc=np.zeros((nf, 32), np.uint8), uright=np.full(nf, -1.0, F), depth=np.full(nf, -1.0, F)))
    return recs, xw, has


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=128); ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pnp_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib, dist as ivd, track
    dev = torch.device("cuda:0")
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    n, nf = a.frames, a.features
    sc = iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors()
    tr = iv.BatchTracker(nf, sc, *cam, (0.0, 0.0, 1241.0, 376.0), max_pairs=n)
    frames = torch.arange(n, dtype=torch.int32, device=dev)
    draws = torch.from_numpy(track.pnp_draws(n, 300, 1).view(np.int32)).to(dev)
    poses = torch.zeros((n, 12), dtype=torch.float32, device=dev); inl = torch.empty((n, nf), dtype=torch.uint8, device=dev)
    ninl = torch.empty(n, dtype=torch.int32, device=dev); its = torch.empty(n, dtype=torch.int32, device=dev)
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), frames=n, features=nf, reps=a.reps, cases=[])
    for n_corr in (20, 100, 1000):
        recs, xw, has = make_frames(np.random.default_rng(n_corr), n, nf, min(n_corr, nf), cam)
        block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
        dxw = torch.from_numpy(xw).to(dev); dhas = torch.from_numpy(has).to(dev)

        def call():
            tr.solve_pnp(block, frames, dxw, dhas, draws, poses, inl, ninl, iterations=its)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        med = float(np.median(ts))
        res["cases"].append(dict(correspondences=n_corr, solve_pnp_ms_median=med, solve_pnp_ms_min=float(np.min(ts)), solve_pnp_us_per_frame=med * 1e3 / n,
                                 frames_with_pose=int((ninl > 0).sum().item()), inliers_per_frame_mean=float(ninl.float().mean().item()),
                                 iterations_per_frame_mean=float(its.float().mean().item())))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
