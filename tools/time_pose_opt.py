#!/usr/bin/env python3
"""Time per frame of ivf_tracker_optimize_pose next to ivf_tracker_run on the same batch: 128 frame pairs, 1000 features, about 300
edges per frame (300 of the 1000 keypoints are stereo points; the next frame is the same scene moved by a small camera motion).

  python tools/time_pose_opt.py [--frames 128] [--features 1000] [--stereo 300] [--reps 30] [--out profiles/pose_opt_latency.json]

Both calls are timed with device events around `reps` back-to-back calls after a warm-up; the median is reported.  The chain is
run -> points_from_pairs -> optimize_pose on device buffers, with the identity as every pose (zero-motion prior)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32


def make_records(rng, n_frames, nf, n_stereo, cam):
    from iv_slam_amd._lib import KP_DTYPE
    fx, fy, cx, cy, bf = cam
    W, H = 1241.0, 376.0
    u = rng.uniform(30, W - 30, nf); v = rng.uniform(30, H - 30, nf); z = rng.uniform(5, 40, nf)
    P = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    desc = rng.integers(0, 256, (nf, 32)).astype(np.uint8)
    octv = rng.integers(0, 4, nf)
    stereo = np.zeros(nf, bool); stereo[rng.permutation(nf)[:n_stereo]] = True
    recs = []
    for k in range(n_frames + 1):
        t = np.array([0.004 * k, 0.0, -0.03 * k])                            # a slow forward motion: a few pixels per frame
        Pc = P + t
        kp = np.zeros(nf, KP_DTYPE)
        kp["x"] = (fx * Pc[:, 0] / Pc[:, 2] + cx + rng.normal(0, 0.3, nf)).astype(F); kp["y"] = (fy * Pc[:, 1] / Pc[:, 2] + cy + rng.normal(0, 0.3, nf)).astype(F)
        kp["octave"] = octv; kp["size"] = 31; kp["angle"] = 10
        ur = np.where(stereo, kp["x"] - bf / Pc[:, 2], -1).astype(F)
        recs.append(dict(kps=kp, desc=desc, uright=ur, depth=np.where(stereo, Pc[:, 2], -1).astype(F)))
    return recs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=128); ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--stereo", type=int, default=300); ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pose_opt_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib, dist as ivd
    dev = torch.device("cuda:0")
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    n, nf = a.frames, a.features
    recs = make_records(np.random.default_rng(1), n, nf, a.stereo, cam)
    sc = iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors()
    tr = iv.BatchTracker(nf, sc, *cam, (0.0, 0.0, 1241.0, 376.0), max_pairs=n)
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    pairs = torch.tensor([(k, k + 1) for k in range(n)], dtype=torch.int32, device=dev)
    cur = pairs[:, 1].contiguous()
    assign = torch.empty((n, nf), dtype=torch.int32, device=dev); nm = torch.empty(n, dtype=torch.int32, device=dev)
    xw = torch.empty((n, nf, 3), dtype=torch.float32, device=dev); has = torch.empty((n, nf), dtype=torch.uint8, device=dev)
    eye = torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=torch.float32, device=dev).repeat(n, 1).contiguous()
    poses = eye.clone()
    outl = torch.empty((n, nf), dtype=torch.uint8, device=dev); ninl = torch.empty(n, dtype=torch.int32, device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(np.min(ts))

    t_run = timed(lambda: tr.run(block, pairs, assign, nm))
    tr.points_from_pairs(block, pairs, assign, xw, has)
    t_pts = timed(lambda: tr.points_from_pairs(block, pairs, assign, xw, has))

    def opt():
        poses.copy_(eye)
        tr.optimize_pose(block, cur, xw, has, poses, outl, ninl)
    t_copy = timed(lambda: poses.copy_(eye))
    t_opt = timed(opt)
    torch.cuda.synchronize()
    edges = has.sum(1).cpu().numpy(); inl = ninl.cpu().numpy()
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), frames=n, features=nf,
               edges_per_frame_mean=float(edges.mean()), inliers_per_frame_mean=float(inl.mean()), matches_per_frame_mean=float(nm.cpu().numpy().mean()),
               reps=a.reps, tracker_run_ms_median=t_run[0], tracker_run_ms_min=t_run[1], points_from_pairs_ms_median=t_pts[0],
               optimize_pose_ms_median=t_opt[0] - t_copy[0], optimize_pose_ms_min=t_opt[1] - t_copy[1], pose_reset_copy_ms_median=t_copy[0],
               optimize_pose_us_per_frame=(t_opt[0] - t_copy[0]) * 1e3 / n, tracker_run_us_per_frame=t_run[0] * 1e3 / n)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
