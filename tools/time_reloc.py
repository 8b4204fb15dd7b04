#!/usr/bin/env python3
"""Time per pair of ivf_tracker_search_reloc, the batched Relocalization search SearchByProjection(F, KF, found, 10, 100), at 128 (keyframe, frame)
pairs of 1000 features, beside the per-call ivf_frame_search_by_projection_reloc looped over the same frames.

  python tools/time_reloc.py [--pairs 128] [--features 1000] [--reps 20] [--out profiles/reloc_latency.json]

Every frame's keypoints are uniform over a 1241 x 376 image; every keyframe keypoint holds the point of one frame keypoint, seen at the identity
pose 0..2 px beside it, with a descriptor 0..40 bits away; a third of the frame's keypoints hold their point on entry (occupied, and in the found
set).  The batched call (3 launches: k_reloc_prepare, k_reloc_window, k_reloc_greedy) is timed with device events around one call after a warm-up,
median over `reps`.  The per-call path is timed by the wall clock around the loop over the frames: the device-resident frames exist before the
clock starts and the queries (projection, PredictScale, radius: host work of the adapter) are prepared before it too, so the loop holds the query
upload, one window kernel, the download of the candidate lists and the host's greedy walk per frame.  There is no bar on these numbers: they are
recorded, not asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32


def make_pairs(rng, n, nf, cam, scale):
    from iv_slam_amd._lib import KP_DTYPE, LOCAL_POINT_DTYPE
    fx, fy, cx, cy, bf = cam
    recs, queries, assign = [], [], np.full((n, nf), -1, np.int32)
    pts = np.zeros((2 * n, nf), LOCAL_POINT_DTYPE); pts["flags"] = 1
    for k in range(n):
        kp = np.zeros(nf, KP_DTYPE)
        kp["x"] = rng.uniform(20, 1221, nf).astype(F); kp["y"] = rng.uniform(20, 356, nf).astype(F); kp["octave"] = rng.integers(0, 8, nf); kp["size"] = 31
        desc = rng.integers(0, 256, (nf, 32)).astype(np.uint8)
        perm = rng.permutation(nf)                                               # keyframe keypoint perm[i] holds the point of frame keypoint i
        u = kp["x"] + rng.uniform(-2, 2, nf); v = kp["y"] + rng.uniform(-2, 2, nf); z = rng.uniform(3, 40, nf)
        pos = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(F)
        dist = np.linalg.norm(pos.astype(np.float64), axis=1)
        flips = np.unpackbits(desc, axis=1)
        for i in range(nf):
            flips[i, rng.permutation(256)[:rng.integers(0, 41)]] ^= 1
        p = pts[2 * k]
        p["pos"][perm] = pos; p["max_distance"][perm] = (dist * 1.2 ** (kp["octave"] - 0.5)).astype(F); p["min_distance"][perm] = p["max_distance"][perm] / F(3.6)
        p["desc"][perm] = np.packbits(flips, axis=1); p["flags"] = 0
        held = rng.uniform(size=nf) < 1.0 / 3.0
        assign[k, held] = perm[held]
        kf = np.zeros(nf, KP_DTYPE); kf["size"] = 31
        recs += [dict(kps=kf, desc=np.zeros((nf, 32), np.uint8), uright=np.full(nf, -1.0, F), depth=np.full(nf, -1.0, F)),
                 dict(kps=kp, desc=desc, uright=np.full(nf, -1.0, F), depth=np.full(nf, -1.0, F))]
        # the same search as per-call queries, in keyframe keypoint order: the projections at the identity pose (recomputed in float)
        o = np.argsort(perm)
        pu = (F(fx) * pos[:, 0] * (F(1) / pos[:, 2]) + F(cx)).astype(F); pv = (F(fy) * pos[:, 1] * (F(1) / pos[:, 2]) + F(cy)).astype(F)
        queries.append(dict(u=pu[o], v=pv[o], radius=(F(10.0) * scale[kp["octave"]]).astype(F)[o], level=kp["octave"][o].astype(np.int32), angle=np.zeros(nf, F),
                            desc=p["desc"], valid=(~held[o]).astype(np.uint8)))
    return recs, pts, assign, queries


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=128); ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reloc_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib, dist as ivd
    dev = torch.device("cuda:0")
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    bounds = (0.0, 0.0, 1241.0, 376.0)
    n, nf = a.pairs, a.features
    scale = np.asarray(iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors(), F)
    recs, pts, assign0, queries = make_pairs(np.random.default_rng(1), n, nf, cam, scale)
    tr = iv.BatchTracker(nf, scale, *cam, bounds, max_pairs=n)
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    dp = torch.tensor([(2 * k, 2 * k + 1) for k in range(n)], dtype=torch.int32, device=dev)
    dpts = torch.from_numpy(pts.view(np.uint8).reshape(-1)).to(dev)
    a0 = torch.from_numpy(assign0).to(dev); assign = a0.clone(); nm = torch.empty(n, dtype=torch.int32, device=dev)

    def call():
        assign.copy_(a0)
        tr.search_reloc(block, dp, dpts, assign, nm, th=10.0, orb_dist=100)       # found = NULL: what the frame holds
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        assign.copy_(a0)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); tr.search_reloc(block, dp, dpts, assign, nm, th=10.0, orb_dist=100); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    batched = assign.cpu().numpy(); bnm = nm.cpu().numpy()

    frames = [iv.DeviceFrame(recs[2 * k + 1]["kps"], recs[2 * k + 1]["desc"], recs[2 * k + 1]["uright"], bounds) for k in range(n)]
    occ = [np.where(assign0[k] >= 0, -2, -1).astype(np.int32) for k in range(n)]
    per = []
    same = 0
    for rep in range(max(2, a.reps // 4) + 1):
        t0 = time.perf_counter()
        out = [frames[k].SearchByProjectionReloc(queries[k], 100, True, occ[k]) for k in range(n)]
        t1 = time.perf_counter()
        if rep:
            per.append((t1 - t0) * 1e3)
    for k in range(n):
        same += int(out[k][1] == bnm[k] and np.array_equal(out[k][0] >= 0, (batched[k] >= 0) & (assign0[k] < 0)))
    med = float(np.median(ts)); pmed = float(np.median(per))
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), pairs=n, features=nf, reps=a.reps,
               batched_launches=3, batched_ms_median=med, batched_ms_min=float(np.min(ts)), batched_us_per_pair=med * 1e3 / n,
               per_call_ms_median=pmed, per_call_us_per_pair=pmed * 1e3 / n, matches_per_pair_mean=float(bnm.mean()),
               pairs_where_both_paths_agree=same)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
