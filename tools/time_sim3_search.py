#!/usr/bin/env python3
"""Time per pair of the two batched loop-closing searches, ivf_tracker_search_by_bow_keyframes and ivf_tracker_search_by_sim3, at 128
keyframe pairs of 1000 features: every keypoint of KF1 holds a point that KF2 sees too under a planted similarity (s = 1.2); the BoW search
runs on a synthetic vocabulary of depth 3 and branching 10, SearchBySim3 with no match given, so both directions project and search all
1000 points.

  python tools/time_sim3_search.py [--pairs 128] [--features 1000] [--reps 20] [--out profiles/sim3_search_latency.json]

Every call is timed with device events around one call after a warm-up; the median over `reps` calls is reported.  Beside it, for scale,
the per-call path on the same machine for ONE of those pairs by the wall clock: ivf_search_by_sim3 from host arrays with the projections
precomputed (upload, two window kernels, download, the agreement check on the host), and ivf_search_by_bow_keyframes with the feature
vectors precomputed.  There is no bar on these numbers: they are recorded, not asserted."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32
W, H = 1241.0, 376.0


def make_vocabulary(rng, depth=3, k=10):
    """flat arrays of a random tree: every inner node has k children with random descriptors, every leaf a word of positive weight"""
    children = [[]]; level = [0]; frontier = [0]
    for lv in range(1, depth + 1):
        nxt = []
        for node in frontier:
            for _ in range(k):
                children.append([]); level.append(lv); children[node].append(len(children) - 1); nxt.append(len(children) - 1)
        frontier = nxt
    n = len(children)
    start = np.zeros(n + 1, np.int32); flat = []
    for i in range(n):
        flat.extend(children[i]); start[i + 1] = len(flat)
    word = np.full(n, -1, np.int32); weight = np.zeros(n, np.float64); w = 0
    for i in range(n):
        if not children[i]:
            word[i] = w; w += 1; weight[i] = float(rng.uniform(0.1, 9.0))
    return start, np.array(flat, np.int32), rng.integers(0, 256, (n, 32), dtype=np.uint8), word, weight, depth


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a); th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def make_pair(rng, nf, cam, scale, lp_dtype, kp_dtype):
    """-> (records of KF1 and KF2, their ivf_local_point arrays, the 16 floats of the similarity, perm, levels)"""
    fx, fy, cx, cy = cam[:4]
    R12 = rot((0.1, 1.0, 0.3), 2.0); t12 = np.array([0.3, 0.1, -0.4]); s12 = 1.2
    u = rng.uniform(80, W - 80, nf); v = rng.uniform(60, H - 60, nf); z = rng.uniform(5, 18, nf)
    X1 = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    X2 = (X1 - t12) @ R12 / s12
    perm = rng.permutation(nf); lv = rng.integers(0, 4, nf)
    desc = rng.integers(0, 256, (nf, 32), dtype=np.uint8)
    proj = lambda X: np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    recs, pts = [], []
    for X, Xo, slot in ((X1, X2, np.arange(nf)), (X2, X1, perm)):                # identity poses: camera frame = world frame per keyframe
        kp = np.zeros(nf, kp_dtype); kp["size"] = 31
        p = proj(X).astype(F)
        kp["x"][slot] = p[:, 0]; kp["y"][slot] = p[:, 1]; kp["octave"][slot] = lv
        d = np.zeros((nf, 32), np.uint8); d[slot] = desc
        P = np.zeros(nf, lp_dtype)
        P["pos"][slot] = X.astype(F)
        dist = np.linalg.norm(Xo, axis=1)
        P["max_distance"][slot] = (dist * 1.2 ** (lv - 0.5)).astype(F); P["min_distance"][slot] = (0.5 * dist).astype(F); P["desc"] = d
        recs.append(dict(kps=kp, desc=d, uright=np.full(nf, -1.0, F), depth=np.full(nf, 8.0, F)))
        pts.append(P)
    sim3 = np.zeros(16, F); sim3[:9] = R12.reshape(9); sim3[9:12] = t12; sim3[12] = s12
    return recs, pts, sim3, perm, lv


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=128); ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sim3_search_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib, dist as ivd
    dev = torch.device("cuda:0")
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    n, nf = a.pairs, a.features
    scale = iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors()
    bounds = (0.0, 0.0, W, H)
    tr = iv.BatchTracker(nf, scale, *cam, bounds, max_pairs=n)
    ls = iv.LoopSearch(tr)
    rng = np.random.default_rng(7)
    voc = make_vocabulary(rng)
    V = iv.ORBVocabulary(*voc)
    recs = []; pts = np.zeros((2 * n, nf), _lib.LOCAL_POINT_DTYPE); sim3 = np.zeros((n, 16), F); first = None
    for p in range(n):
        r, P, s, perm, lv = make_pair(rng, nf, cam, scale, _lib.LOCAL_POINT_DTYPE, _lib.KP_DTYPE)
        recs += r; pts[2 * p] = P[0]; pts[2 * p + 1] = P[1]; sim3[p] = s
        if first is None:
            first = (r, P, perm, lv)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    block = up(ivd.pack_records(recs, nf).reshape(-1))
    pairs = up(np.arange(2 * n, dtype=np.int32).reshape(n, 2))
    poses = up(np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (2 * n, 1)))
    dpts, dsim3 = up(pts.view(np.uint8).reshape(-1)), up(sim3)
    i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev)
    none12, m12, nm, matches, nfound = i32(n, nf), i32(n, nf), i32(n), i32(n, nf), i32(n)
    calls = dict(search_by_bow_keyframes=lambda: ls.search_by_bow_keyframes(V, block, pairs, m12, nm, levelsup=1),
                 search_by_sim3=lambda: ls.search_by_sim3(block, pairs, poses, dpts, dsim3, none12, matches, nfound))
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), pairs=n, features=nf, reps=a.reps)
    for name, call in calls.items():
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        med = float(np.median(ts))
        res[name] = dict(ms_median=med, ms_min=float(np.min(ts)), us_per_pair=med * 1e3 / n)
    res["search_by_bow_keyframes"]["matches_per_pair_mean"] = float(nm.float().mean().item())
    res["search_by_sim3"]["found_per_pair_mean"] = float(nfound.float().mean().item())
    # the per-call path, one pair, wall clock: the projections (here: the true keypoint's position) and the feature vectors precomputed
    (r1, r2), (P1, P2), perm, lv = first
    inv = np.argsort(perm)
    q = lambda tgt, slot_of, P, lvs: dict(u=tgt["kps"]["x"][slot_of], v=tgt["kps"]["y"][slot_of], radius=(F(7.5) * scale[lvs]).astype(F), level=lvs.astype(np.int32),
                                           desc=P["desc"], valid=np.ones(nf, np.uint8))
    q12 = q(r2, perm, P1, lv); q21 = q(r1, inv, P2, lv[inv])
    matcher = iv.ORBmatcher(0.75, True)
    f1 = V.transform(r1["desc"], 1)[1]; f2 = V.transform(r2["desc"], 1)[1]
    has = np.ones(nf, np.uint8)
    percall = dict(search_by_sim3=lambda: matcher.SearchBySim3(r1["kps"], r1["desc"], bounds, r2["kps"], r2["desc"], bounds, q12, q21),
                   search_by_bow_keyframes=lambda: matcher.SearchByBoWKeyFrames(r1["kps"], r1["desc"], has, f1, r2["kps"], r2["desc"], has, f2))
    for name, call in percall.items():
        out = call(); call()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e6)
        res[name]["percall_us_per_pair"] = float(np.median(ts))
        res[name]["percall_result"] = int(out[1])
        res[name]["percall_over_batched"] = res[name]["percall_us_per_pair"] / res[name]["us_per_pair"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
