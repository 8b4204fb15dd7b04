#!/usr/bin/env python3
"""Time per pair of ivf_tracker_search_by_bow (node ids, feature vectors and the search: one call, three kernels) next to the per-call
path on the same inputs: ivf_bow_transform + ivf_bow_vectors of both frames and ivf_search_by_bow, which cross PCIe and replay the
greedy loop on the host.  128 (keyframe, current) pairs, 1000 features, a synthetic tree (branching 10, depth 3, nodes at level 2:
about 100 nodes, as the ORB vocabulary gives at levelsup 4).

  python tools/time_track_bow.py [--pairs 128] [--features 1000] [--reps 30] [--percall-pairs 16] [--out profiles/track_bow_latency.json]

The batched call is timed with device events around `reps` calls after a warm-up (median); the per-call path with the wall clock over
`percall-pairs` pairs.  The split of the batched call over its kernels (k_bow_nodes, k_bow_featvec, k_bow_search) is read from a kernel
trace of this script; the script itself reports the whole call."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32


def make_tree(rng, k, depth):
    children = [[]]; frontier = [0]
    for _ in range(depth):
        nxt = []
        for node in frontier:
            for _ in range(k):
                children.append([]); children[node].append(len(children) - 1); nxt.append(len(children) - 1)
        frontier = nxt
    n = len(children)
    start = np.zeros(n + 1, np.int32); flat = []
    for i in range(n):
        flat.extend(children[i]); start[i + 1] = len(flat)
    word = np.full(n, -1, np.int32); weight = np.zeros(n, np.float64); w = 0
    for i in range(n):
        if not children[i]:
            word[i] = w; w += 1; weight[i] = float(rng.uniform(0.1, 9.0))
    return dict(child_start=start, child=np.array(flat, np.int32), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), word=word, weight=weight, depth=depth)


def make_records(rng, n_frames, nf):
    """frame k + 1 = frame k's descriptors with a few bits flipped, in another order"""
    from iv_slam_amd._lib import KP_DTYPE
    desc = rng.integers(0, 256, (nf, 32), dtype=np.uint8)
    recs = []
    for _ in range(n_frames):
        kp = np.zeros(nf, KP_DTYPE)
        kp["x"] = rng.uniform(30, 1200, nf).astype(F); kp["y"] = rng.uniform(30, 340, nf).astype(F); kp["size"] = 31
        kp["angle"] = rng.uniform(0, 20, nf).astype(F)
        recs.append(dict(kps=kp, desc=desc.copy(), uright=(kp["x"] - F(20.0)).astype(F), depth=np.full(nf, 19.0, F)))
        flips = rng.integers(0, 256, (nf, 6))
        desc = desc[rng.permutation(nf)].copy()
        for j in range(6):
            desc[np.arange(nf), flips[:, j] // 8] ^= (1 << (flips[:, j] % 8)).astype(np.uint8)
    return recs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=128); ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--percall-pairs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "track_bow_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib, dist as ivd
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    n, nf, levelsup = a.pairs, a.features, 1
    tree = make_tree(rng, 10, 3)
    V = iv.ORBVocabulary(tree["child_start"], tree["child"], tree["desc"], tree["word"], tree["weight"], tree["depth"])
    recs = make_records(rng, n + 1, nf)
    sc = iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors()
    tr = iv.BatchTracker(nf, sc, 718.856, 718.856, 607.1928, 185.2157, 386.1448, (0.0, 0.0, 1241.0, 376.0), max_pairs=n)
    block = torch.from_numpy(ivd.pack_records(recs, nf).reshape(-1)).to(dev)
    pairs = torch.tensor([(k, k + 1) for k in range(n)], dtype=torch.int32, device=dev)
    assign = torch.empty((n, nf), dtype=torch.int32, device=dev); nm = torch.empty(n, dtype=torch.int32, device=dev)

    def batched():
        tr.search_by_bow(V, block, pairs, assign, nm, levelsup=levelsup)
    for _ in range(3):
        batched()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); batched(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    got = assign.cpu().numpy(); gnm = nm.cpu().numpy()

    m = iv.ORBmatcher(0.7, True)
    has = np.ones(nf, np.uint8)
    k_pc = min(a.percall_pairs, n)

    def percall(k):
        _, kfv = V.transform(recs[k]["desc"], levelsup); _, ffv = V.transform(recs[k + 1]["desc"], levelsup)
        return m.SearchByBoW(recs[k]["kps"], recs[k]["desc"], has, kfv, recs[k + 1]["kps"], recs[k + 1]["desc"], ffv)
    percall(0)
    t0 = time.perf_counter()
    same = True
    for k in range(k_pc):
        pm, pn = percall(k)
        same = same and pn == gnm[k] and np.array_equal(pm, got[k])
    t_pc = (time.perf_counter() - t0) / k_pc
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), pairs=n, features=nf, levelsup=levelsup,
               tree_nodes=int(len(tree["word"])), reps=a.reps, matches_per_pair_mean=float(gnm.mean()),
               batched_ms_median=float(np.median(ts)), batched_ms_min=float(np.min(ts)), batched_us_per_pair=float(np.median(ts)) * 1e3 / n,
               percall_pairs_timed=k_pc, percall_us_per_pair=t_pc * 1e6, percall_equals_batched=bool(same))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
