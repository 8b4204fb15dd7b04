#!/usr/bin/env python3
"""Time per batch of ivf_tracker_create_map_points: 128 keyframes x 10 neighbours x 1000 features.

  python tools/time_create_points.py [--keyframes 128] [--neighbours 10] [--features 1000] [--runs 5] [--out profiles/create_points_latency.json]

The records are the front end's, from the benchmark's synthetic scene shifted by 3 px per frame; keyframe k stands at x = 2 b k (past the
baseline gate) with the identity rotation and takes the ten records behind it as neighbours; half of the keypoints hold a point already.
The vocabulary is a complete tree of branching 10 and depth 3 whose node descriptors are drawn from the records, levelsup = 1: about a
hundred nodes of ten features each, as ORBvoc gives at levelsup = 4.  The whole call (three launches) is timed with device events after a
warm-up, median over `runs`; the launches are the library's own count.  The call does not expose its phases: the JSON holds the whole call.  There is no
bar on these numbers: they are recorded, not asserted."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32


def complete_tree(k, depth, pool, rng):
    n_inner = (k ** depth - 1) // (k - 1); n = (k ** (depth + 1) - 1) // (k - 1)
    start = np.zeros(n + 1, np.int32); child = []
    for i in range(n):
        if i < n_inner:
            child.extend(range(k * i + 1, k * i + k + 1))
        start[i + 1] = len(child)
    desc = np.zeros((n, 32), np.uint8); desc[1:] = pool[rng.integers(0, len(pool), n - 1)]
    word = np.full(n, -1, np.int32); word[n_inner:] = np.arange(n - n_inner)
    weight = np.zeros(n, np.float64); weight[n_inner:] = 1.0
    return start, np.array(child, np.int32), desc, word, weight


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keyframes", type=int, default=128); ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--features", type=int, default=1000); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "create_points_latency.json"))
    a = ap.parse_args()
    import torch
    import bench
    import iv_slam_amd as iv
    from iv_slam_amd import _lib, synth
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    nK, mn, nf = a.keyframes, a.neighbours, a.features
    L0, R0 = synth.make_pair(bench.W, bench.H, seed=100, idx=0)
    bl = torch.from_numpy(L0).to(dev); br = torch.from_numpy(R0).to(dev)
    left = torch.stack([torch.roll(bl, 3 * k, dims=1) for k in range(nK)]); right = torch.stack([torch.roll(br, 3 * k, dims=1) for k in range(nK)])
    fe = iv.StereoFrontend(bench.W, bench.H, nK, nfeatures=nf, iniThFAST=20, minThFAST=7, bf=bench.BF, fx=bench.FX)
    fe.run(left, right)
    rec_bytes = fe.gather_record_bytes()
    block = torch.zeros(nK * rec_bytes, dtype=torch.uint8, device=dev)
    fe.pack_gather_block(block); fe.sync(); torch.cuda.synchronize()
    host = block.cpu().numpy().reshape(nK, rec_bytes)
    pool = host[:, 16 + nf * 24:16 + nf * 56].reshape(-1, 32)
    pool = pool[pool.any(axis=1)]
    voc = iv.ORBVocabulary(*complete_tree(10, 3, pool, rng), 3)
    scale = np.asarray(iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors(), F)
    tr = iv.BatchTracker(nf, scale, bench.FX, bench.FX, bench.W / 2.0, bench.H / 2.0, bench.BF, (0.0, 0.0, float(bench.W), float(bench.H)), max_pairs=nK * mn)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    poses = np.tile(np.eye(4, dtype=F)[:3].reshape(12), (nK, 1)); poses[:, 3] = -2.0 * (bench.BF / bench.FX) * np.arange(nK)                 # x = 2 b k: past the baseline gate
    kf = np.arange(nK, dtype=np.int32)
    neigh = ((kf[:, None] + 1 + np.arange(mn)[None]) % nK).astype(np.int32)
    has = (rng.random((nK, nf)) < 0.5).astype(np.uint8)
    d = dict(kf=up(kf), neigh=up(neigh), poses=up(poses), has=up(has), kq=up(rng.uniform(0.1, 1, (nK, nf)).astype(F)),
             pts=torch.zeros(nK * nf * 80, dtype=torch.uint8, device=dev), nn=torch.zeros((nK, nf), dtype=torch.int32, device=dev),
             i2=torch.zeros((nK, nf), dtype=torch.int32, device=dev), od=torch.zeros((nK, nf), dtype=torch.int32, device=dev),
             q=torch.zeros((nK, nf), dtype=torch.float32, device=dev), nnew=torch.zeros(nK, dtype=torch.int32, device=dev),
             m=torch.zeros((nK, mn, nf), dtype=torch.int32, device=dev))
    lib = _lib.load()

    def call():
        tr.create_map_points(voc, block, d["kf"], d["neigh"], d["poses"], d["has"], d["pts"], d["nn"], d["i2"], d["od"], d["q"], d["nnew"], levelsup=1,
                             key_quality=d["kq"], matches=d["m"])
    call(); torch.cuda.synchronize()
    n0 = lib.ivf_debug_launch_count(); call(); launches = int(lib.ivf_debug_launch_count() - n0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.runs):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    res = dict(build_id=lib.ivf_build_id().decode(), device=torch.cuda.get_device_name(0), keyframes=nK, neighbours=mn, features=nf, runs=a.runs,
               shape="one workgroup of 512 threads per keyframe walks the ranks", launches=launches,
               create_map_points_ms_median=float(np.median(ts)), create_map_points_ms_min=float(np.min(ts)),
               us_per_keyframe=float(np.median(ts)) * 1e3 / nK, matches_mean_per_keyframe=float((d["m"] >= 0).sum().item()) / nK,
               new_points_mean_per_keyframe=float(d["nnew"].float().mean()))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
