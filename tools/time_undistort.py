#!/usr/bin/env python3
"""Cost of Frame::UndistortKeyPoints inside the batch (ivf_frontend_set_camera): the batched front end at the
benchmark's shape (128 pairs of 1242x375, 1000 features) with and without a TUM1-like camera -- kernel launches per batch
(ivf_debug_launch_count) and wall time per batch over `--batches` batches, three contexts in flight.

  python tools/time_undistort.py [--batches 30]
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o u -- python tools/time_undistort.py     # k_undistort_keys beside the batch's kernels

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30); ap.add_argument("--pairs", type=int, default=128)
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import synth
    lib = iv.load()
    w, h, nf = 1242, 375, 1000
    dev = torch.device("cuda:0")
    pairs = [synth.make_pair(w, h, seed=5, idx=i) for i in range(8)]
    L = torch.from_numpy(np.stack([pairs[i % 8][0] for i in range(a.pairs)])).to(dev)
    R = torch.from_numpy(np.stack([pairs[i % 8][1] for i in range(a.pairs)])).to(dev)
    fe = iv.StereoFrontend(w, h, a.pairs, nfeatures=nf)
    # TUM1's distortion (Examples/RGB-D/TUM1.yaml) on the benchmark's intrinsics
    cam = iv.Camera(718.856, 718.856, 607.1928, 185.2157, [0.262383, -0.953104, -0.005358, 0.002628, 1.163314])
    out = {}
    for label, c in (("no_camera", None), ("camera", cam), ("no_camera_again", None), ("camera_again", cam)):
        fe.set_camera(c)
        for _ in range(3):
            fe.run(L, R)
        fe.sync()
        n0 = lib.ivf_debug_launch_count()
        t0 = time.perf_counter()
        for _ in range(a.batches):
            fe.run(L, R)
        fe.sync()
        dt = time.perf_counter() - t0
        out[label] = dict(ms_per_batch=round(1e3 * dt / a.batches, 4), launches_per_batch=(lib.ivf_debug_launch_count() - n0) / a.batches)
    n_kp = int(sum(len(fe.fetch(k, 0)["kps"]) for k in range(a.pairs)))
    print(json.dumps(dict(tool="time_undistort", pairs=a.pairs, size=[w, h], nfeatures=nf, batches=a.batches, left_keypoints_per_batch=n_kp,
                          build=lib.ivf_build_id().decode(), **out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
