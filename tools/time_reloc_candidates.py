#!/usr/bin/env python3
"""Time per batch of ivf_tracker_bow_vectors and ivf_tracker_reloc_candidates, the first two lines of Tracking::Relocalization, at the KITTI shape:
128 lost frames and a database of 2000 keyframes of 1000 features each, on a synthetic vocabulary of depth 6 and branching 10.

  python tools/time_reloc_candidates.py [--frames 128] [--keyframes 2000] [--features 1000] [--reps 20] [--out profiles/reloc_candidates_latency.json]

Descriptors are uniform random bits; a lost frame shares 600 of its descriptors with one keyframe and 300 with that keyframe's successor, so that
every frame has a few keyframes far above the common-word threshold; every keyframe lists its ten successors as neighbours.  The database's vectors
are made by ivf_tracker_bow_vectors itself (one call over the 2000 keyframe records, timed too).  Both calls are timed with device events around one
call after a warm-up, median over `reps`.  For scale, the same work is timed on the host over a few frames by the wall clock: ivf_bow_transform +
ivf_bow_vectors per frame (ORBVocabulary.transform), and the plain-Python restatement of DetectRelocalizationCandidates (tests/reloc_db_ref.py).
There is no bar on these numbers: they are recorded, not asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def make_tree(k, depth, rng):
    n = (k ** (depth + 1) - 1) // (k - 1)
    start = np.zeros(n + 1, np.int32)
    inner = (k ** depth - 1) // (k - 1)
    start[1:inner + 1] = k * np.arange(1, inner + 1)
    start[inner + 1:] = k * inner
    child = np.arange(1, n, dtype=np.int32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    word = np.full(n, -1, np.int32); word[inner:] = np.arange(n - inner)
    weight = np.zeros(n, np.float64); weight[inner:] = rng.uniform(0.1, 9.0, n - inner)
    return dict(child_start=start, child=child, desc=desc, word=word, weight=weight, depth=depth)


def event_ms(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=128); ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--features", type=int, default=1000); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_candidates_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib
    from iv_slam_amd.track import record_bytes
    import reloc_db_ref as R
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    nF, nK, nf, mc = a.frames, a.keyframes, a.features, 4
    tree = make_tree(10, 6, rng)
    V = iv.ORBVocabulary(tree["child_start"], tree["child"], tree["desc"], tree["word"], tree["weight"], tree["depth"])
    # the record block: keyframes 0 .. nK - 1, then the lost frames; only the count and the descriptors are read
    rb = record_bytes(nf)
    desc = rng.integers(0, 256, (nK + nF, nf, 32), dtype=np.uint8)
    home = rng.integers(0, nK - 1, nF)
    for f in range(nF):
        desc[nK + f, :600] = desc[home[f], :600]; desc[nK + f, 600:900] = desc[home[f] + 1, 600:900]
    block = np.zeros((nK + nF, rb), np.uint8)
    block[:, :4] = np.array([nf], np.int32).view(np.uint8)
    block[:, 16 + nf * 24:16 + nf * 56] = desc.reshape(nK + nF, nf * 32)
    block = torch.from_numpy(block.reshape(-1)).to(dev)
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    scale = np.asarray(iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors(), F)
    tr = iv.BatchTracker(nf, scale, *cam, (0.0, 0.0, 1241.0, 376.0), max_pairs=nF * mc)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    kw, kv, kn = i32(nK, nf), f64(nK, nf), i32(nK)
    fw, fv, fn = i32(nF, nf), f64(nF, nf), i32(nF)
    kf_frames = torch.arange(nK, dtype=torch.int32, device=dev); lost = torch.arange(nK, nK + nF, dtype=torch.int32, device=dev)
    neigh = torch.from_numpy(np.where(np.arange(nK)[:, None] + 1 + np.arange(10)[None] < nK, np.arange(nK)[:, None] + 1 + np.arange(10)[None], -1).astype(np.int32)).to(dev)
    cand, nc, pairs, sel = i32(nF, mc), i32(nF), i32(nF * mc, 2), i32(nF * mc)
    scores = torch.empty((nF, nK), dtype=torch.float32, device=dev); common = i32(nF, nK)

    def database():
        tr.bow_vectors(V, block, kf_frames, kw, kv, kn)

    def vectors():
        tr.bow_vectors(V, block, lost, fw, fv, fn)

    def candidates():
        tr.reloc_candidates(V, kw, kv, kn, neigh, kf_frames, fw, fv, fn, lost, cand, nc, pairs, sel, scores=scores, common=common)
    for fn_ in (database, vectors, candidates, vectors, candidates):
        fn_()
    torch.cuda.synchronize()
    db_ms = event_ms(database, max(2, a.reps // 4))
    vec_ms = event_ms(vectors, a.reps)
    cand_ms = event_ms(candidates, a.reps)
    ncand = nc.cpu().numpy(); got = cand.cpu().numpy()
    hit = int(sum(int(home[f]) in got[f].tolist() or int(home[f]) + 1 in got[f].tolist() for f in range(nF)))
    # the host paths, over a few frames
    hf = min(a.host_frames, nF)
    t0 = time.perf_counter()
    host_vecs = [V.transform(desc[nK + f], 0)[0] for f in range(hf)]
    per_call_ms = (time.perf_counter() - t0) * 1e3 / hf
    kwh, kvh, knh = kw.cpu().numpy(), kv.cpu().numpy(), kn.cpu().numpy()
    fwh, fvh, fnh = fw.cpu().numpy(), fv.cpu().numpy(), fn.cpu().numpy()
    same_vec = sum(int(sorted(host_vecs[f]) == fwh[f, :fnh[f]].tolist() and [host_vecs[f][w] for w in sorted(host_vecs[f])] == fvh[f, :fnh[f]].tolist()) for f in range(hf))
    kvecs = [list(zip(kwh[k, :knh[k]].tolist(), kvh[k, :knh[k]].tolist())) for k in range(nK)]
    nh = neigh.cpu().numpy()
    t0 = time.perf_counter()
    ref = [R.detect(kvecs, nh, list(zip(fwh[f, :fnh[f]].tolist(), fvh[f, :fnh[f]].tolist())))["cand"] for f in range(hf)]
    python_ms = (time.perf_counter() - t0) * 1e3 / hf
    same_cand = sum(int(len(ref[f]) == ncand[f] and ref[f][:mc] == got[f, :min(mc, len(ref[f]))].tolist()) for f in range(hf))
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), frames=nF, keyframes=nK, features=nf, reps=a.reps,
               vocabulary="synthetic, depth 6, branching 10", max_candidates=mc,
               bow_vectors_launches=2, bow_vectors_ms_median=vec_ms[0], bow_vectors_ms_min=vec_ms[1], bow_vectors_us_per_frame=vec_ms[0] * 1e3 / nF,
               database_bow_vectors_ms_median=db_ms[0], database_bow_vectors_us_per_keyframe=db_ms[0] * 1e3 / nK,
               reloc_candidates_launches=3, reloc_candidates_ms_median=cand_ms[0], reloc_candidates_ms_min=cand_ms[1],
               reloc_candidates_us_per_frame=cand_ms[0] * 1e3 / nF,
               words_per_frame_mean=float(fnh.mean()), candidates_per_frame_mean=float(ncand.mean()), frames_whose_home_keyframe_is_a_candidate=hit,
               host_frames=hf, per_call_transform_ms_per_frame=per_call_ms, python_restatement_ms_per_frame=python_ms,
               host_frames_where_vectors_agree=same_vec, host_frames_where_candidates_agree=same_cand)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
