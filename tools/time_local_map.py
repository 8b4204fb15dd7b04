#!/usr/bin/env python3
"""Time per batch of ivf_tracker_update_local_map and of the three tail calls of TrackLocalMap (merge_local, points_from_map,
close_local_map), and of ivf_tracker_search_local on the lists that call writes, padded as it writes them and as a compact CSR of the
same lists built on the host: 128 frames of 1000 features against a synthetic map of 2000 keyframes.

  python tools/time_local_map.py [--frames 128] [--keyframes 2000] [--features 1000] [--runs 5] [--out profiles/local_map_latency.json]

The map is a corridor: keyframe k holds the points 40 k + floor(1.2 i), i < 1000, so a point is observed by about 25 keyframes, a frame
that holds 300 points of its home keyframe votes for about 60 keyframes and their rows hold 3000-4000 distinct points.  Every keyframe
lists its ten successors as neighbours, its successor as child and its predecessor as parent.  The points lie in front of the camera
(identity pose) inside their distance range, so the search projects them and walks their windows; the records are the front end's, from
the benchmark's synthetic scene.  Each call is timed with device events after a warm-up, median over `runs`: update_local_map and the
searches as one call between two events (frame_points is restored before the first event, outside the interval), the tail calls as 20
calls back to back divided by 20, because one of them is near the resolution of the events.  The launches are the library's own count.
The memset of the hash sets is timed alone (hipMemsetAsync of the same number of bytes on a buffer of the tool's) to give its share of
update_local_map.  search_local's difference between the two layouts is the price of the fixed stride: it decides whether a later
change compacts.  The result is checked against the restatement (tests/local_map_ref.py) on two frames, and the two searches must give
the same matches.  There is no bar on these numbers: they are recorded, not asserted."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def event_ms(fn, reps, calls=1, before=None):
    """median and minimum over `reps` of the time of `calls` calls of fn back to back, per call; before() runs outside the interval"""
    import torch
    ts = []
    for _ in range(reps):
        if before:
            before()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ts)), float(np.min(ts))


def hip_memset_async():
    """hipMemsetAsync of the HIP runtime this process has loaded, or None"""
    try:
        with open("/proc/self/maps") as f:
            paths = sorted(set(l.split()[-1] for l in f if "libamdhip64" in l))
        fn = C.CDLL(paths[0]).hipMemsetAsync
        fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        return fn
    except (OSError, IndexError, AttributeError):
        return None


def corridor(nK, nf, rng):
    import local_map_ref as R
    from iv_slam_amd._lib import LOCAL_POINT_DTYPE
    span = (np.arange(nf) * 1.2).astype(np.int64)
    kfp = (40 * np.arange(nK)[:, None] + span[None]).astype(np.int32)
    nP = int(kfp.max()) + 1
    pts = np.zeros(nP, LOCAL_POINT_DTYPE)
    pos = np.stack([rng.uniform(-12, 12, nP), rng.uniform(-3, 3, nP), rng.uniform(6, 40, nP)], 1).astype(F)
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1))
    pts["pos"] = pos; pts["normal"] = (pos / dist[:, None]).astype(F)               # seen head-on from the origin
    pts["max_distance"] = (dist * 1.2 ** 3).astype(F); pts["min_distance"] = (pts["max_distance"] / F(1.2 ** 7)).astype(F)
    pts["desc"] = rng.integers(0, 256, (nP, 32), dtype=np.uint8)
    pts["flags"] = 2
    pts["flags"][rng.random(nP) < 0.02] |= 1
    flat = kfp.reshape(-1)
    by_point = np.argsort(flat, kind="stable")
    obs_kf = (by_point // nf).astype(np.int32)
    obs_off = np.zeros(nP + 1, np.int32); obs_off[1:] = np.cumsum(np.bincount(flat, minlength=nP))
    k = np.arange(nK)
    nb = k[:, None] + 1 + np.arange(10)[None]
    neigh = np.where(nb < nK, nb, -1).astype(np.int32)
    child = np.where(k + 1 < nK, k + 1, -1)
    c_off = np.zeros(nK + 1, np.int32); c_off[1:] = np.cumsum(child >= 0)
    return R.Map(pts, obs_off, obs_kf, np.arange(nK + 1, dtype=np.int32) * nf, flat, neigh, c_off, child[child >= 0], k - 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=128); ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--features", type=int, default=1000); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib
    from iv_slam_amd.track import MapView
    import local_map_ref as R
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    nF, nK, nf, max_lk, max_pts = a.frames, a.keyframes, a.features, 96, 4096
    M = corridor(nK, nf, rng)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    view = MapView(up(M.points.view(np.uint8).reshape(-1)), up(M.obs_offsets), up(M.obs_kf), up(M.kf_point_offsets), up(M.kf_points), up(M.kf_neigh),
                   up(M.kf_child_offsets), up(M.kf_children), up(M.kf_parent))
    home = rng.integers(60, nK - 60, nF)
    fp0 = np.full((nF, nf), -1, np.int32)
    for f in range(nF):
        at = rng.choice(nf, 300, replace=False)
        fp0[f, at] = M.kf_points[home[f] * nf + rng.choice(nf, 300, replace=False)]
    scale = np.asarray(iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors(), F)
    tr = iv.BatchTracker(nf, scale, 718.856, 718.856, 607.1928, 185.2157, 386.1448, (0.0, 0.0, 1241.0, 376.0), max_pairs=nF)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    fp_in = up(fp0); fp = fp_in.clone()
    lk, nlk, ref = i32(nF, max_lk), i32(nF), i32(nF)
    pts = torch.zeros(nF * max_pts * 80, dtype=torch.uint8, device=dev); ids, off, npts = i32(nF, max_pts), i32(nF + 1), i32(nF)
    occ = torch.zeros((nF, nf), dtype=torch.uint8, device=dev)
    assign = up(np.where(rng.random((nF, nf)) < 0.3, rng.integers(0, 3000, (nF, nf)), -1).astype(np.int32))
    xw = torch.zeros((nF, nf, 3), dtype=torch.float32, device=dev); has = torch.zeros((nF, nf), dtype=torch.uint8, device=dev)
    q = torch.zeros((nF, nf), dtype=torch.float32, device=dev); pq = up(rng.uniform(0.2, 1, M.n_points).astype(F))
    outl = up((rng.random((nF, nf)) < 0.1).astype(np.uint8)); nin = i32(nF)
    lib = _lib.load()

    def restore():
        fp.copy_(fp_in)

    def update():
        tr.update_local_map(view, fp, lk, nlk, ref, pts, ids, off, npts, occ)
    res = dict(build_id=lib.ivf_build_id().decode(), device=torch.cuda.get_device_name(0), frames=nF, keyframes=nK, features=nf, runs=a.runs,
               map_points=M.n_points, max_local_keyframes=max_lk, max_points_per_frame=max_pts)

    def timed(name, fn, calls=1, before=None):
        if before:
            before()
        fn(); torch.cuda.synchronize()
        n0 = lib.ivf_debug_launch_count(); fn(); res[name + "_launches"] = int(lib.ivf_debug_launch_count() - n0)
        torch.cuda.synchronize()
        res[name + "_ms_median"], res[name + "_ms_min"] = event_ms(fn, a.runs, calls, before)
    timed("update_local_map", update, before=restore)
    # the memset of the hash sets alone
    set_bytes = int(lib.ivf_tracker_local_map_set_bytes(nf, M.n_points, nF, max_lk))
    res["hash_set_bytes"] = set_bytes
    memset = hip_memset_async()
    if memset is not None and set_bytes > 0:
        buf = torch.empty(set_bytes, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        clear = lambda: memset(buf.data_ptr(), 0xff, set_bytes, st)
        clear(); torch.cuda.synchronize()
        res["hash_set_memset_ms_median"], res["hash_set_memset_ms_min"] = event_ms(clear, a.runs)
        res["hash_set_memset_share_of_update_local_map"] = res["hash_set_memset_ms_median"] / res["update_local_map_ms_median"]
        del buf
    restore(); update(); torch.cuda.synchronize()
    # ---- search_local on the lists just written: padded (the fixed stride) and as a compact CSR built on the host
    import bench
    from iv_slam_amd import synth
    L0, R0 = synth.make_pair(bench.W, bench.H, seed=100, idx=0)
    bl = torch.from_numpy(L0).to(dev); br = torch.from_numpy(R0).to(dev)
    left = torch.stack([torch.roll(bl, 3 * k, dims=1) for k in range(nF)]); right = torch.stack([torch.roll(br, 3 * k, dims=1) for k in range(nF)])
    fe = iv.StereoFrontend(bench.W, bench.H, nF, nfeatures=nf, iniThFAST=20, minThFAST=7, bf=bench.BF, fx=bench.FX)
    fe.run(left, right)
    block = torch.zeros(nF * fe.gather_record_bytes(), dtype=torch.uint8, device=dev)
    fe.pack_gather_block(block); fe.sync(); torch.cuda.synchronize()
    dfr = torch.arange(nF, dtype=torch.int32, device=dev)
    cnt = np.minimum(npts.cpu().numpy(), max_pts)
    padded = pts.cpu().numpy().reshape(nF, max_pts * 80)
    c_off = np.zeros(nF + 1, np.int32); c_off[1:] = np.cumsum(cnt)
    compact = up(np.concatenate([padded[f, :cnt[f] * 80] for f in range(nF)])); d_coff = up(c_off)
    sa = [torch.empty((nF, nf), dtype=torch.int32, device=dev) for _ in range(2)]; sn = [torch.empty(nF, dtype=torch.int32, device=dev) for _ in range(2)]
    timed("search_local_padded", lambda: tr.search_local(block, dfr, pts, off, max_pts, sa[0], sn[0], occupied=occ, th=1.0, nn_ratio=0.8))
    timed("search_local_compact", lambda: tr.search_local(block, dfr, compact, d_coff, max_pts, sa[1], sn[1], occupied=occ, th=1.0, nn_ratio=0.8))
    torch.cuda.synchronize()
    res["search_local_padding_cost_ms"] = res["search_local_padded_ms_median"] - res["search_local_compact_ms_median"]
    res["search_local_layouts_agree"] = bool(torch.equal(sa[0], sa[1]) and torch.equal(sn[0], sn[1]))
    res["search_local_matches_mean"] = float(sn[0].float().mean())
    res["padded_records"], res["compact_records"] = nF * max_pts, int(c_off[-1])
    timed("merge_local", lambda: tr.merge_local(ids, off, assign, fp), calls=20)
    timed("points_from_map", lambda: tr.points_from_map(view, fp, xw, has, quality=q, point_quality=pq), calls=20)
    timed("close_local_map", lambda: tr.close_local_map(view, outl, fp, nin), calls=20)
    restore(); update(); torch.cuda.synchronize()
    res["update_local_map_us_per_frame"] = res["update_local_map_ms_median"] * 1e3 / nF
    res["local_keyframes_mean"] = float(nlk.float().mean()); res["local_points_mean"] = float(npts.float().mean())
    agree = 0
    for f in (0, nF - 1):
        w = R.update_local_map(M, fp0[f], np.zeros(max_lk, np.int32), 0, 0, nf, max_pts)
        agree += int(w["point_ids"].tobytes() == ids[f].cpu().numpy().tobytes() and w["local_kf"].tobytes() == lk[f].cpu().numpy().tobytes())
    res["frames_checked_against_restatement"], res["frames_that_agree"] = 2, agree
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0 if agree == 2 and res["search_local_layouts_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
