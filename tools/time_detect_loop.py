#!/usr/bin/env python3
"""Time per batch of ivf_tracker_loop_candidates and ivf_tracker_loop_consistency, LoopClosing::DetectLoop on the device, at the KITTI shape of
tools/time_reloc_candidates.py (whose synthetic vocabulary of depth 6 and branching 10 and whose descriptors it borrows): 128 new keyframes
appended to a database of 2000 keyframes of 1000 features each, every keyframe connected to its 30 predecessors, and
ivf_tracker_reloc_candidates on the same batch in the same run for comparison.

  python tools/time_detect_loop.py [--queries 128] [--keyframes 2000] [--features 1000] [--reps 20] [--out profiles/detect_loop_latency.json]

A new keyframe shares 600 of its descriptors with one old keyframe (far enough back not to be connected) and 300 with that keyframe's successor;
query q is row keyframes + q of the database and sees the rows before it (visible = its own index), i.e. the batch is the reference's
sequential DetectLoop over 128 consecutive keyframes from one snapshot.  The consistency state starts empty with room for 64 groups of 64.
Each call is timed with device events around one call after a warm-up, median over `reps` (the consistency call starts from the empty state
every time, reset ahead of the first event).  On this batch a query has about one candidate and no group lasts, so the consistency figure is
the floor of the call: per query a chain of about ten workgroup barriers with a global round trip between them.  The candidates of a few queries are compared with the plain-Python restatement (tests/loop_detect_ref.py), timed by the wall
clock.  There is no bar on these numbers: they are recorded, not asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32
CONNECTED = 30


def event_ms(fn, reps, before=None):
    """(median, minimum) of device-event times around one call of fn; `before` runs ahead of the first event of every repetition"""
    import torch
    ts = []
    for _ in range(reps):
        if before:
            before()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--queries", type=int, default=128); ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--features", type=int, default=1000); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-queries", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_loop_latency.json"))
    a = ap.parse_args()
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import _lib
    from iv_slam_amd.track import record_bytes
    from time_reloc_candidates import make_tree
    import loop_detect_ref as L
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    nQ, nOld, nf, mc, gc, mem = a.queries, a.keyframes, a.features, 4, 64, 64
    nK = nOld + nQ
    tree = make_tree(10, 6, rng)
    V = iv.ORBVocabulary(tree["child_start"], tree["child"], tree["desc"], tree["word"], tree["weight"], tree["depth"])
    rb = record_bytes(nf)
    desc = rng.integers(0, 256, (nK, nf, 32), dtype=np.uint8)
    home = rng.integers(0, nOld - 4 * CONNECTED, nQ)
    for q in range(nQ):
        desc[nOld + q, :600] = desc[home[q], :600]; desc[nOld + q, 600:900] = desc[home[q] + 1, 600:900]
    block = np.zeros((nK, rb), np.uint8)
    block[:, :4] = np.array([nf], np.int32).view(np.uint8)
    block[:, 16 + nf * 24:16 + nf * 56] = desc.reshape(nK, nf * 32)
    block = torch.from_numpy(block.reshape(-1)).to(dev)
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    scale = np.asarray(iv.ORBextractor(nf, 1.2, 8, 20, 7).GetScaleFactors(), F)
    tr = iv.BatchTracker(nf, scale, *cam, (0.0, 0.0, 1241.0, 376.0), max_pairs=nQ * mc)
    ls = iv.LoopSearch(tr)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    kw, kv, kn = i32(nK, nf), torch.empty((nK, nf), dtype=torch.float64, device=dev), i32(nK)
    rows = torch.arange(nK, dtype=torch.int32, device=dev)
    idx = np.arange(nK)[:, None]
    neigh_h = np.where(idx + 1 + np.arange(10)[None] < nK, idx + 1 + np.arange(10)[None], -1).astype(np.int32)
    conn_rows = [list(range(max(0, k - CONNECTED), k)) for k in range(nK)]
    start_h = np.concatenate([[0], np.cumsum([len(r) for r in conn_rows])]).astype(np.int32)
    conn_h = np.array([c for r in conn_rows for c in r], np.int32)
    neigh, start, conn = (torch.from_numpy(x).to(dev) for x in (neigh_h, start_h, conn_h))
    qk = torch.arange(nOld, nK, dtype=torch.int32, device=dev)
    ms = torch.empty(nQ, dtype=torch.float32, device=dev)
    cand, nc = i32(nQ, mc), i32(nQ)
    scores = torch.empty((nQ, nK), dtype=torch.float32, device=dev); common = i32(nQ, nK)
    member0 = torch.full((gc, mem), -1, dtype=torch.int32, device=dev)
    member, size, count, ng = member0.clone(), torch.zeros(gc, dtype=torch.int32, device=dev), torch.zeros(gc, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    en, nen, pairs, sel, status = i32(nQ, mc), i32(nQ), i32(nQ, mc, 2), i32(nQ, mc), i32(nQ)
    rcand, rnc, rpairs, rsel = i32(nQ, mc), i32(nQ), i32(nQ * mc, 2), i32(nQ * mc)
    tr.bow_vectors(V, block, rows, kw, kv, kn)

    def candidates():
        ls.loop_candidates(kw, kv, kn, neigh, start, conn, qk, qk, ms, cand, nc, scores=scores, common=common)

    def empty_state():
        ng.zero_()                                             # every repetition starts from an empty state: outside the timed interval

    def consistency():
        ls.loop_consistency(rows, start, conn, qk, cand, nc, member, size, count, ng, en, nen, pairs, sel, status, th=3)

    def reloc():
        tr.reloc_candidates(V, kw, kv, kn, neigh, rows, kw[nOld:], kv[nOld:], kn[nOld:], qk, rcand, rnc, rpairs, rsel, scores=scores, common=common)
    for fn_ in (candidates, consistency, reloc, candidates, empty_state, consistency, reloc):
        fn_()
    torch.cuda.synchronize()
    reloc_ms = event_ms(reloc, a.reps)
    cand_ms = event_ms(candidates, a.reps)
    cons_ms = event_ms(consistency, a.reps, before=empty_state)
    reloc2_ms = event_ms(reloc, a.reps)                        # once more behind the loop calls: the spread of the comparison itself
    candidates(); torch.cuda.synchronize()
    ncand = nc.cpu().numpy(); got = cand.cpu().numpy(); msh = ms.cpu().numpy()
    hit = int(sum(int(home[q]) in got[q].tolist() or int(home[q]) + 1 in got[q].tolist() for q in range(nQ)))
    hq = min(a.host_queries, nQ)
    kwh, kvh, knh = kw.cpu().numpy(), kv.cpu().numpy(), kn.cpu().numpy()
    kvecs = [list(zip(kwh[k, :knh[k]].tolist(), kvh[k, :knh[k]].tolist())) for k in range(nK)]
    fields = L.Fields(nK)
    t0 = time.perf_counter()
    ref = [L.detect(fields, kvecs, neigh_h, None, conn_rows, nOld + q, nOld + q) for q in range(hq)]
    python_ms = (time.perf_counter() - t0) * 1e3 / hq
    same = sum(int(len(ref[q]["cand"]) == ncand[q] and ref[q]["cand"][:mc] == got[q, :min(mc, ncand[q])].tolist()
                   and F(ref[q]["min_score"]).tobytes() == msh[q].tobytes()) for q in range(hq))
    res = dict(build_id=_lib.load().ivf_build_id().decode(), device=torch.cuda.get_device_name(0), queries=nQ, keyframes=nK, features=nf, reps=a.reps,
               vocabulary="synthetic, depth 6, branching 10", max_candidates=mc, connected_per_keyframe=CONNECTED, group_cap=gc, member_cap=mem,
               loop_candidates_launches=4, loop_candidates_ms_median=cand_ms[0], loop_candidates_ms_min=cand_ms[1],
               loop_candidates_us_per_query=cand_ms[0] * 1e3 / nQ,
               loop_consistency_launches=1, loop_consistency_ms_median=cons_ms[0], loop_consistency_ms_min=cons_ms[1],
               loop_consistency_us_per_query=cons_ms[0] * 1e3 / nQ,
               reloc_candidates_same_batch_ms_median=reloc_ms[0], reloc_candidates_same_batch_ms_min=reloc_ms[1],
               reloc_candidates_same_batch_again_ms_median=reloc2_ms[0],
               loop_over_reloc=cand_ms[0] / reloc_ms[0],
               candidates_per_query_mean=float(ncand.mean()), queries_whose_home_keyframe_is_a_candidate=hit,
               enough_consistent_queries=int((nen.cpu().numpy() > 0).sum()), groups_at_the_end=int(ng.cpu().numpy()[0]), status_any=int(status.cpu().numpy().any()),
               host_queries=hq, python_restatement_ms_per_query=python_ms, host_queries_where_candidates_agree=same)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
