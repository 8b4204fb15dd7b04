"""ivf_tracker_update_local_map and the tail of TrackLocalMap (iv_slam_amd/csrc/ivf_track_map.hip, ivf_track_points.hip) against
tests/local_map_ref.py, the restatement of Tracking::UpdateLocalMap (ORB/src/Tracking.cc:2134-2270) and of :1648-1677, at 256
features.  Bar: every output array byte for byte, on outputs pre-filled with marks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_gpu_track import extracted_sequence, iv  # noqa: F401  (iv: the module fixture)
from test_gpu_track_local import map_points_from, pack_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import local_map_ref as R          # noqa: E402
import local_map_scenes as SC      # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
NF = SC.NF
SCENES = SC.all_scenes()
MARK = -77


@pytest.fixture(scope="module")
def tracker(iv):
    sf = np.array([1.2 ** i for i in range(8)], F)
    return iv.BatchTracker(NF, sf, 700.0, 700.0, 600.0, 180.0, 380.0, (0.0, 0.0, 1241.0, 376.0), max_pairs=64)


def to_view(M):
    import torch
    from iv_slam_amd.track import MapView
    dev = torch.device("cuda:0")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return MapView(up(M.points.view(np.uint8).reshape(-1)), up(M.obs_offsets), up(M.obs_kf), up(M.kf_point_offsets), up(M.kf_points),
                   up(M.kf_neigh), up(M.kf_child_offsets), up(M.kf_children), up(M.kf_parent), kf_live=up(M.kf_live), kf_order=up(M.kf_order))


def run_device(tr, M, fps, prev_rows, prev_ns, prev_refs, max_pts, view=None):
    """one call for len(fps) frames -> list of output dicts shaped like the restatement's, and the device tensors"""
    import torch
    dev = torch.device("cuda:0")
    n = len(fps)
    view = view or to_view(M)
    d = dict(fp=torch.from_numpy(np.stack(fps)).to(dev), lk=torch.from_numpy(np.stack(prev_rows)).to(dev),
             nlk=torch.tensor(prev_ns, dtype=torch.int32, device=dev), ref=torch.tensor(prev_refs, dtype=torch.int32, device=dev),
             pts=torch.full((n * max_pts * 80,), 0xAB, dtype=torch.uint8, device=dev), ids=torch.full((n, max_pts), MARK, dtype=torch.int32, device=dev),
             off=torch.full((n + 1,), MARK, dtype=torch.int32, device=dev), npts=torch.full((n,), MARK, dtype=torch.int32, device=dev),
             occ=torch.full((n, NF), 0xAB, dtype=torch.uint8, device=dev), view=view)
    tr.update_local_map(view, d["fp"], d["lk"], d["nlk"], d["ref"], d["pts"], d["ids"], d["off"], d["npts"], d["occ"])
    torch.cuda.synchronize()
    assert d["off"].cpu().numpy().tolist() == [f * max_pts for f in range(n + 1)]
    pts = d["pts"].cpu().numpy().view(R.LOCAL_POINT_DTYPE).reshape(n, max_pts)
    h = {k: d[k].cpu().numpy() for k in ("fp", "lk", "nlk", "ref", "ids", "npts", "occ")}
    outs = [dict(frame_points=h["fp"][f], local_kf=h["lk"][f], n_local_kf=h["nlk"][f], ref_kf=h["ref"][f], points=pts[f], point_ids=h["ids"][f],
                 n_local_points=h["npts"][f], occupied=h["occ"][f]) for f in range(n)]
    return outs, d


def expect(M, sc_inputs, max_pts):
    return [R.update_local_map(M, fp, row, pn, pr, NF, max_pts) for fp, row, pn, pr in sc_inputs]


def assert_same(got, want, what):
    for f, (g, w) in enumerate(zip(got, want)):
        k = R.same(w, g)
        assert k is None, "%s frame %d: %s differs: device %r, restatement %r" % (what, f, k, np.asarray(g[k]).reshape(-1)[:12], np.asarray(w[k]).reshape(-1)[:12])


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scene_alone(tracker, sc):
    M = sc["map"]
    inp = [(sc["frame_points"], sc["prev_row"], sc["prev_n"], sc["prev_ref"])]
    got, _ = run_device(tracker, M, [sc["frame_points"]], [sc["prev_row"]], [sc["prev_n"]], [sc["prev_ref"]], sc["max_pts"])
    assert_same(got, expect(M, inp, sc["max_pts"]), sc["name"])


def merge_maps(maps):
    """one map holding every scene's, each followed by a dead keyframe and a bad point so that a scene's last CSR row keeps its own end;
    in-range indices are shifted, out-of-range ones stay out of range.  -> (Map, point bases, keyframe bases)"""
    pb = np.cumsum([0] + [m.n_points + 1 for m in maps]); kb = np.cumsum([0] + [m.n_keyframes + 1 for m in maps])
    tb = lambda name: np.cumsum([0] + [len(getattr(m, name)) for m in maps])
    ob, qb, cb = tb("obs_kf"), tb("kf_points"), tb("kf_children")

    def shift(v, n, base):
        v = np.asarray(v, np.int64)
        return np.where((v >= 0) & (v < n), v + base, np.where(v < 0, -1, 1 << 30)).astype(np.int32)
    cat = np.concatenate
    pts = cat([cat([m.points, np.zeros(1, R.LOCAL_POINT_DTYPE)]) for m in maps])
    for i, m in enumerate(maps):
        pts["flags"][pb[i + 1] - 1] = 1
    offs = lambda name, base: cat([np.asarray(getattr(m, name), np.int64) + base[i] for i, m in enumerate(maps)] + [[base[-1]]])
    live = cat([cat([np.ones(m.n_keyframes, np.uint8) if m.kf_live is None else m.kf_live, np.zeros(1, np.uint8)]) for m in maps])
    order = cat([cat([shift(np.arange(m.n_keyframes) if m.kf_order is None else m.kf_order, m.n_keyframes, kb[i]), [kb[i + 1] - 1]])
                 for i, m in enumerate(maps)])
    M = R.Map(pts, offs("obs_offsets", ob), cat([shift(m.obs_kf, m.n_keyframes, kb[i]) for i, m in enumerate(maps)]),
              offs("kf_point_offsets", qb), cat([shift(m.kf_points, m.n_points, pb[i]) for i, m in enumerate(maps)]),
              cat([cat([shift(m.kf_neigh, m.n_keyframes, kb[i]), np.full((1, 10), -1, np.int32)]) for i, m in enumerate(maps)]),
              offs("kf_child_offsets", cb), cat([shift(m.kf_children, m.n_keyframes, kb[i]) for i, m in enumerate(maps)]),
              cat([cat([shift(m.kf_parent, m.n_keyframes, kb[i]), [-1]]) for i, m in enumerate(maps)]), live, order)
    return M, pb, kb, shift


def test_all_scenes_one_batch_shuffled_and_rerun(tracker):
    M, pb, kb, shift = merge_maps([s["map"] for s in SCENES])
    rng = np.random.default_rng(3)
    pick = rng.permutation(len(SCENES)).tolist()
    pick.insert(5, pick[-1])                                                     # one scene twice
    max_lk, max_pts = 96, 300
    inp = []
    for i in pick:
        s = SCENES[i]
        row = np.full(max_lk, -3, np.int32); n = min(len(s["prev_row"]), max_lk)
        row[:n] = shift(s["prev_row"][:n], s["map"].n_keyframes, kb[i])
        inp.append((shift(s["frame_points"], s["map"].n_points, pb[i]), row, s["prev_n"], s["prev_ref"]))
    want = expect(M, inp, max_pts)
    # the merged map keeps what every scene is about: the scene's own list, shifted
    for (i, w) in zip(pick, want):
        ex = SCENES[i]["expect"]
        if not ex["early"] and len(SCENES[i]["prev_row"]) == max_lk:
            assert w["local_kf"][:len(ex["list"])].tolist() == [k + kb[i] for k in ex["list"]], SCENES[i]["name"]
    view = to_view(M)
    args = ([a[0] for a in inp], [a[1] for a in inp], [a[2] for a in inp], [a[3] for a in inp], max_pts)
    got, _ = run_device(tracker, M, *args, view=view)
    assert_same(got, want, "batch")
    again, _ = run_device(tracker, M, *args, view=view)
    assert_same(again, got, "second run")


def size_case(name):
    """maps on both sides of what the kernels switch on; -> (Map, frame_points, max_lk, max_pts, a check that the path is taken)"""
    from iv_slam_amd.track import local_map_lds_keyframes
    LDS = local_map_lds_keyframes()                                               # the kernel's own switch, read from the library
    fp = np.full(NF, -1, np.int32)
    if name in ("vote_row_lds_last", "vote_row_scratch_first"):
        n_kf = LDS if name == "vote_row_lds_last" else LDS + 1
        M = SC.base(n_kf=n_kf, neigh={n_kf - 1: [5]}, order=list(range(n_kf))[::-1])
        fp[:3] = [3 * (n_kf - 1), 3 * (n_kf - 1) + 1, 9]                         # the last keyframe of the row, twice, and keyframe 3
        return M, fp, 96, 70, lambda st: (n_kf > LDS) == (name == "vote_row_scratch_first") and st["list"] == [n_kf - 1, 3, 5]
    if name == "voted_beyond_one_compaction_chunk":                              # 300 voted keyframes: two chunks of 256, no expansion
        M = SC.base(n_kf=400, obs={0: list(range(50, 350))}, neigh={50: [1]})
        fp[:2] = [0, 152]
        return M, fp, 320, 1999, lambda st: len(st["list"]) == 300 and st["list"][0] == 50
    if name == "row_cut_below_voted":                                            # the row holds 70 of 300, the points 64 + 6 of its 210
        M = SC.base(n_kf=400, obs={0: list(range(50, 350))})
        fp[:1] = [0]
        return M, fp, 70, 70, lambda st: len(st["list"]) == 300 and sum(c == R.CUT_BY_CAP for _, _, c in st["points"]) == 140
    if name == "keyframe_rows_of_nf_and_more":                                   # rows of 256 (one chunk, full) and 300 (read up to 256)
        nP = 700
        kfp = {0: list(range(0, 256)), 1: list(range(200, 500)), 2: [699, 0, 456]}
        M = R.make_map(nP, 3, obs={0: [0, 1, 2]}, kf_points=kfp, seed=5)
        fp[:1] = [0]
        return M, fp, 8, 600, lambda st: st["list"] == [0, 1, 2] and sum(c == R.KEPT for _, _, c in st["points"]) == 256 + 200 + 2
    if name == "children_beyond_one_ballot":                                     # the first eligible child is the 67th
        M = SC.base(n_kf=100, children={0: list(range(10, 80))}, bad_keyframes=list(range(10, 76)))
        fp[:1] = [0]
        return M, fp, 96, 65, lambda st: st["list"] == [0, 76]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["vote_row_lds_last", "vote_row_scratch_first", "voted_beyond_one_compaction_chunk", "row_cut_below_voted",
                                  "keyframe_rows_of_nf_and_more", "children_beyond_one_ballot"])
def test_size_paths(tracker, name):
    M, fp, max_lk, max_pts, taken = size_case(name)
    row = np.full(max_lk, -3, np.int32)
    st = {}
    want = R.update_local_map(M, fp, row, 0, -7, NF, max_pts, stages=st)
    assert taken(st), "the case does not reach the path it is named after"
    got, _ = run_device(tracker, M, [fp, fp], [row, row], [0, 0], [-7, -7], max_pts)
    assert_same(got, [want, want], name)


def test_hostile_tables_return_ok(tracker):
    from iv_slam_amd import _lib
    for sc in SCENES:
        if sc["name"].startswith("hostile"):
            got, d = run_device(tracker, sc["map"], [sc["frame_points"]], [sc["prev_row"]], [sc["prev_n"]], [sc["prev_ref"]], sc["max_pts"])
            v = d["view"]
            rc = tracker._lib.ivf_tracker_update_local_map(tracker._h, C.byref(v.c), d["fp"].data_ptr(), 1, len(sc["prev_row"]), sc["max_pts"], d["lk"].data_ptr(),
                                                           d["nlk"].data_ptr(), d["ref"].data_ptr(), d["pts"].data_ptr(), d["ids"].data_ptr(),
                                                           d["off"].data_ptr(), d["npts"].data_ptr(), d["occ"].data_ptr(), None)
            assert rc == _lib.IVF_OK


def test_argument_errors(tracker):
    import torch
    from iv_slam_amd import _lib
    sc = SCENES[1]
    _, d = run_device(tracker, sc["map"], [sc["frame_points"]], [sc["prev_row"]], [sc["prev_n"]], [sc["prev_ref"]], sc["max_pts"])
    names = ("fp", "lk", "nlk", "ref", "pts", "ids", "off", "npts", "occ")

    def call(n=1, lk=96, mp=64, view=d["view"].c, null=None):
        p = {k: (None if k == null else d[k].data_ptr()) for k in names}
        return tracker._lib.ivf_tracker_update_local_map(tracker._h, C.byref(view), p["fp"], n, lk, mp, p["lk"], p["nlk"], p["ref"], p["pts"], p["ids"],
                                                         p["off"], p["npts"], p["occ"], None)
    assert call() == _lib.IVF_OK
    for k in names:
        assert call(null=k) == _lib.IVF_E_INVALID, k
    assert call(n=65) == _lib.IVF_E_INVALID and call(n=-1) == _lib.IVF_E_INVALID and call(lk=0) == _lib.IVF_E_INVALID and call(mp=0) == _lib.IVF_E_INVALID
    assert call(n=0) == _lib.IVF_OK
    big = torch.zeros((65, NF), dtype=torch.int32, device="cuda:0")
    with pytest.raises(_lib.IvfError):
        tracker.merge_local(torch.zeros((65, 4), dtype=torch.int32, device="cuda:0"), torch.zeros(66, dtype=torch.int32, device="cuda:0"), big, big)
    torch.cuda.synchronize()


def test_chain_with_search_local_and_the_tail(iv):
    """update_local_map -> search_local equals search_local fed with the restatement's list packed on the host; then merge_local ->
    points_from_map -> optimize_pose -> close_local_map against the restated tail"""
    import torch
    from iv_slam_amd import dist as ivd
    cam, recs, _, _ = extracted_sequence(iv, 640, 240, NF, 4, seed=311)
    rng = np.random.default_rng(12)
    I = np.eye(4, dtype=F)
    # the map: keyframe s holds the stereo points of record s; a point is observed by its keyframe (and the next one now and then)
    per_kf = [map_points_from(cam, recs[s], I, rng) for s in range(3)]
    pts, off = pack_points(iv, per_kf)
    nP, nK = int(off[-1]), 3
    pts["flags"] &= ~1
    pts["flags"][rng.random(nP) < 0.04] |= 1
    obs = {m: [k] + ([(k + 1) % nK] if rng.random() < 0.3 else []) for k in range(nK) for m in range(off[k], off[k + 1])}
    kfp = {k: list(range(off[k], off[k + 1]))[:NF] for k in range(nK)}
    M = R.make_map(nP, nK, obs=obs, kf_points=kfp, neigh={0: [1], 2: [1]}, children={0: [2]}, parent={1: 0})
    M.points[:] = pts[:nP]
    frames = [1, 2, 3, 0]
    fps = []
    for f in frames:                                                             # what the first search left: a few points of one keyframe
        fp = np.full(NF, -1, np.int32)
        k = f % nK
        nC = len(recs[f]["kps"])
        take = rng.choice(np.arange(off[k], off[k + 1]), 25, replace=False)
        fp[rng.choice(nC, 25, replace=False)] = take
        fps.append(fp)
    fps[3][:] = -1                                                               # a frame that holds nothing: the previous list
    max_lk, max_pts = 8, 250
    rows = [np.full(max_lk, -3, np.int32) for _ in frames]; rows[3][:2] = [2, 0]
    prev_n = [0, 0, 0, 2]
    want = [R.update_local_map(M, fp, row, n, -7, NF, max_pts) for fp, row, n in zip(fps, rows, prev_n)]
    assert all(w["n_local_points"] > 100 for w in want)
    dev = torch.device("cuda:0")
    tr = iv.BatchTracker(NF, cam["scale"], float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam["bf"]), cam["bounds"],
                         max_pairs=len(frames), b=float(cam["b"]))
    got, d = run_device(tr, M, fps, rows, prev_n, [-7] * 4, max_pts)
    assert_same(got, want, "chain")
    block = torch.from_numpy(ivd.pack_records(recs, NF).reshape(-1)).to(dev)
    dfr = torch.tensor(frames, dtype=torch.int32, device=dev)

    def search(points, offsets, occupied):
        a = torch.full((4, NF), MARK, dtype=torch.int32, device=dev); nm = torch.full((4,), MARK, dtype=torch.int32, device=dev)
        tr.search_local(block, dfr, points, offsets, max_pts, a, nm, occupied=occupied, th=3.0, nn_ratio=0.8)
        torch.cuda.synchronize()
        return a, nm
    a_dev, nm_dev = search(d["pts"], d["off"], d["occ"])
    h_pts = torch.from_numpy(np.stack([w["points"] for w in want]).view(np.uint8).reshape(-1)).to(dev)
    h_off = torch.tensor([f * max_pts for f in range(5)], dtype=torch.int32, device=dev)
    h_occ = torch.from_numpy(np.stack([w["occupied"] for w in want])).to(dev)
    a_host, nm_host = search(h_pts, h_off, h_occ)
    assert torch.equal(a_dev, a_host) and torch.equal(nm_dev, nm_host)
    assert int(nm_dev.sum()) > 100, "the search must match something for the comparison to mean anything"
    # ---- the tail
    a_np = a_dev.cpu().numpy()
    tr.merge_local(d["ids"], d["off"], a_dev, d["fp"])
    pq = rng.uniform(0.2, 1.0, nP).astype(F)
    dpq = torch.from_numpy(pq).to(dev)
    xw = torch.full((4, NF, 3), 9.0, dtype=torch.float32, device=dev); has = torch.full((4, NF), 9, dtype=torch.uint8, device=dev)
    q = torch.full((4, NF), 9.0, dtype=torch.float32, device=dev)
    tr.points_from_map(d["view"], d["fp"], xw, has, quality=q, point_quality=dpq)
    poses = torch.from_numpy(np.tile(I[:3, :4].reshape(12), (4, 1)).astype(F)).to(dev)
    outl = torch.full((4, NF), 9, dtype=torch.uint8, device=dev); nin = torch.full((4,), MARK, dtype=torch.int32, device=dev)
    tr.optimize_pose(block, dfr, xw, has, poses, outl, nin, quality=q)
    torch.cuda.synchronize()
    merged = d["fp"].cpu().numpy().copy()
    outl = outl | torch.from_numpy((rng.random((4, NF)) < 0.2).astype(np.uint8)).to(dev)     # and some more, whatever the solver found
    o_np = outl.cpu().numpy()
    for f in range(4):
        m = R.merge_local(want[f]["frame_points"], want[f]["point_ids"], a_np[f])
        assert merged[f].tobytes() == m.tobytes(), "merge_local frame %d" % f
        rx, rh, rq = R.points_from_map(M, m, pq)
        assert xw[f].cpu().numpy().tobytes() == rx.tobytes() and has[f].cpu().numpy().tobytes() == rh.tobytes() and q[f].cpu().numpy().tobytes() == rq.tobytes()
    for only_tracking, stereo in ((False, False), (True, False), (False, True)):
        fpc = torch.from_numpy(merged).to(dev); n2 = torch.full((4,), MARK, dtype=torch.int32, device=dev)
        tr.close_local_map(d["view"], outl, fpc, n2, only_tracking=only_tracking, stereo=stereo)
        torch.cuda.synchronize()
        for f in range(4):
            n, fp2 = R.close_local_map(M, merged[f], o_np[f], only_tracking, stereo)
            assert int(n2[f]) == n and fpc[f].cpu().numpy().tobytes() == fp2.tobytes(), (only_tracking, stereo, f)
