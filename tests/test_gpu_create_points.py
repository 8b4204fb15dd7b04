"""ivf_tracker_create_map_points (iv_slam_amd/csrc/ivf_track_create.hip) against tests/create_points_ref.py, the restatement of
LocalMapping::CreateNewMapPoints (ORB/src/LocalMapping.cc:273-525), on the hand-made scenes of tests/create_points_scenes.py at 64
features.  Bar: every output array, diagnostics included, byte for byte, on outputs pre-filled with marks; each scene alone and all scenes
of equal parameters stacked into one call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_gpu_track import iv  # noqa: F401  (the module fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import create_points_ref as R          # noqa: E402
import create_points_scenes as SC      # noqa: E402
import local_map_ref as LM             # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
NF = SC.NF
SCENES = SC.all_scenes()
MARK = -77


@pytest.fixture(scope="module")
def tracker(iv):
    c = SC.CAM
    return iv.BatchTracker(NF, c["scale"], float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), float(c["bf"]), c["bounds"], max_pairs=64,
                           b=float(c["b"]))


@pytest.fixture(scope="module")
def vocabulary(iv):
    t = SC.TREE
    return iv.ORBVocabulary(t["child_start"], t["child"], t["desc"], t["word"], t["weight"], t["depth"])


def run_device(iv, tr, voc, scenes, diagnostics=True):
    """one call with one keyframe slot per scene (all of one max_neigh, all with or all without F12 / key qualities / kf_order): the scenes'
    records side by side, indices shifted -> list of output dicts shaped like the restatement's"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base = np.cumsum([0] + [len(s["records"]) for s in scenes])
    n_rec, n, mn = int(base[-1]), len(scenes), len(scenes[0]["neigh"])
    shift = lambda v, b, m: v + b if 0 <= v < m else (-1 if v < 0 else n_rec + 5)
    recs = [r for s in scenes for r in s["records"]]
    kf = np.array([shift(s["kf"], base[i], len(s["records"])) for i, s in enumerate(scenes)], np.int32)
    neigh = np.array([[shift(v, base[i], len(s["records"])) for v in s["neigh"]] for i, s in enumerate(scenes)], np.int32)
    opt = lambda key, f: None if scenes[0][key] is None else up(f())
    d = dict(block=up(ivd.pack_records(recs, NF).reshape(-1)), kf=up(kf), neigh=up(neigh), poses=up(np.concatenate([s["poses"].reshape(-1, 12) for s in scenes])),
             has=up(np.concatenate([s["has_point"] for s in scenes])),
             kq=opt("key_quality", lambda: np.concatenate([s["key_quality"] for s in scenes])),
             F12=opt("F12", lambda: np.stack([s["F12"] for s in scenes])),
             order=opt("kf_order", lambda: np.concatenate([s["kf_order"] + base[i] for i, s in enumerate(scenes)]).astype(np.int32)),
             pts=torch.full((n * NF * 80,), 0xAB, dtype=torch.uint8, device=dev), nn=torch.full((n, NF), MARK, dtype=torch.int32, device=dev),
             i2=torch.full((n, NF), MARK, dtype=torch.int32, device=dev), od=torch.full((n, NF), MARK, dtype=torch.int32, device=dev),
             q=torch.full((n, NF), 9.0, dtype=torch.float32, device=dev), nnew=torch.full((n,), MARK, dtype=torch.int32, device=dev),
             m=torch.full((n, mn, NF), MARK, dtype=torch.int32, device=dev) if diagnostics else None,
             st=torch.full((n, mn, NF), 0xAB, dtype=torch.uint8, device=dev) if diagnostics else None)
    tr.create_map_points(voc, d["block"], d["kf"], d["neigh"], d["poses"], d["has"], d["pts"], d["nn"], d["i2"], d["od"], d["q"], d["nnew"],
                         levelsup=SC.LEVELSUP, key_quality=d["kq"], F12=d["F12"], kf_order=d["order"], matches=d["m"], stage=d["st"])
    torch.cuda.synchronize()
    pts = d["pts"].cpu().numpy().view(R.LOCAL_POINT_DTYPE).reshape(n, NF)
    h = {k: d[k].cpu().numpy() for k in ("nn", "i2", "od", "q", "nnew") + (("m", "st") if diagnostics else ())}
    outs = [dict(new_point=pts[k], new_neigh=h["nn"][k], new_idx2=h["i2"][k], new_order=h["od"][k], new_quality=h["q"][k], n_new=h["nnew"][k],
                 matches=h["m"][k] if diagnostics else None, stage=h["st"][k] if diagnostics else None) for k in range(n)]
    return outs, d


def assert_same(got, want, what, diagnostics=True):
    for k, (g, w) in enumerate(zip(got, want)):
        if not diagnostics:
            g = dict(g, matches=w["matches"], stage=w["stage"])
        key = R.same(w, g)
        assert key is None, "%s slot %d: %s differs: device %r, restatement %r" % (what, k, key, np.asarray(g[key]).reshape(-1)[:16], np.asarray(w[key]).reshape(-1)[:16])


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scene_alone(iv, tracker, vocabulary, sc):
    want = SC.run_ref(sc)
    got, _ = run_device(iv, tracker, vocabulary, [sc])
    assert_same(got, [want], sc["name"])
    for (rank, idx1), code in sc["expect"].items():
        if code is not None:
            assert got[0]["stage"][rank, idx1] == code, (sc["name"], rank, idx1)


def test_scenes_of_equal_parameters_in_one_batch_and_rerun(iv, tracker, vocabulary):
    groups = {}
    for sc in SCENES:
        groups.setdefault((len(sc["neigh"]), sc["F12"] is None, sc["key_quality"] is None, sc["kf_order"] is None), []).append(sc)
    assert max(len(g) for g in groups.values()) >= 3
    for key, g in groups.items():
        want = [SC.run_ref(sc) for sc in g]
        got, _ = run_device(iv, tracker, vocabulary, g)
        assert_same(got, want, "batch %r" % (key,))
        again, _ = run_device(iv, tracker, vocabulary, g, diagnostics=False)
        assert_same(again, want, "second run, no diagnostics %r" % (key,), diagnostics=False)


def test_argument_errors(iv, tracker, vocabulary):
    from iv_slam_amd import _lib
    sc = SCENES[2]
    _, d = run_device(iv, tracker, vocabulary, [sc])
    names = ("block", "kf", "neigh", "poses", "has", "pts", "nn", "i2", "od", "q", "nnew")

    def call(n_kf=1, mn=1, null=None, levelsup=1):
        p = {k: (None if k == null else d[k].data_ptr()) for k in names}
        return tracker._lib.ivf_tracker_create_map_points(tracker._h, vocabulary._h, levelsup, p["block"], tracker.record_bytes, len(sc["records"]), p["kf"],
                                                          n_kf, p["neigh"], mn, p["poses"], p["has"], None, None, None, p["pts"], p["nn"], p["i2"], p["od"],
                                                          p["q"], p["nnew"], None, None, None)
    assert call() == _lib.IVF_OK
    for k in names:
        assert call(null=k) == _lib.IVF_E_INVALID, k
    assert call(n_kf=65) == _lib.IVF_E_CAPACITY and call(n_kf=7, mn=10) == _lib.IVF_E_CAPACITY
    assert call(mn=0) == _lib.IVF_E_INVALID and call(n_kf=-1) == _lib.IVF_E_INVALID and call(levelsup=-1) == _lib.IVF_E_INVALID
    assert call(n_kf=0) == _lib.IVF_OK
    import torch
    torch.cuda.synchronize()


def test_chain_new_points_reach_the_next_search(iv, tracker, vocabulary):
    """the new records appended to a map -> update_local_map -> search_local: a frame that is the keyframe's own record, at its pose, holding two
    of the new points, finds the others on the keypoints they were made from"""
    import torch
    from iv_slam_amd import dist as ivd
    from iv_slam_amd.track import MapView
    sc = [s for s in SCENES if s["name"] == "stereo_forward"][0]
    got, d = run_device(iv, tracker, vocabulary, [sc])
    o = got[0]
    n_new = int(o["n_new"])
    assert n_new >= 6
    by_order = np.argsort(np.where(o["new_order"] >= 0, o["new_order"], 1 << 20))[:n_new]          # idx1 in creation order
    pts = o["new_point"][by_order].copy()                                                           # the caller appends the records in that order
    kfp = {0: [-1] * NF, 1: [-1] * NF}
    for p, i1 in enumerate(by_order):
        kfp[0][i1] = p; kfp[1][int(o["new_idx2"][i1])] = p                                           # AddMapPoint on both keyframes; the last on a shared idx2 stays
    M = LM.make_map(n_new, 2, obs={p: [0, 1] for p in range(n_new)}, kf_points=kfp)
    M.points[:] = pts
    dev = torch.device("cuda:0")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    view = MapView(up(M.points.view(np.uint8).reshape(-1)), up(M.obs_offsets), up(M.obs_kf), up(M.kf_point_offsets), up(M.kf_points), up(M.kf_neigh),
                   up(M.kf_child_offsets), up(M.kf_children), up(M.kf_parent), kf_live=up(M.kf_live), kf_order=up(M.kf_order))
    fp = np.full((1, NF), -1, np.int32)
    held = [int(by_order[0]), int(by_order[1])]
    fp[0, held[0]] = 0; fp[0, held[1]] = 1
    max_lk, max_pts = 8, 32
    t = dict(fp=up(fp), lk=torch.full((1, max_lk), -3, dtype=torch.int32, device=dev), nlk=torch.zeros(1, dtype=torch.int32, device=dev),
             ref=torch.full((1,), -7, dtype=torch.int32, device=dev), pts=torch.zeros(max_pts * 80, dtype=torch.uint8, device=dev),
             ids=torch.full((1, max_pts), MARK, dtype=torch.int32, device=dev), off=torch.zeros(2, dtype=torch.int32, device=dev),
             npts=torch.zeros(1, dtype=torch.int32, device=dev), occ=torch.zeros((1, NF), dtype=torch.uint8, device=dev))
    tracker.update_local_map(view, t["fp"], t["lk"], t["nlk"], t["ref"], t["pts"], t["ids"], t["off"], t["npts"], t["occ"])
    assign = torch.full((1, NF), MARK, dtype=torch.int32, device=dev); nm = torch.full((1,), MARK, dtype=torch.int32, device=dev)
    frames = torch.zeros(1, dtype=torch.int32, device=dev)
    tracker.search_local(d["block"], frames, t["pts"], t["off"], max_pts, assign, nm, poses=up(sc["poses"][0].reshape(1, 12)), occupied=t["occ"], th=1.0,
                         nn_ratio=0.8)
    torch.cuda.synchronize()
    assert int(t["npts"][0]) == n_new, "every new point is a local point of the frame"
    ids = t["ids"].cpu().numpy()[0]; a = assign.cpu().numpy()[0]
    found = {i: int(ids[a[i]]) for i in range(NF) if a[i] >= 0}
    assert all(int(by_order[p]) == i for i, p in found.items()), "a point comes back on the keypoint it was made from"
    assert not set(found) & set(held) and len(found) >= (n_new - 2) // 2, found
