"""The yardstick of ivf_tracker_update_local_map checked on its own (no GPU): tests/local_map_ref.py, the plain-Python restatement of
Tracking::UpdateLocalMap (ORB/src/Tracking.cc:2134-2270) and of the tail of TrackLocalMap (:1648-1677), on the hand-made maps of
tests/local_map_scenes.py.  Every scene states what the reference must do; a second, array-only statement must agree with the literal
one on random maps; every injected mistake must show on some scene; and the new entry points answer their argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import local_map_ref as R          # noqa: E402
import local_map_scenes as SC      # noqa: E402

SCENES = SC.all_scenes()


def run(sc, faults=frozenset(), stages=None):
    return R.update_local_map(sc["map"], sc["frame_points"], sc["prev_row"], sc["prev_n"], sc["prev_ref"], SC.NF, sc["max_pts"], faults, stages)


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scene_stage_codes(sc):
    st = {}
    out = run(sc, stages=st)
    ex = sc["expect"]
    max_lk = len(sc["prev_row"])
    assert st["early"] == ex["early"]
    assert st["list"] == ex["list"], "the local keyframes"
    if ex["early"]:
        assert out["local_kf"].tobytes() == sc["prev_row"].tobytes() and out["n_local_kf"] == min(max(sc["prev_n"], 0), max_lk)
    else:
        assert out["n_local_kf"] == len(ex["list"]), "the true count"
        want = (ex["list"] + [-1] * max_lk)[:max_lk]
        assert out["local_kf"].tolist() == want
    assert out["ref_kf"] == (SC.PREV_REF if ex["ref"] is None else ex["ref"])
    for k, codes in ex.get("stages", {}).items():
        assert st["keyframes"].get(k) == codes, "keyframe %d" % k
    for k in ex.get("absent", ()):
        assert k not in st["list"]
    if "stops" in ex:
        assert st["stops"] == ex["stops"]
    if "ids" in ex:
        assert out["n_local_points"] == len(ex["ids"]), "the true count"
        assert out["point_ids"].tolist() == (ex["ids"] + [-1] * sc["max_pts"])[:sc["max_pts"]]
    if "points" in ex:
        assert st["points"] == ex["points"]
    for m in ex.get("nulled", ()):
        assert m in sc["frame_points"] and m not in out["frame_points"]
    n = min(int(out["n_local_points"]), sc["max_pts"])
    ids, fl = out["point_ids"][:n], out["points"]["flags"][:n]
    M = sc["map"]
    held = set(int(m) for m in out["frame_points"] if 0 <= m < M.n_points)
    for m, f in zip(ids, fl):
        assert (f & 1) == (1 if m in held else 0) and (f & 2) == (M.points["flags"][m] & 2)
        assert not M.bad(m)
    for m in ex.get("held_listed", ()):
        assert fl[list(ids).index(m)] & 1
    for m in ex.get("bit1_clear", ()):
        assert not fl[list(ids).index(m)] & 2
    assert (out["points"]["flags"][n:] == 1).all() and (out["point_ids"][n:] == -1).all(), "padding"
    assert len(set(ids.tolist())) == n, "every point once"


def random_map(seed):
    rng = np.random.default_rng(seed)
    nK, nP, nf = int(rng.integers(1, 40)), int(rng.integers(1, 120)), 32
    obs = {m: rng.choice(nK, rng.integers(0, min(nK, 4) + 1), replace=False).tolist() for m in range(nP)}
    kfp = {k: rng.integers(-1, nP, rng.integers(0, nf + 6)).tolist() for k in range(nK)}
    neigh = {k: rng.integers(-1, nK, rng.integers(0, 11)).tolist() for k in range(nK)}
    children = {k: rng.integers(0, nK, rng.integers(0, 4)).tolist() for k in range(nK)}
    parent = {k: int(rng.integers(-1, nK)) for k in range(nK)}
    order = rng.permutation(nK).tolist() if seed % 2 else None
    M = R.make_map(nP, nK, obs=obs, kf_points=kfp, neigh=neigh, children=children, parent=parent,
                   bad_points=np.flatnonzero(rng.random(nP) < 0.15), no_obs_points=np.flatnonzero(rng.random(nP) < 0.2),
                   bad_keyframes=np.flatnonzero(rng.random(nK) < 0.2), order=order, seed=seed)
    if seed % 5 == 0:                                                             # some hostile entries
        for tab, hi in ((M.obs_kf, nK), (M.kf_points, nP), (M.kf_children, nK)):
            if len(tab):
                tab[rng.integers(0, len(tab))] = hi + int(rng.integers(0, 3))
        M.kf_point_offsets[rng.integers(0, nK + 1)] = int(rng.integers(-2, len(M.kf_points) + 3))
    fp = np.full(nf, -1, np.int32)
    n_held = int(rng.integers(0, nf)) if seed % 7 else 0
    fp[:n_held] = rng.integers(-1, nP, n_held)
    max_lk = int(rng.integers(1, 12)) if seed % 3 == 0 else 96
    prev = rng.integers(-1, nK + 1, max_lk).astype(np.int32)
    return M, fp, prev, int(rng.integers(-1, max_lk + 3)), nf, int(rng.integers(1, 60))


def test_array_statement_equals_the_literal_one_on_random_maps():
    early = capped = 0
    for seed in range(300):
        M, fp, prev, prev_n, nf, max_pts = random_map(seed)
        st = {}
        a = R.update_local_map(M, fp, prev, prev_n, -7, nf, max_pts, stages=st)
        b = R.update_local_map_arrays(M, fp, prev, prev_n, -7, nf, max_pts)
        assert R.same(a, b) is None, "seed %d: %s differs" % (seed, R.same(a, b))
        early += st["early"]; capped += int(a["n_local_points"]) > max_pts
    assert early > 10 and capped > 10 and early < 250, "the random maps must reach both returns and the cap"


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_fault_changes_a_scene(fault):
    hit = [sc["name"] for sc in SCENES if R.same(run(sc), run(sc, frozenset([fault]))) is not None]
    assert hit, "no scene notices the fault %r" % fault


def test_tail_restatement_known_answers():
    M = SC.base(no_obs_points=[4])
    fp = np.array([0, -1, 4, 7, 99], np.int32)
    ids = np.array([10, 11, 12, -1], np.int32)
    assert R.merge_local(fp, ids[:3], [2, -1, 0, -1, 1]).tolist() == [12, -1, 10, 7, 11]
    xw, has, q = R.points_from_map(M, fp, np.arange(36, dtype=np.float32) / 36)
    assert has.tolist() == [1, 0, 1, 1, 0] and (xw[2] == M.points["pos"][4]).all() and (xw[1] == 0).all() and q[3] == np.float32(7 / 36) and q[4] == 1
    out = np.array([0, 0, 0, 1, 1], np.uint8)
    assert R.close_local_map(M, fp, out, only_tracking=False, stereo=True)[0] == 1          # point 4 has no observations
    n, fp2 = R.close_local_map(M, fp, out, only_tracking=True, stereo=True)
    assert n == 2 and fp2.tolist() == [0, -1, 4, -1, 99]
    assert R.close_local_map(M, fp, out, only_tracking=True, stereo=False)[1].tolist() == fp.tolist()


def test_entry_points_exist_and_check_arguments_without_gpu():
    from iv_slam_amd import _lib
    from iv_slam_amd.track import BatchTracker, MapView
    for name in ("update_local_map", "merge_local", "points_from_map", "close_local_map"):
        assert callable(getattr(BatchTracker, name))
    lib = _lib.load()
    buf = np.zeros(256, np.uint8)
    p = _lib.ptr(buf)
    one = C.c_void_p(16)                                                          # a non-null handle that must not be touched
    view = _lib.MapViewC()
    for f, _ in _lib.MapViewC._fields_[:11]:
        setattr(view, f, p.value if hasattr(p, "value") else p)
    good = dict(t=one, m=C.byref(view), fp=p, n=1, lk=4, mp=4, a=p, b=p, c=p, d=p, e=p, f=p, g=p, h=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ivf_tracker_update_local_map(a["t"], a["m"], a["fp"], a["n"], a["lk"], a["mp"], a["a"], a["b"], a["c"], a["d"], a["e"], a["f"],
                                                a["g"], a["h"], None)
    for kw in [dict(t=None), dict(m=None), dict(fp=None), dict(lk=0), dict(mp=0)] + [{k: None} for k in "abcdefgh"]:
        assert call(**kw) == _lib.IVF_E_INVALID, kw
    assert b"max_points_per_frame" in (call(mp=0), lib.ivf_last_error())[1]
    neg = _lib.MapViewC.from_buffer_copy(view); neg.n_obs = -1
    assert call(m=C.byref(neg)) == _lib.IVF_E_INVALID
    nul = _lib.MapViewC.from_buffer_copy(view); nul.kf_parent = None; nul.n_keyframes = 1
    assert call(m=C.byref(nul)) == _lib.IVF_E_INVALID
    assert lib.ivf_tracker_merge_local(None, p, p, p, 1, p, None) == _lib.IVF_E_INVALID
    assert lib.ivf_tracker_merge_local(one, p, p, p, 1, None, None) == _lib.IVF_E_INVALID
    assert lib.ivf_tracker_points_from_map(one, p, 4, None, None, 1, p, p, None, None) == _lib.IVF_E_INVALID
    assert lib.ivf_tracker_points_from_map(one, p, -1, None, p, 1, p, p, None, None) == _lib.IVF_E_INVALID
    assert lib.ivf_tracker_close_local_map(one, p, 4, None, 1, 0, 1, p, p, None) == _lib.IVF_E_INVALID
    assert lib.ivf_tracker_close_local_map(one, None, 4, p, 1, 0, 1, p, p, None) == _lib.IVF_E_INVALID
    # MapView refuses tables that do not fit together before anything reaches the library
    import torch
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    pts = torch.zeros(2 * 80, dtype=torch.uint8)
    ok = dict(points=pts, obs_offsets=i32(0, 1, 2), obs_kf=i32(0, 0), kf_point_offsets=i32(0, 2), kf_points=i32(0, 1),
              kf_neigh=torch.full((1, 10), -1, dtype=torch.int32), kf_child_offsets=i32(0, 0), kf_children=i32(), kf_parent=i32(-1))
    v = MapView(**ok)
    assert (v.c.n_points, v.c.n_keyframes, v.c.n_obs, v.c.n_kf_points, v.c.n_children) == (2, 1, 2, 2, 0)
    for bad in (dict(points=pts[:80]), dict(kf_neigh=torch.full((1, 9), -1, dtype=torch.int32)), dict(kf_order=i32(0, 0)),
                dict(obs_kf=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(AssertionError):
            MapView(**dict(ok, **bad))
