"""ivf_tracker_solve_sim3 (iv_slam_amd/csrc/ivf_sim3.hip) -- Sim3Solver (ORB/src/Sim3Solver.cc) as LoopClosing::ComputeSim3 runs it, batched
on the device -- against tests/sim3_ref.py, the numpy restatement, on the hand-made scenes of tests/sim3_scenes.py, through
BatchTracker.solve_sim3.

A 3-point Horn hypothesis has one closed-form answer, so every iteration is compared: ninliers, the inlier flags, iterations, the state and
hyp_ninliers must be EQUAL to the restatement's on every scene, each alone and all scenes that share their parameters in one call; sim3 and
hyp_sim3 must agree within 8 x the spread recorded in tests/golden/sim3_noise.json.  The margin: the device differs from the restatement
only in libm (atan2, sin, cos) and in product contraction; the recorded spread is what separates two f64 eigen-solvers on the same float
input, a difference of the same kind and far larger, and a power of two covers it.  The integer results can be equal because
tests/test_sim3_cpu.py keeps every err of every scene further from its bound than 64 x that spread.

A scene with several calls is run call after call through the state array (a resumed call equals the reference's continued iterate); in a
shared call the scenes that have no further call are left out through the select mask, which must leave them untouched."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ref as R
import sim3_scenes as S
from test_gpu_track import iv  # noqa: F401  (the module fixture)
from test_sim3_cpu import SCENES, ref_runs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NOISE = json.load(open(os.path.join(ROOT, "tests", "golden", "sim3_noise.json")))
TOL = 8 * NOISE["spread"]
SIM_FILL, FLAG_FILL, INT_FILL = 7.0, 9, -7
NF = S.NF
WORST = [0.0]                                                                 # the largest |device - restatement| over sim3 and hyp_sim3 seen


def make_tracker(iv, max_pairs):
    c = S.CAM
    return iv.BatchTracker(NF, S.SCALE, float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), float(c["bf"]), S.BOUNDS, max_pairs=max_pairs)


def params_key(sc):
    return tuple(sorted(sc["params"].items()))


def run_calls(iv, names, tracker=None, stream=False, hyp=True, order=None, with_state=None):
    """the scenes `names` (equal parameters) in ONE call per round of their calls -> {name: [dict of device results as numpy per call]}"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    scs = [SCENES[n] for n in names]
    order = list(range(len(scs))) if order is None else list(order)
    scs = [scs[k] for k in order]
    p = scs[0]["params"]
    assert all(params_key(s) == params_key(scs[0]) for s in scs)
    n = len(scs); mi = p["max_iterations"]
    recs = []; pairs = []
    poses = np.zeros((2 * n, 12), F); xw = np.zeros((2 * n, NF, 3), F); flags = np.zeros((2 * n, NF), np.uint8)
    m12 = np.full((n, NF), -1, np.int32); draws = np.zeros((n, mi, 3), np.uint32)
    for j, sc in enumerate(scs):
        for side, kf in enumerate((sc["kf1"], sc["kf2"])):
            r = 2 * j + side
            recs.append(dict(kps=kf["kps"], desc=kf["desc"], uright=kf["uright"], depth=kf["depth"]))
            poses[r] = kf["pose"]; xw[r, :kf["n"]] = kf["xw"]; flags[r, :kf["n"]] = kf["flags"]
            flags[r, kf["n"]:] = 1; xw[r, kf["n"]:] = (0.0, 0.0, 10.0)        # a live point on the slots past the count: never collected
        pairs.append((2 * j, 2 * n + 5 if sc["bad"] else 2 * j + 1))
        m12[j] = sc["match12"]; draws[j] = sc["draws"]
    block = torch.from_numpy(ivd.pack_records(recs, NF).reshape(-1)).to(dev)
    tr = tracker or make_tracker(iv, n)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dpairs, dposes, dxw, dflags, dm12 = up(np.array(pairs, np.int32)), up(poses), up(xw), up(flags), up(m12)
    ddraws = up(draws.view(np.int32))
    rounds = max(len(sc["calls"]) for sc in scs)
    use_state = any(c["state"] is not None for sc in scs for c in sc["calls"]) if with_state is None else with_state
    state = np.zeros((n, 2), np.int32)
    out = {sc["name"]: [] for sc in scs}
    st = torch.cuda.Stream() if stream else None
    for k in range(rounds):
        sel = np.array([int(sc["select"] and k < len(sc["calls"])) for sc in scs], np.int32)
        for j, sc in enumerate(scs):
            if k < len(sc["calls"]) and isinstance(sc["calls"][k]["state"], tuple):
                state[j] = sc["calls"][k]["state"]
        d = dict(sim3=torch.full((n, 16), SIM_FILL, dtype=torch.float32, device=dev), inlier=torch.full((n, NF), FLAG_FILL, dtype=torch.uint8, device=dev),
                 ninl=torch.full((n,), INT_FILL, dtype=torch.int32, device=dev), its=torch.full((n,), INT_FILL, dtype=torch.int32, device=dev),
                 hyp_sim3=torch.full((n, mi, 16), SIM_FILL, dtype=torch.float32, device=dev),
                 hyp_n=torch.full((n, mi), INT_FILL, dtype=torch.int32, device=dev), state=up(state))
        if st is not None:
            st.wait_stream(torch.cuda.current_stream())
        tr.solve_sim3(block, dpairs, dposes, dxw, dflags, dm12, ddraws, d["sim3"], d["inlier"], d["ninl"], max_iterations=mi,
                      probability=p["probability"], min_inliers=p["min_inliers"], fix_scale=p["fix_scale"], select=None if sel.all() else up(sel),
                      state=d["state"] if use_state else None, iterations=d["its"], hyp_sim3=d["hyp_sim3"] if hyp else None,
                      hyp_ninliers=d["hyp_n"] if hyp else None, stream_ptr=st.cuda_stream if st is not None else None)
        torch.cuda.synchronize()
        got = {key: v.cpu().numpy() for key, v in d.items()}
        state_in = state.copy()
        state = got["state"].copy()
        for j, sc in enumerate(scs):
            if k < len(sc["calls"]):
                out[sc["name"]].append(dict({key: v[j] for key, v in got.items()}, state_in=state_in[j], used_state=use_state, selected=bool(sel[j])))
            else:                                                            # left out of this round: nothing but ninliers = -2
                assert got["ninl"][j] == -2 and (got["inlier"][j] == FLAG_FILL).all() and (got["sim3"][j] == SIM_FILL).all()
                assert got["its"][j] == INT_FILL and (got["hyp_n"][j] == INT_FILL).all() and np.array_equal(got["state"][j], state_in[j])
    return out


def close(a, b, what):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "%s: NaN where the restatement has none, or the reverse" % what
    ok = ~np.isnan(a)
    d = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
    WORST[0] = max(WORST[0], d)
    assert d <= TOL, "%s: %.3g off the restatement (bound %.3g)" % (what, d, TOL)
    return d


def compare(sc, k, o, g, hyp=True):
    """device results g of call k of scene sc against the restatement's o"""
    tag = "%s call %d" % (sc["name"], k)
    untouched = np.full(16, SIM_FILL, F).tobytes()
    if o is None:
        assert g["ninl"] == (-1 if sc["bad"] else -2), tag
        assert (g["inlier"] == FLAG_FILL).all() and g["sim3"].tobytes() == untouched and g["its"] == INT_FILL and (g["hyp_n"] == INT_FILL).all(), tag
        assert np.array_equal(g["state"], g["state_in"]), tag
        return
    n1 = sc["kf1"]["n"]
    assert g["ninl"] == o["ninliers"], "%s: ninliers %d, the restatement %d" % (tag, g["ninl"], o["ninliers"])
    assert g["its"] == o["iterations"], "%s: iterations %d, the restatement %d" % (tag, g["its"], o["iterations"])
    if g["used_state"]:
        assert tuple(g["state"]) == tuple(o["state"]), "%s: state %r, the restatement %r" % (tag, g["state"], o["state"])
    assert np.array_equal(g["inlier"][:n1], o["inlier"]) and not g["inlier"][n1:].any(), "%s: inlier flags differ at %r" % (tag, np.nonzero(g["inlier"][:n1] != o["inlier"])[0][:8])
    ran = [info["it"] for info in o["info"]]
    if hyp:
        # the hypotheses are computed at once: every iteration from the state's to mRansacMaxIts is written, also those after the success
        first, infos = S.hypotheses_checked(sc, o)
        rest = np.delete(np.arange(sc["params"]["max_iterations"]), np.arange(first, max(first, o["max_its"])))
        assert (g["hyp_n"][rest] == INT_FILL).all() and (g["hyp_sim3"][rest] == SIM_FILL).all(), "%s: an iteration outside the call's range was written" % tag
        assert (g["hyp_n"][first:o["max_its"]] != INT_FILL).all(), "%s: an iteration of the call's range was not written" % tag
        for info in infos:
            it = info["it"]
            assert g["hyp_n"][it] == info["ninliers"], "%s iteration %d: %d inliers, the restatement %d" % (tag, it, g["hyp_n"][it], info["ninliers"])
            close(g["hyp_sim3"][it], R.sim3_16(info["R"], info["t"], info["s"]), "%s iteration %d" % (tag, it))
    if o["sim3"] is None:
        assert g["sim3"].tobytes() == untouched, "%s: no transform, but sim3 was written" % tag
    else:
        d = close(g["sim3"], o["sim3"], tag)
        if hyp:
            assert g["sim3"].tobytes() == g["hyp_sim3"][ran[-1]].tobytes(), "%s: the transform is not the winning iteration's" % tag
        print("%s: N %d, %d iterations, %d inliers, sim3 %.3g off the restatement (bound %.3g)" % (tag, o["N"], g["its"], g["ninl"], d, TOL))


def groups():
    g = {}
    for name in sorted(SCENES):
        g.setdefault(params_key(SCENES[name]), []).append(name)
    return sorted(g.values())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_alone(iv, name):
    """every scene of tests/sim3_scenes.py in a call of its own: an exact similarity, s != 1 under fix_scale 0 and 1, err 9.1 at level 0, the
    bound's edges on both sides, N = min_inliers - 1 / min_inliers / + 1, the resumed tie (success at iterations 7 and 40 through the state, then
    exhaustion), a blocking mnBestInliers, collinear and repeated samples, a point behind the cameras, the constructor's gates, swap-with-back,
    N = 3 / 64 / 65 / 128, max_iterations 1 and 300, a record out of range, an unselected pair"""
    sc = SCENES[name]
    got = run_calls(iv, [name])[name]
    for k, (o, g) in enumerate(zip(ref_runs(name), got)):
        compare(sc, k, o, g)


_GROUP = {}


def group_run(iv, names):
    key = tuple(names)
    if key not in _GROUP:
        _GROUP[key] = run_calls(iv, names)
    return _GROUP[key]


@pytest.mark.parametrize("names", groups(), ids=lambda g: g[0] + "+%d" % (len(g) - 1))
def test_scenes_in_one_call(iv, names):
    """all scenes that share their parameters in one call, at most 8 pairs at a time"""
    for i0 in range(0, len(names), 8):
        part = names[i0:i0 + 8]
        got = group_run(iv, part)
        for name in part:
            for k, (o, g) in enumerate(zip(ref_runs(name), got[name])):
                compare(SCENES[name], k, o, g)
    print("worst |device - restatement| so far: %.3g (bound %.3g)" % (WORST[0], TOL))


def test_runs_are_bit_identical_on_any_stream_in_any_pair_order_and_without_the_diagnostics(iv):
    names = ["resume_tie", "exact", "bound_edges", "gates", "n65", "bad_record", "unselected", "collinear_sample"]
    a = group_run(iv, names)
    tr = make_tracker(iv, len(names))
    b = run_calls(iv, names, tracker=tr)
    c = run_calls(iv, names, tracker=tr, stream=True)
    d = run_calls(iv, names, tracker=tr, order=list(range(len(names)))[::-1])
    e = run_calls(iv, names, hyp=False)
    for name in names:
        for k, ga in enumerate(a[name]):
            for key in ("sim3", "inlier", "ninl", "its", "hyp_sim3", "hyp_n", "state"):
                assert ga[key].tobytes() == b[name][k][key].tobytes(), "%s call %d: %s differs between two runs" % (name, k, key)
                assert ga[key].tobytes() == c[name][k][key].tobytes(), "%s call %d: %s differs on a non-default stream" % (name, k, key)
                assert ga[key].tobytes() == d[name][k][key].tobytes(), "%s call %d: %s differs under another pair order" % (name, k, key)
                if not key.startswith("hyp"):
                    assert ga[key].tobytes() == e[name][k][key].tobytes(), "%s call %d: %s differs without the hypothesis outputs" % (name, k, key)


def test_a_null_state_is_zero_and_nothing_is_written_back(iv):
    """the first call of resume_tie with state = NULL equals the call with {0, 0}; a resumed call in one piece equals the reference's next
    iterate: the state the first call left is (8, 43), the second finds iteration 40"""
    a = run_calls(iv, ["exact"], with_state=False)["exact"][0]
    b = run_calls(iv, ["exact"], with_state=True)["exact"][0]
    for key in ("sim3", "inlier", "ninl", "its", "hyp_sim3", "hyp_n"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert tuple(a["state"]) == (0, 0) and tuple(b["state"]) == (1, 40)
    got = run_calls(iv, ["resume_tie"])["resume_tie"]
    assert [tuple(g["state"]) for g in got] == [(8, 43), (41, 43), (47, 43), (47, 43)] and [int(g["ninl"]) for g in got] == [43, 43, 0, 0]


def test_arguments_are_checked(iv):
    base = SCENES["exact"]
    for bad in (dict(max_iterations=0), dict(max_iterations=301), dict(probability=1.0), dict(probability=0.0), dict(min_inliers=-1)):
        sc = dict(base, params=dict(base["params"], **bad), name="exact_bad")
        SCENES["exact_bad"] = sc
        try:
            with pytest.raises((iv.IvfError, ValueError)):
                run_calls(iv, ["exact_bad"])
        finally:
            del SCENES["exact_bad"]
    with pytest.raises(iv.IvfError):
        run_calls(iv, ["exact", "exact"], tracker=make_tracker(iv, 1))         # n_pairs > max_pairs


def test_chain_search_by_bow_keyframes_solve_sim3_search_by_sim3(iv):
    """the loop-closing chain on two synthetic keyframes related by a known similarity (s = 1.2 between the two maps, fix_scale 0):
    ivf_search_by_bow_keyframes finds vpMatched12 from the descriptors, solve_sim3 recovers the similarity from the matched map points,
    and ivf_search_by_sim3, fed with the projections under that similarity, finds every correspondence the first search was not given"""
    import torch
    from iv_slam_amd import dist as ivd, track
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    fx, fy, cx, cy = (np.float64(S.CAM[k]) for k in ("fx", "fy", "cx", "cy"))
    n = 60
    R12 = S.PS.rot((0.1, 1.0, 0.3), 2.0); t12 = np.array([0.3, 0.1, -0.4]); s12 = 1.2   # every point stays inside both images
    u = rng.uniform(80, S.W - 80, n); v = rng.uniform(60, S.H - 60, n); z = rng.uniform(5, 18, n)
    X1 = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    X2 = (X1 - t12) @ R12 / s12
    perm = rng.permutation(n)                                                  # KF1 keypoint i1 <-> KF2 keypoint perm[i1]
    proj = lambda X: np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    desc1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kp1 = np.zeros(n, S.KP_DTYPE); kp2 = np.zeros(n, S.KP_DTYPE)
    kp1["size"] = 31; kp2["size"] = 31
    kp1["x"], kp1["y"] = proj(X1).astype(F).T
    p2 = proj(X2).astype(F)
    kp2["x"][perm] = p2[:, 0]; kp2["y"][perm] = p2[:, 1]
    desc2 = np.zeros((n, 32), np.uint8); desc2[perm] = desc1
    (R1, t1), (R2, t2) = S.POSE1, S.POSE2
    xw = np.zeros((2, NF, 3), F); flags = np.zeros((2, NF), np.uint8)
    xw[0, :n] = ((X1 - t1) @ R1).astype(F); xw[1, perm] = ((X2 - t2) @ R2).astype(F)
    flags[:, :n] = 1
    known = np.arange(n) % 3 != 0                                              # the BoW search sees two thirds of the points through one node
    matcher = iv.ORBmatcher(0.75, True)
    fv1 = {0: [int(i) for i in np.nonzero(known)[0]]}; fv2 = {0: sorted(int(perm[i]) for i in np.nonzero(known)[0])}
    m12, nm = matcher.SearchByBoWKeyFrames(kp1, desc1, flags[0, :n], fv1, kp2, desc2, flags[1, :n], fv2)
    assert nm == known.sum() and np.array_equal(m12[known], perm[known]) and (m12[~known] == -1).all()
    rec = lambda kp, d: dict(kps=kp, desc=d, uright=np.full(n, -1.0, F), depth=np.full(n, -1.0, F))
    block = torch.from_numpy(ivd.pack_records([rec(kp1, desc1), rec(kp2, desc2)], NF).reshape(-1)).to(dev)
    tr = make_tracker(iv, 1)
    match = np.full((1, NF), -1, np.int32); match[0, :n] = m12
    poses = np.stack([S.pose12(*S.POSE1), S.pose12(*S.POSE2)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sim3 = torch.zeros((1, 16), dtype=torch.float32, device=dev); inl = torch.zeros((1, NF), dtype=torch.uint8, device=dev)
    ninl = torch.zeros(1, dtype=torch.int32, device=dev)
    tr.solve_sim3(block, up(np.array([[0, 1]], np.int32)), up(poses), up(xw), up(flags), up(match), up(track.sim3_draws(1, 300, 4).view(np.int32)),
                  sim3, inl, ninl, fix_scale=False)
    torch.cuda.synchronize()
    s = sim3.cpu().numpy()[0].astype(np.float64)
    Rg, tg, sg = s[:9].reshape(3, 3), s[9:12], s[12]
    print("chain: %d matches, %d inliers, R %.3g t %.3g s %.3g off the planted similarity" %
          (nm, ninl.item(), np.abs(Rg - R12).max(), np.abs(tg - t12).max(), abs(sg - s12)))
    assert ninl.item() == known.sum() and np.array_equal(inl.cpu().numpy()[0, :n], known.astype(np.uint8))
    assert np.abs(Rg - R12).max() < 1e-4 and np.abs(tg - t12).max() < 2e-3 and abs(sg - s12) < 1e-4
    # SearchBySim3 (ORBmatcher.cc:1145-1254): every map point of one keyframe projected into the other under the recovered similarity
    q = lambda Xc, d: dict(u=proj(Xc)[:, 0], v=proj(Xc)[:, 1], radius=np.full(n, 7.5, F), level=np.zeros(n, np.int32), desc=d, valid=np.ones(n, np.uint8))
    X1in2 = (X1 - tg) @ Rg / sg                                                # T21 X1
    X2in1 = sg * (X2[np.argsort(perm)] @ Rg.T) + tg                            # T12 X2, per KF2 keypoint slot
    found, nfound = matcher.SearchBySim3(kp1, desc1, S.BOUNDS, kp2, desc2, S.BOUNDS, q(X1in2, desc1), q(X2in1, desc2))
    assert nfound == n and np.array_equal(found, perm)
