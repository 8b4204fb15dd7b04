"""sim3_scenes.py -- the hand-made scenes of the Sim3Solver tests (test infrastructure only), shared by tests/test_sim3_cpu.py (the
restatement tests/sim3_ref.py against these expectations, every injected misreading caught by a named scene, the spreads in
tests/golden/sim3_noise.json) and tests/test_gpu_sim3.py (ivf_tracker_solve_sim3 against the restatement), on the camera of
tests/pose_opt_scenes.py with nfeatures = 128.

A scene is one (KF1, KF2) pair of its own two records.  N correspondences obey a planted similarity X1 = s R X2 + t between the two camera
frames exactly (up to the float storage of the world points: reprojection errors of 1e-6 px^2), except the planted ones:
  ("err1", d) / ("err2", d)  the reprojection into camera 1 / camera 2 is moved by d px along x, so err1 / err2 = d^2; the other side's
                             keypoint sits at octave 4 (bound 39), so only the named comparison decides
  ("gross",)                 X2 is another point altogether (errors of 1e3 px^2 and more)
  ("behind",)                the point lies behind both cameras; it obeys the similarity
and the samples of the iterations are chosen through the draws (sim3_ref.draws_for) wherever a scene depends on them.  Each call of a scene
states what must come out: N, ninliers, iterations, the state, the inlier correspondences, iterations that must fail.  `ties` lists the
groups of iterations whose inlier counts are equal by construction; no other two iterations of a scene may tie."""
import numpy as np

import pose_opt_scenes as PS
import sim3_ref as R

F = np.float32
D = np.float64
CAM, SCALE, BOUNDS, KP_DTYPE, W, H = PS.CAM, PS.SCALE, PS.BOUNDS, PS.KP_DTYPE, PS.W, PS.H
SIGMA2 = R.level_sigma2(SCALE)
NF = 128
DEFAULTS = dict(max_iterations=300, probability=0.99, min_inliers=20, fix_scale=True)
POSE1 = (PS.rot((0.1, 1.0, 0.2), 20.0), np.array([1.0, -0.5, 2.0]))
POSE2 = (PS.rot((-0.3, 1.0, 0.1), -15.0), np.array([-2.0, 0.3, 1.0]))


def pose12(Rm, t):
    T = np.zeros((3, 4), F); T[:, :3] = Rm; T[:, 3] = t
    return T.reshape(12)


def make_scene(name, seed, N, plant=None, extras=(), s12=1.0, rot12=((0.2, 1.0, -0.1), 12.0), t12=(0.4, -0.2, 0.3), samples=None, params=None,
               calls=None, ties=(), shape=None, note=""):
    """plant: {correspondence ordinal: spec}; extras: kinds of KF1 keypoints that are NOT collected ("nomatch", "dead1", "dead2", "beyond",
    "far_beyond"), spread among the correspondences; samples: {iteration: three ordinals} (the others: `fill`, or the seeded draws);
    shape: "collinear" / "repeated" = correspondences 0, 1, 2 lie on a line / 0 and 1 carry one point."""
    rng = np.random.default_rng(seed)
    plant = dict(plant or {}); p = dict(DEFAULTS, **(params or {}))
    fx, fy, cx, cy = (D(CAM[k]) for k in ("fx", "fy", "cx", "cy"))
    R12 = PS.rot(*rot12); t12 = np.asarray(t12, D)
    nk1 = N + len(extras); nk2 = min(NF, N + 3) if N + 3 <= NF else N
    assert nk1 <= NF
    # the correspondences in camera 1, then camera 2 through the planted similarity
    u = rng.uniform(60, W - 60, N); v = rng.uniform(40, H - 40, N); z = rng.uniform(4, 20, N)
    X1 = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    if shape == "collinear":
        X1[1] = X1[0] + np.array([0.9, 0.3, 1.1]); X1[2] = X1[0] + 2.5 * np.array([0.9, 0.3, 1.1])
    oct1 = rng.integers(0, 8, N); oct2 = rng.integers(0, 8, N)
    for j, spec in plant.items():
        if spec[0] == "behind":
            X1[j, 2] = -X1[j, 2]
    if shape == "repeated":
        X1[1] = X1[0]
    to2 = lambda X: (X - t12) @ R12 / s12                                    # X2 = R^T (X1 - t) / s
    X2 = to2(X1)
    for j, spec in plant.items():
        if spec[0] == "err1":                                               # T12 X2 projects d px beside P1im1
            X2[j] = to2(X1[j] + np.array([spec[1] * X1[j, 2] / fx, 0.0, 0.0])); oct1[j] = 0; oct2[j] = 4
        elif spec[0] == "err2":                                             # T21 X1 projects d px beside P2im2
            X2[j] = X2[j] + np.array([spec[1] * X2[j, 2] / fx, 0.0, 0.0]); oct1[j] = 4; oct2[j] = 0
        elif spec[0] == "gross":
            X2[j] = X2[j] + rng.uniform(2.0, 4.0, 3) * rng.choice([-1.0, 1.0], 3)
    # the keypoint slots: correspondences and extras interleaved in KF1, a permutation in KF2
    kinds = ["corr"] * N + list(extras)
    order = rng.permutation(nk1) if extras else np.arange(nk1)
    slot_kind = [kinds[k] for k in order]
    slot1 = np.array([i for i, k in enumerate(slot_kind) if k == "corr"])     # correspondence ordinal -> i1, in collection order
    slot2 = rng.permutation(nk2)[:N]
    (R1, t1), (R2, t2) = POSE1, POSE2
    xw1 = np.zeros((nk1, 3), F); xw2 = np.zeros((nk2, 3), F)
    xw1[slot1] = ((X1 - t1) @ R1).astype(F); xw2[slot2] = ((X2 - t2) @ R2).astype(F)
    flags1 = np.zeros(nk1, np.uint8); flags2 = np.zeros(nk2, np.uint8)
    flags1[slot1] = 1; flags2[slot2] = 1
    kp1 = np.zeros(nk1, KP_DTYPE); kp2 = np.zeros(nk2, KP_DTYPE)
    kp1["size"] = 31; kp2["size"] = 31
    kp1["x"] = rng.uniform(20, W - 20, nk1).astype(F); kp1["y"] = rng.uniform(20, H - 20, nk1).astype(F)
    kp2["x"] = rng.uniform(20, W - 20, nk2).astype(F); kp2["y"] = rng.uniform(20, H - 20, nk2).astype(F)
    kp1["octave"][slot1] = oct1; kp2["octave"][slot2] = oct2
    match12 = np.full(NF, -1, np.int32)
    match12[slot1] = slot2
    spare2 = [i for i in range(nk2) if i not in set(slot2.tolist())]
    want_stage = np.full(nk1, R.NO_MATCH, np.int32)
    want_stage[slot1] = R.INLIER
    for i1, kind in enumerate(slot_kind):
        if kind == "corr" or kind == "nomatch":
            continue
        xw1[i1] = (1.0, 1.0, 8.0)
        if kind == "dead1":                                                  # KF1's keypoint holds no live point; KF2's does
            match12[i1] = slot2[0]; flags1[i1] = 2; want_stage[i1] = R.NO_POINT1
        elif kind == "dead2":                                                # KF2's keypoint holds no live point
            match12[i1] = spare2[0]; flags1[i1] = 1; flags2[spare2[0]] = 2; xw2[spare2[0]] = (1.0, 2.0, 9.0); want_stage[i1] = R.NO_POINT2
        elif kind == "beyond":                                               # one past KF2's count: inside the arrays, not a keypoint
            match12[i1] = nk2; flags1[i1] = 1; want_stage[i1] = R.BAD
        elif kind == "far_beyond":                                           # outside every array
            match12[i1] = 100000; flags1[i1] = 1; want_stage[i1] = R.BAD
    match12[nk1:nk1 + 2] = slot2[:2] if nk1 + 2 <= NF else match12[nk1:nk1 + 2]   # past KF1's count: never read
    kf = lambda kp, n, pose, xw, fl: dict(kps=kp, n=n, pose=pose12(*pose), xw=xw, flags=fl, desc=np.zeros((n, 32), np.uint8),
                                          uright=np.full(n, -1.0, F), depth=np.full(n, -1.0, F))
    mi = p["max_iterations"]
    draws = np.random.default_rng(seed + 7).integers(0, 2 ** 31, size=(mi, 3), dtype=np.uint32)
    for it, smp in (samples or {}).items():
        if it == "fill":
            continue
        draws[it] = R.draws_for(N, smp)
    if samples and "fill" in samples:
        for it in range(mi):
            if it not in samples:
                draws[it] = R.draws_for(N, samples["fill"])
    its, x = R.ransac_iterations(N, p["probability"], p["min_inliers"], mi)
    assert x is None or abs(x - round(x)) > 1e-6, "%s: log(1 - p) / log(1 - eps^3) = %r is too close to an integer" % (name, x)
    return dict(name=name, kf1=kf(kp1, nk1, POSE1, xw1, flags1), kf2=kf(kp2, nk2, POSE2, xw2, flags2), match12=match12, draws=draws, params=p,
                N=N, slot1=slot1, slot2=slot2, truth=(R12, t12, s12), calls=calls, ties=[list(g) for g in ties], want_stage=want_stage,
                max_its=its, bad=False, select=1, note=note, plant=plant)


def call(ninliers, iterations, state=None, state_out=None, outliers=(), fail_its=(), truth=True):
    """one call of a scene: the state it starts from (None = no state array, "chain" = what the previous call left, or a tuple) and what
    must come out; outliers = correspondence ordinals that are not inliers of the returned transform; fail_its = iterations whose count
    must stay at or below min_inliers; truth = the returned transform is the planted one"""
    return dict(state=state, ninliers=ninliers, iterations=iterations, state_out=state_out, outliers=list(outliers), fail_its=list(fail_its), truth=truth)


def scenes():
    S = []
    add = lambda *a, **k: S.append(make_scene(*a, **k))
    # every match an inlier at iteration 0
    add("exact", 1, 40, calls=[call(40, 1)])
    add("max_it_1", 2, 40, params=dict(max_iterations=1), calls=[call(40, 1)])
    # s != 1: found with fix_scale 0; under fix_scale 1 the one iteration fits with s = 1 and fails
    add("scale_free", 3, 40, s12=1.3, params=dict(fix_scale=False), calls=[call(40, 1)])
    add("scale_fixed", 3, 40, s12=1.3, params=dict(max_iterations=1), calls=[call(0, 1, fail_its=[0])])
    # err1 = 9.1 at level 0: 9.21 * 1 truncates to 9
    add("err_9p1_level0", 4, 30, plant={5: ("err1", 9.1 ** 0.5)}, samples={0: (0, 1, 2)}, calls=[call(29, 1, outliers=[5])])
    # just inside and outside the bound, on each side
    add("bound_edges", 5, 30, plant={3: ("err1", 8.9 ** 0.5), 4: ("err1", 9.1 ** 0.5), 6: ("err2", 8.9 ** 0.5), 7: ("err2", 9.1 ** 0.5)},
        samples={0: (0, 1, 2)}, calls=[call(28, 1, outliers=[4, 7])])
    # around the refusal: N = 19 refused; N = 20 = mRansacMinInliers: one iteration whose 20 inliers are not MORE than 20; N = 21
    add("n_min_minus_1", 6, 19, calls=[call(0, 0)])
    add("n_eq_min", 7, 20, calls=[call(0, 1, fail_its=[0])])
    add("n_min_plus_1", 8, 21, calls=[call(21, 1)])
    # a first success at iteration 7, a second at iteration 40 reached through the state: its count TIES with mnBestInliers and must
    # replace it (:186); then the remaining iterations fail, and a call on an exhausted solver runs nothing.  Sample (0, 1, 2) holds the
    # gross outlier 0.  N = 44: epsilon = 20 / 44, 47 iterations
    bad, good1, good2 = (0, 1, 2), (3, 4, 5), (6, 7, 8)
    add("resume_tie", 9, 44, plant={0: ("gross",)}, samples={"fill": bad, 7: good1, 40: good2},
        calls=[call(43, 8, state=(0, 0), state_out=(8, 43), outliers=[0], fail_its=range(7)),
               call(43, 41, state="chain", state_out=(41, 43), outliers=[0], fail_its=range(8, 40)),
               call(0, 47, state="chain", state_out=(47, 43), fail_its=range(41, 47)),
               call(0, 47, state="chain", state_out=(47, 43))],
        ties=[[i for i in range(47) if i not in (7, 40)], [7, 40]])
    # mnBestInliers on entry above every count: 35 clean iterations, none may succeed
    add("state_blocks", 10, 40, calls=[call(0, 35, state=(0, 100), state_out=(35, 100))], ties=[list(range(35))])
    # degenerate samples at iteration 0, a clean one at iteration 1
    add("collinear_sample", 11, 30, shape="collinear", samples={0: (0, 1, 2), 1: (3, 4, 5)}, calls=[call(30, 2, fail_its=[0])])
    add("repeated_sample", 12, 30, shape="repeated", samples={0: (0, 1, 2), 1: (3, 4, 5)}, calls=[call(30, 2, fail_its=[0])])
    # a point behind both cameras obeys the similarity: an inlier, there is no test on z
    add("behind_camera", 13, 30, plant={4: ("behind",)}, samples={0: (0, 1, 2)}, calls=[call(30, 1)])
    # the gates of the constructor
    add("gates", 14, 25, extras=("nomatch", "nomatch", "dead1", "dead2", "beyond", "far_beyond"), calls=[call(25, 1)])
    # swap-with-back: draws (0, 0, 0) take correspondences 0, N - 1, N - 2; erasing in order would take 0, 1, 2, and 1 is a gross outlier
    sc = make_scene("swap_with_back", 15, 30, plant={1: ("gross",)}, params=dict(max_iterations=1), calls=[call(29, 1, outliers=[1])])
    sc["draws"][0] = 0
    S.append(sc)
    # sizes: N = 3 (min_inliers 2), one wave, one wave and one more, every slot of the record; 30 % gross outliers, seeded draws
    add("n3", 16, 3, params=dict(min_inliers=2), calls=[call(3, 1)])
    for name, seed, N in (("n64", 17, 64), ("n65", 18, 65), ("n128", 23, 128)):
        rng = np.random.default_rng(seed)
        out = sorted(rng.permutation(N)[:int(0.3 * N)].tolist())
        S.append(make_scene(name, seed, N, plant={j: ("gross",) for j in out}, calls=[call(N - len(out), None, outliers=out)]))
    # a record index outside the block, and a pair left out
    sc = make_scene("bad_record", 20, 30, calls=[call(-1, None, truth=False)]); sc["bad"] = True; S.append(sc)
    sc = make_scene("unselected", 21, 30, calls=[call(-2, None, truth=False)]); sc["select"] = 0; S.append(sc)
    return {s["name"]: s for s in S}


def run_ref(sc, mis=()):
    """the restatement on every call of a scene -> list of sim3_ref.solve results (None for a pair the call does not reach)"""
    outs = []
    state = None
    for c in sc["calls"]:
        if sc["bad"] or not sc["select"]:
            outs.append(None)
            continue
        st = state if c["state"] == "chain" else c["state"]
        o = R.solve(sc["kf1"], sc["kf2"], sc["match12"], CAM, SIGMA2, sc["draws"], state=st, mis=mis, **sc["params"])
        state = o["state"]
        outs.append(o)
    return outs


def hypotheses_checked(sc, o):
    """the info records the device's per-iteration outputs are compared with: every iteration the restatement ran in this call, and the
    first 8 behind them up to mRansacMaxIts (the device computes all of them at once; the reference would not have run these)"""
    first = o["iterations"] - len(o["info"])
    ran = set(info["it"] for info in o["info"])
    after = [it for it in range(first, o["max_its"]) if it not in ran][:8]
    return first, o["info"] + [R.hypothesis(o["C"], it, sc["draws"], CAM, sc["params"]["fix_scale"]) for it in after]


def mismatch(sc, outs):
    """why the results of run_ref (or the device's, in the same form) do not meet the scene's expectations; None when they do"""
    for k, (c, o) in enumerate(zip(sc["calls"], outs)):
        if o is None:
            continue
        tag = "%s call %d: " % (sc["name"], k)
        if o["N"] != sc["N"] or o["max_its"] != sc["max_its"]:
            return tag + "N %d, mRansacMaxIts %d, expected %d, %d" % (o["N"], o["max_its"], sc["N"], sc["max_its"])
        if o["ninliers"] != c["ninliers"]:
            return tag + "ninliers %d, expected %d" % (o["ninliers"], c["ninliers"])
        if c["iterations"] is not None and o["iterations"] != c["iterations"]:
            return tag + "iterations %d, expected %d" % (o["iterations"], c["iterations"])
        if c["state_out"] is not None and tuple(o["state"]) != tuple(c["state_out"]):
            return tag + "state %r, expected %r" % (o["state"], c["state_out"])
        for info in o["info"]:
            if info["it"] in c["fail_its"] and info["ninliers"] > sc["params"]["min_inliers"]:
                return tag + "iteration %d has %d inliers, it must fail" % (info["it"], info["ninliers"])
        want = np.zeros(sc["kf1"]["n"], np.uint8)
        if c["ninliers"] > 0:
            want[np.delete(sc["slot1"], c["outliers"])] = 1
        if not np.array_equal(o["inlier"], want):
            return tag + "inlier flags differ at %r" % np.nonzero(o["inlier"] != want)[0][:8]
        if (o["sim3"] is None) != (c["ninliers"] <= 0):
            return tag + "a transform without a success, or none with one"
        if c["ninliers"] > 0:
            st = sc["want_stage"].copy()
            for j in c["outliers"]:
                kind = sc["plant"][j][0]
                got = o["stage"][sc["slot1"][j]]
                if got not in ((R.FAIL_ERR1,) if kind == "err1" else (R.FAIL_ERR2,) if kind == "err2" else (R.FAIL_ERR1, R.FAIL_ERR2)):
                    return tag + "correspondence %d (%s) has stage %s" % (j, kind, R.STAGE_NAMES[got])
                st[sc["slot1"][j]] = got
            if not np.array_equal(o["stage"], st):
                return tag + "stage codes differ at %r" % np.nonzero(o["stage"] != st)[0][:8]
            if c["truth"]:
                R12, t12, s12 = sc["truth"]
                s = o["sim3"]
                if sc["params"]["fix_scale"] and s[12] != 1.0:
                    return tag + "scale %r under fix_scale" % s[12]
                dR = np.abs(s[:9].reshape(3, 3) - R12).max(); dt = np.abs(s[9:12] - t12).max(); ds = abs(s[12] - s12)
                if not (dR < 1e-4 and dt < 2e-3 and ds < 1e-4):
                    return tag + "transform off the planted one: R %.3g t %.3g s %.3g" % (dR, dt, ds)
    return None
