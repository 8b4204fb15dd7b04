"""CPU side of the batched PnPsolver (ivf_tracker_solve_pnp): the entry point is exported, bound, documented and checks its arguments
without a GPU; tests/pnp_ref.py, the numpy f64 restatement of ORB/src/PnPsolver.cc, is checked against itself (two SVD back ends), against
the planted truth of tests/pnp_scenes.py and on hand-made values (the sampler, the iteration count); and tests/golden/pnp_noise.json, the
restatement's own noise floor, is current.

The floor is measured on the reference side only, never on the code under test: compute_pose on the planted inliers of every frame (what
Refine solves) under both back ends and 8 random summation orders; `floor` = max(measured spread, sqrt(3) * 2^-23), the float quantum of
the output pose (tests/test_pose_opt_cpu.py).  It is data, written by `python tests/test_pnp_cpu.py --write`.

What is NOT asserted, because the reference's algorithm does not promise it: that a 4-point hypothesis agrees between two back ends, or
that RANSAC finds a pose within the 1 iteration N = 10 gets or the 4 iterations N = 11 gets (an EPnP pose from 4 noisy points often
misses one of 10 points).  Both back ends must return a pose on every scene with an inlier share >= 0.7, N >= 15 and no degeneracy."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ref as R
import pnp_scenes as S
import pose_opt_ref as PR
import ransac_ref as RR
import sim3_ref as R3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_PATH = os.path.join(ROOT, "tests", "golden", "pnp_noise.json")
QUANTUM = float(np.sqrt(3.0) * 2.0 ** -23)
SCENARIOS = S.scenarios()
F = np.float32


def test_entry_point_is_exported_bound_and_documented():
    from iv_slam_amd import _lib, track
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    name = "ivf_tracker_solve_pnp"
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % name, hdr, flags=re.S)
    assert m and "Tracking.cc:" in m.group(1) and "PnPsolver.cc" in m.group(1), "the header comment cites the reference"
    assert len(_lib._SIGS[name][1]) == 21
    assert callable(track.BatchTracker.solve_pnp) and callable(track.pnp_draws)
    d = track.pnp_draws(3, 40, 15)
    assert d.dtype == np.uint32 and d.shape == (3, 40, 4) and d.max() <= R.RAND_MAX and np.array_equal(d, S.R_draws(15, 3, 40))


def test_argument_validation_without_gpu():
    from iv_slam_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    p = _lib.ptr(buf)
    one = C.c_void_p(16)                                                       # a non-null handle that must not be touched

    def call(t=one, rec=p, frames=p, xw=p, has=p, draws=p, mi=300, prob=0.99, mn=10, eps=0.5, th2=5.991, poses=p, inl=p, ninl=p, n_frames=1):
        return lib.ivf_tracker_solve_pnp(t, rec, 64, 1, frames, n_frames, xw, has, draws, mi, prob, mn, eps, th2, poses, inl, ninl, None, None, None, None)
    for kw in (dict(t=None), dict(rec=None), dict(frames=None), dict(xw=None), dict(has=None), dict(draws=None), dict(poses=None), dict(inl=None),
               dict(ninl=None), dict(mi=0), dict(mi=301), dict(prob=0.0), dict(prob=1.0), dict(eps=-0.1), dict(eps=1.5), dict(th2=0.0), dict(mn=-1)):
        assert call(**kw) == _lib.IVF_E_INVALID, kw
    assert b"max_iterations" in (call(mi=301), lib.ivf_last_error())[1]
    if lib.ivf_device_count() == 0:
        cfg = _lib.TrackConfig()
        cfg.nfeatures = 64; cfg.nlevels = 8
        for i in range(8):
            cfg.scale_factors[i] = 1.2 ** i
        cfg.fx = cfg.fy = 700.0; cfg.cx = 600.0; cfg.cy = 180.0; cfg.bf = 380.0; cfg.b = 0.5
        cfg.bounds = _lib.Bounds(0, 0, 1241, 376); cfg.th = 7.0; cfg.th_retry = 14.0; cfg.max_pairs = 1
        h = C.c_void_p()
        assert lib.ivf_tracker_create(C.byref(cfg), C.byref(h)) == _lib.IVF_E_NO_DEVICE, "no device: no handle, so no PnP either"


# ---- hand-made values --------------------------------------------------------------------------------------------------------------------
def transcribed_sample(N, draws, k=4):
    """a direct transcription of PnPsolver.cc:192-205 (k = 4) and Sim3Solver.cc:166-180 (k = 3) with RandomInt spelled out in integers"""
    v = list(range(N)); out = []
    for i in range(k):
        size = len(v)
        randi = int(int(draws[i]) / 2147483648.0 * size)
        out.append(v[randi]); v[randi] = v[-1]; v.pop()
    return out


def test_sampler_known_answers():
    RM = R.RAND_MAX
    assert R.random_int(0, 0, 9) == 0 and R.random_int(RM, 0, 9) == 9 and R.random_int(RM // 2, 0, 9) == 4 and R.random_int(RM // 2 + 1, 0, 9) == 5
    assert R.sample_indices(10, [0, 0, 0, 0]) == [0, 9, 8, 7]                  # the back moves to the front each time
    assert R.sample_indices(10, [RM, RM, RM, RM]) == [9, 8, 7, 6]
    assert R.sample_indices(4, [RM, 0, RM, 0]) == [3, 0, 1, 2]
    assert R.sample_indices(5, [0, RM, 0, RM]) == [0, 3, 4, 1]
    rng = np.random.default_rng(3)
    for N in (4, 5, 6, 7, 8, 11, 64, 1000):
        for _ in range(50):
            d = rng.integers(0, 2 ** 31, 4, dtype=np.uint32)
            if rng.uniform() < 0.3:
                d[rng.integers(0, 4)] = rng.choice([0, RM])
            got = R.sample_indices(N, d)
            assert got == transcribed_sample(N, d) and len(set(got)) == 4 and max(got) < N
            got3 = R3.sample_indices(N, d[:3])
            assert got3 == transcribed_sample(N, d, 3) == RR.sample_indices(N, d, 3) and got == RR.sample_indices(N, d, 4)


def test_iteration_count_known_answers():
    """SetRansacParameters (:137-156) with (0.99, 10, 300, 4, 0.5, 5.991) for the sizes the scenes use, worked out by hand:
    N < 10: refused; N = 10: mRansacMinInliers == N, one iteration; N = 11: eps = 10/11, ceil(3.31) = 4; N = 15: eps = 2/3, ceil(13.1) = 14;
    N >= 20: eps = 0.5, ceil(log(0.01) / log(0.875)) = ceil(34.49) = 35"""
    want = {0: (10, 0), 3: (10, 0), 9: (10, 0), 10: (10, 1), 11: (10, 4), 15: (10, 14), 64: (32, 35), 65: (32, 35), 257: (128, 35), 1000: (500, 35)}
    for N, (n_min, its) in want.items():
        assert R.ransac_parameters(N)[:2] == (n_min, its), N
    assert R.ransac_parameters(1000, max_iterations=20)[:2] == (500, 20)
    assert R.ransac_parameters(257, epsilon=0.3, max_iterations=40)[:2] == (77, 40) and R.ransac_parameters(257, epsilon=0.3)[:2] == (77, 169)
    assert R.ransac_parameters(6, min_inliers=2)[:2] == (4, 14)                # minSet = 4 bounds mRansacMinInliers; eps = 4/6 as for N = 15


def test_sampler_scene_tags_the_sample_and_catches_both_misreadings():
    """tests/pnp_scenes.py:sampler_scene, the CPU twin of tests/test_gpu_pnp.py's sampler test.  Under both back ends compute_pose is finite
    on every 4-sample the draws select from the clean frame and all-NaN on the frame whose NaN point the sample holds: the non-finite
    hypotheses of the 12 tagged frames name the sample.  The sets the device test expects differ from those of the no_swap misreading on
    every planted row that reads a rewritten position, and from those of draws read with stride 3 on more than half of the rows (row 0
    is the same under any stride; a random row coincides with probability 1 / 495): either mistake fails that test."""
    sc = S.sampler_scene()
    fr0 = sc["frames"][0]
    N, its, draws = fr0["N"], fr0["max_its"], sc["draws"][0]
    assert (N, fr0["n_min"], its) == (12, 4, 64) and all((d == draws).all() for d in sc["draws"])
    want = [RR.sample_indices(N, draws[it], 4) for it in range(its)]
    for it, (name, row, rewritten, smp) in enumerate(sc["rows"]):
        assert smp is None or want[it] == smp, name
        no_swap = RR.sample_indices(N, draws[it], 4, {"no_swap"})
        assert not rewritten or set(no_swap) != set(want[it]), name
    by_name = {row[0]: it for it, row in enumerate(sc["rows"])}
    assert want[by_name["all_zero"]] == [0, 11, 10, 9] and want[by_name["all_rand_max"]] == [11, 10, 9, 8]
    assert want[by_name["bit31_set"]] == want[by_name["bit31_clear"]] and (draws[by_name["bit31_set"]] >> 31).all()
    flat = draws.reshape(-1)
    stride3 = [RR.sample_indices(N, flat[3 * it:3 * it + 4], 4) for it in range(its)]
    assert sum(set(a) != set(b) for a, b in zip(stride3, want)) > its // 2
    _, X0, uv, _ = S.correspondences(fr0)
    for backend in ("numpy", "jacobi"):
        for it in range(its):
            smp = want[it]
            Rm, t, _ = R.compute_pose(X0[smp], uv[smp], S.CAM, backend)
            assert np.isfinite(Rm).all() and np.isfinite(t).all(), (backend, it, smp)
            for j in smp:
                _, Xj, _, _ = S.correspondences(sc["frames"][1 + j])
                assert np.isnan(Xj[j]).sum() == 1 and np.isfinite(np.delete(Xj, j, 0)).all()
                Rm, t, _ = R.compute_pose(Xj[smp], uv[smp], S.CAM, backend)
                assert np.isnan(Rm).all() and np.isnan(t).all(), (backend, it, j)


# ---- the restatement against itself and the planted truth ----------------------------------------------------------------------------------
def solve(sc, k, backend):
    fr = sc["frames"][k]
    idx, X, uv, s2 = S.correspondences(fr)
    dr = S.R_draws(sc["seed"], len(sc["frames"]), sc["params"]["max_iterations"])[k]
    return idx, R.solve(X, uv, s2, S.CAM, dr, backend=backend, **sc["params"])


@pytest.mark.parametrize("name", sorted(n for n, s in SCENARIOS.items() if not s["degenerate"]))
def test_both_back_ends_find_the_planted_inliers(name):
    sc = SCENARIOS[name]
    kinds = set()
    for k, fr in enumerate(sc["frames"]):
        for backend in ("numpy", "jacobi"):
            idx, o = solve(sc, k, backend)
            assert o["max_its"] == fr["max_its"] and o["n_min"] == fr["n_min"]
            kinds.add(o["pose"] is not None)
            if fr["max_its"] == 0:
                assert o["pose"] is None and o["iterations"] == 0 and o["ninliers"] == 0
            if o["pose"] is not None and o["refined"]:
                assert np.array_equal(o["mask"], fr["planted"][idx]), (name, k, backend)
                rot, tr = PR.pose_difference(o["pose"], fr["pose_gt"])
                assert rot < 2e-3 and tr < 2e-2, (name, k, backend, rot, tr)
            if fr["share"] >= 0.7 and fr["N"] >= 15:
                assert o["pose"] is not None and o["refined"], (name, k, backend)
            if name == "share_04_default":
                assert o["pose"] is None and o["iterations"] == 35, "fewer inliers than mRansacMinInliers = N / 2: no hypothesis qualifies"
    if name == "share_04_eps03":
        assert kinds == {True, False}, "the 40 % scenes keep seeds with and without a pose"


def test_compute_pose_on_the_planted_inliers_agrees_between_the_back_ends():
    n = 0
    for name, sc in SCENARIOS.items():
        for fr in sc["frames"]:
            idx, X, uv, s2 = S.correspondences(fr)
            keep = fr["planted"][idx]
            if sc["degenerate"] or keep.sum() < 11:
                continue
            a = R.compute_pose(X[keep], uv[keep], S.CAM, "numpy"); b = R.compute_pose(X[keep], uv[keep], S.CAM, "jacobi")
            rot, tr = PR.pose_difference(R.pose12(a[0], a[1]), R.pose12(b[0], b[1]))
            assert rot <= QUANTUM and tr <= QUANTUM and abs(a[2] - b[2]) < 1e-9, (name, fr["seed"], rot, tr)
            n += 1
    assert n >= 12


def test_jacobi_svd_is_an_svd():
    rng = np.random.default_rng(1)
    for m, n in ((3, 3), (6, 3), (6, 4), (6, 5), (12, 12)):
        A = rng.normal(size=(m, n))
        if m == 12:
            B = rng.normal(size=(8, 12)); A = B.T @ B                          # rank 8, like a hypothesis's MtM
        U, w, V = R.svd_jacobi(A)
        assert np.allclose(V.T @ V, np.eye(n), atol=1e-13) and (np.diff(w) <= 0).all()
        assert np.allclose((U * w) @ V.T, A, atol=1e-12 * max(1.0, w[0]))
        assert np.allclose(w, np.linalg.svd(A, compute_uv=False), atol=1e-12 * max(1.0, w[0]))


# ---- the noise floor ----------------------------------------------------------------------------------------------------------------------------
def measure():
    out = {}
    for name, sc in sorted(SCENARIOS.items()):
        if sc["degenerate"]:
            continue
        rot = tr = 0.0
        border = {}; gt = {}
        for k, fr in enumerate(sc["frames"]):
            if k in sc["bad"] or fr["planted"].sum() < 11:
                continue
            base, r, t, b = S.refine_spread(fr)
            rot = max(rot, r); tr = max(tr, t)
            if b:
                border[str(k)] = b
            gt[str(k)] = [float(v) for v in PR.pose_difference(R.pose12(base[0], base[1]), fr["pose_gt"])]
        out[name] = dict(spread_rot=rot, spread_trans=tr, floor_rot=max(rot, QUANTUM), floor_trans=max(tr, QUANTUM), borderline=border, gt=gt,
                         n_points=int(sum(fr["N"] for fr in sc["frames"])))
    return out


def test_noise_floor_file_is_current_and_under_the_cap():
    gold = json.load(open(NOISE_PATH))
    m = measure()
    assert sorted(gold) == sorted(m)
    for name, v in m.items():
        g = gold[name]
        assert v["spread_rot"] <= g["floor_rot"] and v["spread_trans"] <= g["floor_trans"], (name, v, g)
        assert g["floor_rot"] >= QUANTUM and g["floor_trans"] >= QUANTUM
        assert g["borderline"] == v["borderline"] and g["n_points"] == v["n_points"], name
        assert sum(len(b) for b in g["borderline"].values()) <= 0.01 * g["n_points"]
        for k, d in v["gt"].items():
            assert np.allclose(d, g["gt"][k], rtol=0, atol=4 * QUANTUM)


if __name__ == "__main__":
    if "--write" in sys.argv:
        with open(NOISE_PATH, "w") as f:
            json.dump(measure(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", NOISE_PATH)
