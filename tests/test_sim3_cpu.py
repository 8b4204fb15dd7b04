"""CPU side of the batched Sim3Solver (ivf_tracker_solve_sim3): the entry point is exported, bound, documented and checks its arguments
without a GPU; tests/sim3_ref.py, the numpy restatement of ORB/src/Sim3Solver.cc, meets the expectation every scene of
tests/sim3_scenes.py states; every misreading it can inject is caught by a named scene; its closed form agrees with an independent
statement (full f64, numpy.linalg.eigh); and tests/golden/sim3_noise.json, the spreads measured here, is current.

The spreads are measured on the reference side only, never on the code under test: `spread` = the worst difference of R, t and s between
the restatement (float M and N, frozen Jacobi) and the independent statement over every non-degenerate sample the scenes draw and 400
seeded random triples; `min_margin` = the smallest distance of any err1 / err2 from its integer bound over every iteration every scene
runs and the 8 behind them that tests/test_gpu_sim3.py also compares.  Non-vacuity, asserted: min_margin > 64 x spread (no comparison
of any scene can turn on the arithmetic the two statements differ in), and no two iterations a scene runs tie in their inlier count
except the groups the scene declares.  The file is data, written by `python tests/test_sim3_cpu.py --write`; tests/test_gpu_sim3.py
holds the device to 8 x spread."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ref as R
import sim3_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_PATH = os.path.join(ROOT, "tests", "golden", "sim3_noise.json")
SCENES = S.scenes()
F = np.float32
DEGENERATE = {("collinear_sample", 0), ("repeated_sample", 0)}            # (scene, iteration): the top eigenvalue of N is double

# the scene that catches each misreading of tests/sim3_ref.py
CATCHES = {
    "float_threshold": "err_9p1_level0",
    "best_strict": "resume_tie",
    "success_nonstrict": "n_eq_min",
    "return_best": "n_eq_min",
    "no_swap": "swap_with_back",
    "z_sign": "behind_camera",
    "scale_not_fixed": "scale_fixed",
    "t21_not_inverted": "exact",
    "state_not_resumed": "resume_tie",
}

_REF = {}


def ref_runs(name):
    """the restatement's answer on a scene, computed once and shared among the tests"""
    if name not in _REF:
        _REF[name] = S.run_ref(SCENES[name])
    return _REF[name]


def test_entry_point_is_exported_bound_and_documented():
    from iv_slam_amd import _lib, track
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    name = "ivf_tracker_solve_sim3"
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % name, hdr, flags=re.S)
    assert m and "Sim3Solver.cc" in m.group(1) and "LoopClosing.cc:" in m.group(1), "the header comment cites the reference"
    assert "GetIndexInKeyFrame" in m.group(1), "the header states what the index in the keyframe is taken to be"
    assert len(_lib._SIGS[name][1]) == 24
    assert callable(track.BatchTracker.solve_sim3) and callable(track.sim3_draws)
    d = track.sim3_draws(3, 40, 15)
    assert d.dtype == np.uint32 and d.shape == (3, 40, 3) and d.max() <= R.RAND_MAX
    assert np.array_equal(d, np.random.default_rng(15).integers(0, 2 ** 31, size=(3, 40, 3), dtype=np.uint32))


def test_argument_validation_without_gpu():
    from iv_slam_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    p = _lib.ptr(buf)
    one = C.c_void_p(16)                                                       # a non-null handle that must not be touched

    def call(t=one, rec=p, pairs=p, poses=p, xw=p, flags=p, m12=p, draws=p, mi=300, prob=0.99, mn=20, sim3=p, inl=p, ninl=p):
        return lib.ivf_tracker_solve_sim3(t, rec, 64, 1, pairs, 1, None, poses, xw, flags, m12, draws, mi, prob, mn, 1, None, sim3, inl, ninl,
                                          None, None, None, None)
    for kw in (dict(t=None), dict(rec=None), dict(pairs=None), dict(poses=None), dict(xw=None), dict(flags=None), dict(m12=None), dict(draws=None),
               dict(sim3=None), dict(inl=None), dict(ninl=None), dict(mi=0), dict(mi=301), dict(prob=0.0), dict(prob=1.0), dict(mn=-1)):
        assert call(**kw) == _lib.IVF_E_INVALID, kw
    assert b"max_iterations" in (call(mi=301), lib.ivf_last_error())[1]


# ---- hand-made values ----------------------------------------------------------------------------------------------------------------------
def test_bound_sampler_and_iteration_count_known_answers():
    s2 = R.level_sigma2(S.SCALE)
    assert [int(R.max_error(v)) for v in s2[:5]] == [9, 13, 19, 27, 39]        # 9.21 x 1, 1.44, 2.0736, 2.985984, 4.29981696, truncated
    assert float(R.max_error(s2[0], {"float_threshold"})) == float(F(9.21))
    RM = R.RAND_MAX
    assert R.sample_indices(10, [0, 0, 0]) == [0, 9, 8] and R.sample_indices(10, [RM, RM, RM]) == [9, 8, 7]
    assert R.sample_indices(5, [0, RM, 0]) == [0, 3, 4] and R.sample_indices(3, [RM, 0, 0]) == [2, 0, 1]
    assert R.sample_indices(10, [0, 0, 0], {"no_swap"}) == [0, 1, 2]
    rng = np.random.default_rng(3)
    for N in (3, 4, 5, 11, 64, 128):
        for _ in range(40):
            want = [int(v) for v in rng.permutation(N)[:3]]
            assert R.sample_indices(N, R.draws_for(N, want)) == want
    # SetRansacParameters with (0.99, 20, 300): N < 20 refused; N = 20 one iteration; N = 21: eps = 20 / 21, ceil(2.31) = 3; N = 30: eps = 2 / 3,
    # ceil(13.1) = 14; N = 40: eps = 0.5, ceil(34.49) = 35; N = 44: ceil(46.7) = 47; N = 64: ceil(148.6) = 149; N = 128: 1204 -> 300
    want = {2: 0, 19: 0, 20: 1, 21: 3, 30: 14, 40: 35, 44: 47, 64: 149, 128: 300}
    for N, its in want.items():
        assert R.ransac_iterations(N)[0] == its, N
    assert R.ransac_iterations(40, max_iterations=20)[0] == 20 and R.ransac_iterations(3, min_inliers=2)[0] == 14
    assert R.ransac_iterations(2, min_inliers=0)[0] == 0 and R.ransac_iterations(5, min_inliers=0)[0] == 1


def test_jacobi_eigen4_is_an_eigendecomposition():
    rng = np.random.default_rng(1)
    for _ in range(50):
        B = rng.normal(size=(4, 4)); A = B + B.T
        w, V = R.jacobi_eigen4(A)
        V = np.array(V); w = np.array(w)
        assert np.allclose(V.T @ V, np.eye(4), atol=1e-13) and np.allclose(V @ np.diag(w) @ V.T, A, atol=1e-12)
        assert np.allclose(np.sort(w), np.linalg.eigvalsh(A), atol=1e-12)
    w, V = R.jacobi_eigen4(np.diag([1.0, 3.0, 2.0, -1.0]))                     # a diagonal N is left alone: the vector of 3 is e1
    assert w == [1.0, 3.0, 2.0, -1.0] and np.array_equal(np.array(V), np.eye(4))


def test_a_vanishing_imaginary_part_gives_nan_and_no_inlier():
    """a pure translation of points whose coordinates the centroid subtraction keeps exact: N is diagonal, evec.row(0) = (1, 0, 0, 0),
    vec / norm(vec) = 0 / 0 (:283): the hypothesis is NaN and counts no inlier, as in the reference"""
    P1 = np.array([[0, 0, 4], [3, 0, 7], [0, 3, 10]], F); P2 = P1 + F(1.0)
    Rm, t, s = R.compute_sim3(P1, P2, True)
    assert np.isnan(Rm).all() and np.isnan(t).all()
    C0 = dict(X1=P1, X2=P2, e1=np.full(3, 9, F), e2=np.full(3, 9, F), im1=np.array([R.to_image(x, S.CAM) for x in P1], F),
              im2=np.array([R.to_image(x, S.CAM) for x in P2], F))
    assert not R.check_inliers(C0, R.transforms_of(Rm, t, s), S.CAM)[0].any()


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_meets_the_scene(name):
    sc = SCENES[name]
    assert S.mismatch(sc, ref_runs(name)) is None
    if name == "gates":
        st = ref_runs(name)[0]["stage"]
        assert sorted(set(st.tolist())) == [R.NO_MATCH, R.NO_POINT1, R.NO_POINT2, R.BAD, R.INLIER] and (st == R.BAD).sum() == 2


@pytest.mark.parametrize("mis", sorted(R.MISREADINGS))
def test_every_misreading_is_caught_by_its_scene(mis):
    sc = SCENES[CATCHES[mis]]
    assert S.mismatch(sc, ref_runs(sc["name"])) is None
    why = S.mismatch(sc, S.run_ref(sc, mis={mis}))
    print("%s (%s): %s" % (mis, R.MISREADINGS[mis], why))
    assert why is not None, "%s is not caught by scene %s" % (mis, sc["name"])


def test_only_declared_iterations_tie():
    for name, sc in SCENES.items():
        counts = {}
        for o in ref_runs(name):
            for info in (o["info"] if o else []):
                counts.setdefault(info["ninliers"], []).append(info["it"])
        tied = sorted(sorted(v) for v in counts.values() if len(v) > 1)
        assert tied == sorted(sorted(g) for g in sc["ties"]), "%s: iterations tie: %r" % (name, tied)


# ---- the closed form against an independent statement, and the spreads ---------------------------------------------------------------------
def random_triples(n=400, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        P1 = rng.uniform(-6, 6, (3, 3)); P1[:, 2] = rng.uniform(4, 20, 3)
        a, b = P1[1] - P1[0], P1[2] - P1[0]
        if np.linalg.norm(np.cross(a, b)) < 0.2 * np.linalg.norm(a) * np.linalg.norm(b):
            continue                                                            # sin of the angle at point 0 below 0.2: close to a line
        Rm = S.PS.rot(rng.normal(size=3), rng.uniform(1, 60)); t = rng.uniform(-2, 2, 3); s = rng.uniform(0.7, 1.4)
        P2 = (P1 - t) @ Rm / s + rng.normal(scale=0.02, size=(3, 3))
        out.append((P1.astype(F), P2.astype(F), bool(len(out) % 2)))
    return out


def measure():
    dR = dt = ds = 0.0
    n = 0
    margin = np.inf
    triples = random_triples()
    for name, sc in sorted(SCENES.items()):
        for o in ref_runs(name):
            for info in (S.hypotheses_checked(sc, o)[1] if o else []):
                Cc = o["C"]
                with np.errstate(all="ignore"):
                    d = np.concatenate([np.abs(info["err1"].astype(np.float64) - Cc["e1"]), np.abs(info["err2"].astype(np.float64) - Cc["e2"])])
                d = d[np.isfinite(d)]
                if len(d):
                    margin = min(margin, float(d.min()))
                if (name, info["it"]) not in DEGENERATE and info["it"] < o["iterations"]:
                    triples.append((Cc["X1"][info["sample"]], Cc["X2"][info["sample"]], sc["params"]["fix_scale"]))
    for P1, P2, fix in triples:
        Rm, t, s = R.compute_sim3(P1, P2, fix)
        R64, t64, s64 = R.horn_f64(P1, P2, fix)
        assert np.isfinite(Rm).all(), "a non-degenerate triple gave NaN"
        dR = max(dR, float(np.abs(Rm.astype(np.float64) - R64).max())); dt = max(dt, float(np.abs(t.astype(np.float64) - t64).max()))
        ds = max(ds, abs(float(s) - s64)); n += 1
    return dict(spread_R=dR, spread_t=dt, spread_s=ds, spread=max(dR, dt, ds), min_margin=margin, n_triples=n)


_MEASURED = []


def measured():
    if not _MEASURED:
        _MEASURED.append(measure())
    return _MEASURED[0]


def test_closed_form_agrees_with_the_independent_statement():
    """float M and N against nothing narrowed: the difference is the float rounding of M (2^-24 relative) through the conditioning of the
    triple, bounded here at 1e-3 for triples whose angle at the first point has a sine of 0.2 or more"""
    m = measured()
    print(m)
    assert m["n_triples"] >= 400 and m["spread"] < 1e-3


def test_noise_file_is_current_and_the_scenes_are_not_vacuous():
    gold = json.load(open(NOISE_PATH))
    m = measured()
    for k in ("spread_R", "spread_t", "spread_s", "spread"):
        assert m[k] <= 1.5 * gold[k] and gold[k] <= 1.5 * max(m[k], 1e-9), (k, m[k], gold[k])
    assert gold["n_triples"] == m["n_triples"] and abs(gold["min_margin"] - m["min_margin"]) <= 1e-3 * gold["min_margin"]
    assert m["min_margin"] > 64 * gold["spread"], "an err lies within 64 x the spread of its bound: %r vs %r" % (m["min_margin"], gold["spread"])


if __name__ == "__main__":
    if "--write" in sys.argv:
        with open(NOISE_PATH, "w") as f:
            json.dump(measure(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", NOISE_PATH)
