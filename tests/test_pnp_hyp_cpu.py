"""CPU side of the EPnP hypothesis tests: ivf_test_pnp_hypotheses is exported, bound, documented and checks its arguments without a GPU;
the tail of tests/pnp_ref.py (pose_tail: everything of compute_pose after the SVD of MtM, as a function of a GIVEN null-space basis) is
measured against itself on every sample of tests/pnp_hyp_scenes.py, and shown to tell each misreading of pnp_ref.MISREADINGS apart.

The floor (tests/golden/pnp_hyp_noise.json, written by `python tests/test_pnp_hyp_cpu.py --write`) is measured on the restatement alone,
never on the device.  For every sample the basis is null_basis() under numpy's SVD; the tail runs on it under both SVD back ends, and
again on that basis moved by one ulp per entry (4 runs).  The spread of a (sample, candidate) is the largest difference of a run to the
first, per quantity (betas before and after gauss_newton, R, t, err), relative to the quantity's own size -- for err relative to the
larger of err and the sample's largest image coordinate: err is a mean of distances between image coordinates, so its rounding error
scales with those coordinates and not with err, which is 1e-5 px on noise-free data.  A (sample, candidate) whose spread exceeds 1e-8
in any quantity is ill-conditioned and left out, at most 1 % of them; the floor of a quantity is the largest spread among the others.
tests/test_gpu_pnp_hyp.py allows the device max(8 x floor, 2^-40) and leaves out exactly the same results.

Power: for every misreading there is a named frame on which pose_tail(mis) differs from pose_tail() by more than that bound in a tapped
quantity of a result that is not left out (CAUGHT_BY).  For best_02 the difference is in `best`, on a sample whose two lowest err lie more
than 1e-6 apart.  best_le (the candidate chosen with <=) cannot differ from the reference's < on such a sample: the two comparisons
disagree on exact ties only, and no sample of the scenes has one (asserted).  It is told apart on hand-made err triples, which is also
what the device test's check of `best` against the device's own three err values covers."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_hyp_scenes as HS
import pnp_ref as R
import pnp_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_PATH = os.path.join(ROOT, "tests", "golden", "pnp_hyp_noise.json")
ILL, CAP, MARGIN, LEAST = 1e-8, 0.01, 8, 2.0 ** -40
SC = HS.scenarios()
# misreading -> the frame of the "hyp" scenario that is asserted to catch it (others may as well)
CAUGHT_BY = {"approx1_cols": "noise", "b0_branch_cand0": "noise", "b0_branch_cand12": "outliers", "no_b1_flip": "clean", "b3_undivided": "near",
             "gn_4_steps": "noise", "sign_last_point": "outliers", "det_row0": "turned", "best_02": "noise"}


def bound_of(gold):
    """the device test's bound per quantity"""
    return np.array([max(MARGIN * gold["floor"][q], LEAST) for q in HS.QUANTITIES])


def sample_inputs(sc, k, smp):
    _, X, uv, _ = S.correspondences(sc["frames"][k])
    return X[smp], uv[smp]


_BASE = {}


def base_results():
    """(k, it) -> (X, uv, cws, vv, the tail on that basis), once for the module"""
    if not _BASE:
        sc = SC["hyp"]
        for k, it, smp in HS.samples(sc):
            X, uv = sample_inputs(sc, k, smp)
            cws, vv, _, _ = R.null_basis(X, uv, S.CAM)
            _BASE[(k, it)] = (X, uv, cws, vv, R.pose_tail(X, uv, S.CAM, cws, vv))
    return _BASE


def measure():
    sc = SC["hyp"]
    floor = np.zeros(len(HS.QUANTITIES)); left_out = []; n = 0
    for (k, it), (X, uv, cws, vv, base) in sorted(base_results().items()):
        d = np.zeros((3, len(HS.QUANTITIES)))
        for backend in ("numpy", "jacobi"):
            for basis in (vv, HS.perturbed(vv, 1000 * k + it)):
                if backend == "numpy" and basis is vv:
                    continue
                d = np.maximum(d, HS.tail_difference(base, R.pose_tail(X, uv, S.CAM, cws, basis, backend), uv))
        for c in range(3):
            n += 1
            if not d[c].max() <= ILL:
                left_out.append([k, it, c])
            else:
                floor = np.maximum(floor, d[c])
    return dict(floor={q: float(v) for q, v in zip(HS.QUANTITIES, floor)}, left_out=left_out, n_results=n)


def test_entry_point_is_exported_bound_and_documented():
    from iv_slam_amd import _lib, track
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    name = "ivf_test_pnp_hypotheses"
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define IVF_PNP_TAP_DOUBLES (\d+)\s*int\s+%s\s*\(" % name, hdr, flags=re.S)
    assert m and "Testing hook" in m.group(1) and "ivf_tracker_solve_pnp" in m.group(1), "the header comment says what it is"
    assert int(m.group(2)) == track.PNP_TAP_DOUBLES == 4 + 12 + 48 + 12 + 3 * (4 + 4 + 9 + 3 + 1) + 1
    # the inputs of ivf_tracker_solve_pnp, then taps, hyp_poses, hyp_ninliers, stream
    assert _lib._SIGS[name][1][:14] == _lib._SIGS["ivf_tracker_solve_pnp"][1][:14] and len(_lib._SIGS[name][1]) == 18
    assert callable(track.BatchTracker.pnp_hypotheses)
    assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), "listed in INTEGRATION.md (as test-only)"


def test_argument_validation_without_gpu():
    from iv_slam_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    p = _lib.ptr(buf)
    one = C.c_void_p(16)                                                       # a non-null handle that must not be touched

    def call(t=one, rec=p, frames=p, xw=p, has=p, draws=p, mi=64, prob=0.99, mn=4, eps=0.1, th2=5.991, taps=p, poses=p, ninl=p):
        return lib.ivf_test_pnp_hypotheses(t, rec, 64, 1, frames, 1, xw, has, draws, mi, prob, mn, eps, th2, taps, poses, ninl, None)
    for kw in (dict(t=None), dict(rec=None), dict(frames=None), dict(xw=None), dict(has=None), dict(draws=None), dict(taps=None), dict(poses=None),
               dict(ninl=None), dict(mi=0), dict(mi=301), dict(prob=0.0), dict(prob=1.0), dict(eps=-0.1), dict(eps=1.5), dict(th2=0.0), dict(mn=-1)):
        assert call(**kw) == _lib.IVF_E_INVALID, kw


def test_the_scenes_are_what_they_say():
    sc = SC["hyp"]
    assert sc["nf"] == 64 and sc["params"]["max_iterations"] == 64 and [f["max_its"] for f in sc["frames"]] == [64, 64, 64, 64, 64, 64, 7, 1]
    fr = sc["frames"][2]
    idx = np.nonzero(fr["has"])[0]
    kinds = [sum(bool(fr["planted"][idx[j]]) for j in R.sample_indices(fr["N"], sc["draws"][2, it])) for it in range(6)]
    assert kinds == [4, 3, 2, 1, 0, 2], "the planted samples of the outlier frame mix inliers and outliers"
    T = sc["frames"][4]["pose_gt"].reshape(3, 4)
    assert abs(np.degrees(np.arccos((np.trace(T[:, :3]) - 1) / 2)) - 120.0) < 1e-9
    _, X, _, _ = S.correspondences(sc["frames"][3])
    Pc = X.astype(np.float64) @ sc["frames"][3]["pose_gt"].reshape(3, 4)[:, :3].T + sc["frames"][3]["pose_gt"].reshape(3, 4)[:, 3]
    assert 0.5 - 1e-3 <= Pc[:, 2].min() and Pc[:, 2].max() <= 2.0 + 1e-3
    # the clean frame reaches the planted pose with some sample, under the tail on the restatement's own basis
    hits = 0
    for (k, it), (X, uv, cws, vv, base) in base_results().items():
        if k == 0:
            T = sc["frames"][0]["pose_gt"].reshape(3, 4)
            hits += bool(np.abs(base["R"][base["best"]] - T[:, :3]).max() < 1e-3 and np.abs(base["t"][base["best"]] - T[:, 3]).max() < 1e-2)
    assert hits >= 16, hits
    dg = SC["degenerate"]
    for k, name in enumerate(dg["names"]):
        _, X, uv, _ = S.correspondences(dg["frames"][k])
        smp = R.sample_indices(dg["frames"][k]["N"], dg["draws"][k, 0])
        assert smp == dg["planted"][k][0]
        P = X[smp].astype(np.float64)
        if name == "coplanar":
            assert np.linalg.svd(P - P.mean(0), compute_uv=False)[2] < 1e-6
        elif name == "collinear":
            assert np.linalg.svd(P[:3] - P[:3].mean(0), compute_uv=False)[1] < 1e-6
        else:
            assert np.isnan(P).sum() == 1


def test_noise_floor_file_is_current_and_under_the_cap():
    gold = json.load(open(NOISE_PATH))
    m = measure()
    print("floor", m["floor"], "left out", m["left_out"], "of", m["n_results"])
    assert m["n_results"] == gold["n_results"] == 3 * sum(1 for _ in HS.samples(SC["hyp"]))
    assert len(m["left_out"]) <= CAP * m["n_results"], "more than 1 %% of the (sample, candidate) results are ill-conditioned: %r" % m["left_out"]
    assert m["left_out"] == gold["left_out"]
    for q in HS.QUANTITIES:
        assert m["floor"][q] <= gold["floor"][q] <= ILL, q


@pytest.mark.parametrize("mis", [m for m in R.MISREADINGS if m != "best_le"])
def test_a_named_frame_catches_the_misreading(mis):
    gold = json.load(open(NOISE_PATH))
    bound = bound_of(gold); left = {tuple(v) for v in gold["left_out"]}
    sc = SC["hyp"]
    caught = {}
    for (k, it), (X, uv, cws, vv, base) in sorted(base_results().items()):
        wrong = R.pose_tail(X, uv, S.CAM, cws, vv, mis=[mis])
        if mis == "best_02":
            e = np.sort(base["err"])
            hit = np.isfinite(e).all() and e[1] - e[0] > 1e-6 * e[1] and wrong["best"] != base["best"] and all((k, it, c) not in left for c in range(3))
        else:
            d = HS.tail_difference(base, wrong, uv)
            hit = any((d[c] > bound).any() and (k, it, c) not in left for c in range(3))
        if hit:
            caught[sc["names"][k]] = caught.get(sc["names"][k], 0) + 1
    print(mis, caught)
    assert caught.get(CAUGHT_BY[mis], 0) >= 1, (mis, caught)


def test_best_le_differs_on_exact_ties_only():
    for err, lt, le in (((1.0, 1.0, 2.0), 0, 1), ((2.0, 1.0, 1.0), 1, 2), ((1.0, 2.0, 1.0), 0, 2), ((1.0, 1.0, 1.0), 0, 2)):
        assert (R.choose_best(err) == lt and R.choose_best(err, {"best_le"}) == le), err
    rng = np.random.default_rng(4)
    for _ in range(200):
        err = rng.uniform(0, 5, 3)
        assert R.choose_best(err) == R.choose_best(err, {"best_le"}) == int(np.argmin(err))
    nan = float("nan")
    assert R.choose_best((nan, 1.0, 2.0)) == R.choose_best((nan, 1.0, 2.0), {"best_le"}) == 0, "a NaN rep_errors[0] keeps candidate 0 or 2"
    assert R.choose_best((1.0, nan, 0.5)) == 2 and R.choose_best((1.0, 0.5, nan)) == 1
    for (k, it), (_, _, _, _, base) in base_results().items():
        e = base["err"]
        assert len(set(e.tolist())) == 3 or not np.isfinite(e).all(), "an exact tie of two err values in frame %d iteration %d" % (k, it)


if __name__ == "__main__":
    if "--write" in sys.argv:
        m = measure()
        with open(NOISE_PATH, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", NOISE_PATH, m)
