"""The 4-point EPnP hypotheses of ivf_tracker_solve_pnp (k_pnp_hyp, iv_slam_amd/csrc/ivf_pnp.hip) against tests/pnp_ref.py, through the
taps of ivf_test_pnp_hypotheses, on the scenes of tests/pnp_hyp_scenes.py.

Which basis of MtM's four-dimensional null space an SVD returns is rounding's choice, so the device's basis is taken as given -- after
checking that it IS such a basis -- and everything else is compared:
  sample     the four indices equal ransac_ref.sample_indices, exactly
  cws        basis-free: cws[0] is the centroid; cws[i] - cws[0] are eigenvectors of PW0^t PW0 (built in numpy) of squared length
             lambda_i / 4 with lambda descending, mutually orthogonal, their largest component positive
  basis      with M built in numpy from the DEVICE's cws: the four vectors are orthonormal, M v_i vanishes, the singular values are
             those of MtM with the four smallest at the bottom
  tail       pnp_ref.pose_tail on the device's cws and vectors: every candidate's betas before and after gauss_newton, R, t and err
             within max(8 x the floor of tests/golden/pnp_hyp_noise.json, 2^-40) relative (tests/test_pnp_hyp_cpu.py: how the floor is
             measured, what `relative` means per quantity, which results are left out).  8 is the margin of tests/test_gpu_sim3.py, for
             the same reason: the device differs from the restatement in libm, in product contraction and in the small SVDs only.
  choice     best follows PnPsolver.cc:522-524 on the device's own three err; hyp_poses is the float narrowing of Rs[best], ts[best] to
             the bit; hyp_ninliers is numpy's CheckInliers count under the f64 pose, exactly (no band: the pose is not narrowed)
  product    solve_pnp on the same inputs returns the same hyp_poses / hyp_ninliers byte for byte; nothing is written past mRansacMaxIts
             or for a bad record index
Every check runs on each frame in a call of its own and on all frames in one call.

BOUND = 64 x 2^-52 x n for an n-column matrix.  A backward-stable SVD returns the exact factors of A + E with |E| <= p(n) eps |A| for a
modest polynomial p (Golub & Van Loan, 5.4 / 8.6; for one-sided Jacobi, Demmel & Veselic 1992); 64 n stands for p(n) with room for the
numpy side's own rounding in forming A.  It bounds: the departure of V^t V from I; the eigen-residual |A c - lambda c| <= BOUND |A| |c|
of the 3 x 3 PW0^t PW0; |w_device - w_numpy| <= BOUND |MtM| (Weyl); |MtM v_i| <= BOUND |MtM| for the four null vectors.  The issue's
form, |M v_i| <= BOUND |M|, is the statement for an SVD of M itself; through MtM, as the reference computes it, theory gives only
|M v_i|^2 = v_i^t MtM v_i <= 2 |E|.  It is asserted as set: M has 8 rows, so MtM's null space is exact and far from the range, and both
back ends of the restatement reach 7e-16 on these scenes, 260 times under the bound.  Nothing here is measured on the device."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_hyp_scenes as HS
import pnp_ref as R
import pnp_scenes as S
from test_gpu_pnp import make_tracker, run_pnp
from test_gpu_track import iv  # noqa: F401  (the module fixture)
from test_pnp_hyp_cpu import bound_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPS = 2.0 ** -52
NOISE = json.load(open(os.path.join(ROOT, "tests", "golden", "pnp_hyp_noise.json")))
SC = HS.scenarios()
TAP = 140
TAP_FILL, POSE_FILL, INT_FILL = -77.0, 7.0, -7


def bound(n):
    return 64 * EPS * n


def run_taps(iv, sc, stream=False, tracker=None):
    """-> dict(taps [n, mi, 140] f64, hyp_pose [n, mi, 12] f32, hyp_n [n, mi] i32) as numpy, every buffer filled before the call"""
    import torch
    from iv_slam_amd import dist as ivd
    dev = torch.device("cuda:0")
    frames, nf, p = sc["frames"], sc["nf"], sc["params"]
    n = len(frames); mi = p["max_iterations"]
    block = torch.from_numpy(ivd.pack_records([dict(kps=f["kps"], desc=f["desc"], uright=f["uright"], depth=f["depth"]) for f in frames], nf).reshape(-1)).to(dev)
    tr = tracker or make_tracker(iv, nf, sc["max_pairs"])
    xw = np.zeros((n, nf, 3), F); has = np.zeros((n, nf), np.uint8)
    for k, f in enumerate(frames):
        xw[k, :f["n"]] = f["xw"]; has[k, :f["n"]] = f["has"]
    idx = [(n + 5 if k in sc["bad"] else k) for k in range(n)]
    d = dict(taps=torch.full((n, mi, TAP), TAP_FILL, dtype=torch.float64, device=dev),
             hyp_pose=torch.full((n, mi, 12), POSE_FILL, dtype=torch.float32, device=dev), hyp_n=torch.full((n, mi), INT_FILL, dtype=torch.int32, device=dev))
    ddraws = torch.from_numpy(np.ascontiguousarray(sc["draws"]).view(np.int32)).to(dev)
    st = torch.cuda.Stream() if stream else None
    if st is not None:
        st.wait_stream(torch.cuda.current_stream())
    tr.pnp_hypotheses(block, torch.tensor(idx, dtype=torch.int32, device=dev), torch.from_numpy(xw).to(dev), torch.from_numpy(has).to(dev), ddraws,
                      d["taps"], d["hyp_pose"], d["hyp_n"], max_iterations=mi, probability=p["probability"], min_inliers=p["min_inliers"],
                      epsilon=p["epsilon"], th2=p["th2"], stream_ptr=st.cuda_stream if st is not None else None)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def only(sc, k):
    """the scenario that holds frame k of sc alone"""
    return dict(sc, frames=[sc["frames"][k]], draws=sc["draws"][k:k + 1], bad=[0] if k in sc["bad"] else [], max_pairs=1)


_RUNS = {}


def device(iv, name, mode):
    """mode "all": every frame of the scenario in one call; "alone": one call per frame, stacked.  -> (taps call, solve_pnp call), once"""
    if (name, mode) not in _RUNS:
        sc = SC[name]
        if mode == "all":
            _RUNS[(name, mode)] = (run_taps(iv, sc), run_pnp(iv, sc))
        else:
            t = [run_taps(iv, only(sc, k)) for k in range(len(sc["frames"]))]; p = [run_pnp(iv, only(sc, k)) for k in range(len(sc["frames"]))]
            _RUNS[(name, mode)] = ({q: np.concatenate([r[q] for r in t]) for q in t[0]}, {q: np.concatenate([r[q] for r in p]) for q in p[0]})
    return _RUNS[(name, mode)]


def record(T):
    """one tap record -> dict in the layout of pnp_ref.pose_tail, plus sample, cws, vv, w"""
    c = T[76:139].reshape(3, 21)
    return dict(sample=T[0:4], cws=T[4:16].reshape(4, 3), vv=T[16:64].reshape(4, 12), w=T[64:76], betas0=c[:, 0:4], betas1=c[:, 4:8],
                R=c[:, 8:17].reshape(3, 3, 3), t=c[:, 17:20], err=c[:, 20], best=T[139])


def run_samples(sc):
    for k, it, smp in HS.samples(sc):
        _, X, uv, s2 = S.correspondences(sc["frames"][k])
        yield k, it, smp, X, uv, s2


MODES = ["alone", "all"]


@pytest.mark.parametrize("mode", MODES)
def test_sample_is_the_restatements(iv, mode):
    taps, _ = device(iv, "hyp", mode)
    n = 0
    for k, it, smp, _, _, _ in run_samples(SC["hyp"]):
        assert taps["taps"][k, it, 0:4].tolist() == [float(j) for j in smp], (k, it)
        n += 1
    assert n == 5 * 64 + 7 + 1


@pytest.mark.parametrize("mode", MODES)
def test_control_points_basis_free(iv, mode):
    """The taps hold cws[i] = cws[0] + c_i, not c_i: each entry is rounded at the size of cws, so c_i = cws[i] - cws[0] is known to
    delta = sqrt(3) * 2 eps * max|cws| only (one rounding of the sum per entry, doubled for the product before it), however short c_i
    is -- four nearly coplanar points 40 m away have a third axis of centimetres.  Each check allows what that moves it by, on top of
    BOUND: the residual |A c - lambda c| by 2 |A| delta, a scalar product by delta (|c_i| + |c_j|), a squared length by 8 |c| delta.
    Figures are printed as shares of what is allowed."""
    taps, _ = device(iv, "hyp", mode)
    b = bound(3)
    worst = np.zeros(4)
    for k, it, smp, X, _, _ in run_samples(SC["hyp"]):
        P = X[smp].astype(np.float64)
        cws = record(taps["taps"][k, it])["cws"]
        worst[0] = max(worst[0], np.abs(cws[0] - P.mean(0)).max() / (b * np.abs(P).max()))
        A = (P - cws[0]).T @ (P - cws[0])
        nA = np.linalg.norm(A, 2)
        lam = np.sort(np.linalg.eigvalsh(A))[::-1]
        c = cws[1:] - cws[0]
        ln = np.linalg.norm(c, axis=1)
        delta = np.sqrt(3.0) * 2 * EPS * np.abs(cws).max()
        for i in range(3):
            worst[1] = max(worst[1], np.linalg.norm(A @ c[i] - lam[i] * c[i]) / (b * nA * ln[i] + 2 * nA * delta))
            worst[2] = max(worst[2], abs(4 * (c[i] @ c[i]) - lam[i]) / (b * nA + 8 * ln[i] * delta))
            assert c[i][np.argmax(np.abs(c[i]))] > 0, (k, it, i, c[i])
            for j in range(i):
                worst[3] = max(worst[3], abs(c[i] @ c[j]) / (b * ln[i] * ln[j] + delta * (ln[i] + ln[j])))
        assert (worst <= 1.0).all(), (k, it, worst)
    print("cws (%s), as shares of the bound: centroid %.3g, eigen-residual %.3g, squared length %.3g, orthogonality %.3g" % ((mode,) + tuple(worst)))


@pytest.mark.parametrize("mode", MODES)
def test_basis_is_a_null_space_basis_of_numpys_M(iv, mode):
    taps, _ = device(iv, "hyp", mode)
    b = bound(12)
    worst = np.zeros(5)
    for k, it, smp, X, uv, _ in run_samples(SC["hyp"]):
        r = record(taps["taps"][k, it])
        P = X[smp].astype(np.float64)
        M = R.fill_M(R.barycentric(R.svd_numpy, r["cws"])(P), uv[smp].astype(np.float64), S.CAM)
        A = M.T @ M
        nM = np.linalg.norm(M, 2); nA = nM * nM
        worst[0] = max(worst[0], np.abs(r["vv"] @ r["vv"].T - np.eye(4)).max())
        worst[1] = max(worst[1], max(np.linalg.norm(M @ v) for v in r["vv"]) / nM)
        worst[2] = max(worst[2], max(np.linalg.norm(A @ v) for v in r["vv"]) / nA)
        assert (np.diff(r["w"]) <= 0).all(), "the singular values are in descending order"
        # numpy's M is not the device's to the bit: both solve CC alphas = p - cws[0], a 3 x 3 system of condition kappa (the longest over
        # the shortest control axis, 1e3 for four nearly coplanar points), each to 64 * 3 eps kappa relative; MtM doubles it
        kappa = np.linalg.cond((r["cws"][1:] - r["cws"][0]).T)
        worst[3] = max(worst[3], np.abs(r["w"] - np.linalg.svd(A, compute_uv=False)).max() / nA / (1 + 4 * 3 * kappa / 12))
        worst[4] = max(worst[4], r["w"][8:].max() / nA)
        assert r["w"][7] > 1e3 * b * nA, "M has rank 8 on these scenes: the four smallest are apart from the others"
        assert (worst <= b).all(), (k, it, worst, b)
    print("basis (%s): orthonormality %.3g, |M v| / |M| %.3g, |MtM v| / |MtM| %.3g, singular values %.3g, the four smallest %.3g (bound %.3g)"
          % ((mode,) + tuple(worst) + (b,)))


@pytest.mark.parametrize("mode", MODES)
def test_tail_follows_the_restatement_on_the_devices_basis(iv, mode):
    taps, _ = device(iv, "hyp", mode)
    bnd = bound_of(NOISE); left = {tuple(v) for v in NOISE["left_out"]}
    assert len(left) <= 0.01 * NOISE["n_results"] and (bnd >= 2.0 ** -40).all()
    worst = np.zeros(len(HS.QUANTITIES)); fails = []
    for k, it, smp, X, uv, _ in run_samples(SC["hyp"]):
        r = record(taps["taps"][k, it])
        want = R.pose_tail(X[smp], uv[smp], S.CAM, r["cws"], r["vv"])
        d = HS.tail_difference(want, r, uv[smp])
        for c in range(3):
            if (k, it, c) in left:
                continue
            worst = np.maximum(worst, d[c])
            if not (d[c] <= bnd).all():
                fails.append((SC["hyp"]["names"][k], it, c, d[c].tolist()))
    print("tail (%s): device minus restatement, largest relative difference / bound: %s"
          % (mode, ", ".join("%s %.3g / %.3g" % (q, w, b) for q, w, b in zip(HS.QUANTITIES, worst, bnd))))
    assert not fails, fails[:10]


@pytest.mark.parametrize("mode", MODES)
def test_choice_narrowing_and_inlier_count(iv, mode):
    taps, _ = device(iv, "hyp", mode)
    sc = SC["hyp"]
    for k, it, smp, X, uv, s2 in run_samples(sc):
        r = record(taps["taps"][k, it])
        best = R.choose_best(r["err"])
        assert r["best"] == float(best), (k, it, r["err"], r["best"])
        assert taps["hyp_pose"][k, it].tobytes() == R.pose12(r["R"][best], r["t"][best]).tobytes(), (k, it)
        mask, _ = R.check_inliers(r["R"][best], r["t"][best], X, uv, R.max_error(s2, sc["params"]["th2"]), S.CAM)
        assert taps["hyp_n"][k, it] == int(mask.sum()), (k, it, taps["hyp_n"][k, it], int(mask.sum()))


@pytest.mark.parametrize("mode", MODES)
def test_product_path_is_untouched_and_nothing_else_is_written(iv, mode):
    taps, prod = device(iv, "hyp", mode)
    sc = SC["hyp"]
    assert taps["hyp_pose"].tobytes() == prod["hyp_pose"].tobytes() and taps["hyp_n"].tobytes() == prod["hyp_n"].tobytes()
    for k, fr in enumerate(sc["frames"]):
        its = 0 if k in sc["bad"] else fr["max_its"]
        assert (taps["taps"][k, its:] == TAP_FILL).all() and (taps["hyp_pose"][k, its:] == POSE_FILL).all() and (taps["hyp_n"][k, its:] == INT_FILL).all(), k
        assert (taps["taps"][k, :its] != TAP_FILL).all(), "every double of a record that ran is written"
    assert prod["ninl"][5] == -1


def test_runs_are_bit_identical_alone_together_and_on_any_stream(iv):
    sc = SC["hyp"]
    a, _ = device(iv, "hyp", "all")
    b, _ = device(iv, "hyp", "alone")
    tr = make_tracker(iv, sc["nf"], sc["max_pairs"])
    c = run_taps(iv, sc, tracker=tr)
    d = run_taps(iv, sc, stream=True, tracker=tr)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), "%s differs between one call per frame and one call" % key
        assert a[key].tobytes() == c[key].tobytes(), "%s differs between two runs" % key
        assert a[key].tobytes() == d[key].tobytes(), "%s differs on a non-default stream" % key


@pytest.mark.parametrize("mode", MODES)
def test_degenerate_samples_return_and_are_self_consistent(iv, mode):
    """four coplanar points, three collinear points plus one, a sample that holds a NaN point: the call returns; every record is finite
    throughout, or not finite in any entry of any candidate's R, t and err with hyp_ninliers = 0.  A finite record obeys the choice
    checks.  Nothing is compared with the restatement."""
    taps, prod = device(iv, "degenerate", mode)
    sc = SC["degenerate"]
    assert taps["hyp_pose"].tobytes() == prod["hyp_pose"].tobytes() and taps["hyp_n"].tobytes() == prod["hyp_n"].tobytes()
    kinds = {}
    for k, it, smp, X, uv, s2 in run_samples(sc):
        T = taps["taps"][k, it]
        r = record(T)
        assert r["sample"].tolist() == [float(j) for j in smp]
        out = np.concatenate([r["R"].reshape(-1), r["t"].reshape(-1), r["err"]])
        name = sc["names"][k]
        if np.isfinite(T).all():
            best = R.choose_best(r["err"])
            assert r["best"] == float(best) and taps["hyp_pose"][k, it].tobytes() == R.pose12(r["R"][best], r["t"][best]).tobytes()
            mask, _ = R.check_inliers(r["R"][best], r["t"][best], X, uv, R.max_error(s2, sc["params"]["th2"]), S.CAM)
            assert taps["hyp_n"][k, it] == int(mask.sum()), (name, it)
            kinds.setdefault(name, set()).add(True)
        else:
            assert not np.isfinite(out).any(), "%s iteration %d: a record that is finite in part: %r" % (name, it, T)
            assert taps["hyp_n"][k, it] == 0 and not np.isfinite(taps["hyp_pose"][k, it]).any()
            kinds.setdefault(name, set()).add(False)
        if name == "nan_point":
            assert np.isfinite(T).all() == (2 not in smp), "the records that are not finite are those whose sample holds the NaN point"
    print("degenerate (%s): finite records per frame %r" % (mode, kinds))
    assert kinds["nan_point"] == {True, False}
