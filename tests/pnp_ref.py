"""pnp_ref.py -- numpy f64 restatement of PnPsolver (ORB/src/PnPsolver.cc) as Tracking::Relocalization drives it (test infrastructure
only): SetRansacParameters (:125-161), the sampling of :192-205 on given rand() values, compute_pose and everything under it
(:379-530, :554-956), CheckInliers with its float / double mix (:312-343), Refine (:264-309) and the bookkeeping of iterate (:213-259).
It is the yardstick of ivf_tracker_solve_pnp (iv_slam_amd/csrc/ivf_pnp.hip); OpenCV is not needed.

cvSVD / cvInvert / cvSolve(CV_SVD) have two interchangeable back ends: "numpy" (numpy.linalg.svd) and "jacobi" (a plain cyclic one-sided
Jacobi written below).  A 4-point hypothesis has an 8x12 M, so MtM has a four-dimensional null space whose basis rounding chooses: two
correct back ends may return different poses for the same sample.  compute_pose on >= 11 non-planar points (Refine) is comparable as a
whole.  Of a hypothesis, everything but that basis is: pose_tail() is compute_pose after the SVD of MtM as a function of a GIVEN basis
(well conditioned: tests/test_pnp_hyp_cpu.py measures its spread), null_basis() what comes before.  tests/test_gpu_pnp_hyp.py takes the
device's basis from the taps of ivf_test_pnp_hypotheses, checks that it is a null-space basis of the M numpy builds, and replays the tail
on it; which basis of that space the device's SVD chose is the one thing still taken as given."""
import itertools
import math

import numpy as np

from ransac_ref import RAND_MAX, draws_for, iteration_count, level_sigma2, random_int, sample_indices as _sample_indices  # noqa: F401  (R.random_int, ...)

D = np.float64
F = np.float32
EPS = 2.0 ** -52


# ---- the SVD back ends: svd(A) -> (U, w, V) with A = U diag(w) V^T, w descending, V orthonormal --------------------------------------
def svd_numpy(A):
    A = np.asarray(A, D)
    if not np.isfinite(A).all():
        n = A.shape[1]
        return np.full(A.shape, np.nan), np.full(n, np.nan), np.full((n, n), np.nan)
    U, w, Vt = np.linalg.svd(A, full_matrices=False)
    return U, w, Vt.T


def svd_jacobi(A, sweeps=30):
    A = np.array(A, D)
    m, n = A.shape
    V = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    x = A[:, p]; y = A[:, q]
                    a = float(x @ x); b = float(y @ y); g = float(x @ y)
                    if not abs(g) > EPS * math.sqrt(a * b):
                        continue
                    rotated = True
                    zeta = (b - a) / (2.0 * g)
                    t = math.copysign(1.0, zeta) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / math.sqrt(1.0 + t * t); s = c * t
                    A[:, p], A[:, q] = c * x - s * y, s * x + c * y
                    vx = V[:, p].copy(); vy = V[:, q].copy()
                    V[:, p], V[:, q] = c * vx - s * vy, s * vx + c * vy
            if not rotated:
                break
        w = np.sqrt((A * A).sum(0))
        order = sorted(range(n), key=lambda j: -w[j] if w[j] == w[j] else 0.0)
        w = w[order]; A = A[:, order]; V = V[:, order]
        U = A / w
        if m == 3 and n == 3 and not w[2] > 2 * EPS * w.sum():
            U[:, 2] = np.cross(U[:, 0], U[:, 1])
    return U, w, V


BACKENDS = {"numpy": svd_numpy, "jacobi": svd_jacobi}


def pinv_solve(svd, A, b):
    """cvSolve(A, b, x, CV_SVD) / cvInvert(CV_SVD): SVD::backSubst, singular values at or below 2 eps sum(w) dropped"""
    U, w, V = svd(A)
    with np.errstate(all="ignore"):
        keep = w > 2 * EPS * w.sum()
        d = np.where(keep, (U.T @ b).T / np.where(keep, w, 1.0), 0.0).T
    return V @ d


# ---- RANSAC parameters and sampling ---------------------------------------------------------------------------------------------------
def ransac_parameters(N, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, min_set=4):
    """-> (mRansacMinInliers, mRansacMaxIts, x) with mRansacMaxIts = 0 for the early refusal N < mRansacMinInliers (:177-181);
    x = the real number whose ceil is taken (None where there is none)"""
    eps = F(epsilon)
    n_min = int(F(N) * eps)
    n_min = max(n_min, int(min_inliers), int(min_set))
    if N < n_min:
        return n_min, 0, None
    if eps < F(n_min) / F(N):
        eps = F(n_min) / F(N)
    return (n_min,) + iteration_count(probability, eps, n_min == N, max_iterations)


def sample_indices(N, draws4, min_set=4, mis=()):
    """:192-205 (ransac_ref.sample_indices with the four points of minSet)"""
    return _sample_indices(N, draws4, min_set, mis)


# ---- CheckInliers -------------------------------------------------------------------------------------------------------------------------
def check_inliers(R, t, X, uv, max_err, cam):
    """R [3,3], t [3] double; X [N,3], uv [N,2], max_err [N] float -> (mask, error2 float).  Xc, Yc, invZc, distX, distY, error2 are float
    (rounded from double expressions), ue and ve double."""
    R = np.asarray(R, D); t = np.asarray(t, D)
    X = np.asarray(X, F).astype(D); uv32 = np.asarray(uv, F)
    fu, fv, uc, vc = (D(F(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        Xc = (((R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1]) + R[0, 2] * X[:, 2]) + t[0]).astype(F)
        Yc = (((R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1]) + R[1, 2] * X[:, 2]) + t[1]).astype(F)
        invZc = (1 / (((R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1]) + R[2, 2] * X[:, 2]) + t[2])).astype(F)
        ue = uc + fu * Xc.astype(D) * invZc.astype(D)
        ve = vc + fv * Yc.astype(D) * invZc.astype(D)
        dx = (uv32[:, 0].astype(D) - ue).astype(F)
        dy = (uv32[:, 1].astype(D) - ve).astype(F)
        e2 = (dx * dx + dy * dy).astype(F)
        mask = e2 < np.asarray(max_err, F)
    return mask, e2


def max_error(sigma2, th2):
    return (np.asarray(sigma2, F) * F(th2)).astype(F)


# ---- EPnP ---------------------------------------------------------------------------------------------------------------------------------
def qr_solve(A, b, x):
    """:864-954 as written there (the pivot scale eta looks at rows k .. nr - 2 of column k); x is left alone when A is singular"""
    a = np.array(A, D); b = np.array(b, D)
    nr, nc = a.shape
    A1 = np.zeros(nc); A2 = np.zeros(nc)
    with np.errstate(all="ignore"):
        for k in range(nc):
            eta = abs(a[k, k])
            for i in range(k + 1, nr):
                elt = abs(a[i - 1, k])
                if eta < elt:
                    eta = elt
            if eta == 0:
                return x
            inv_eta = 1. / eta
            s = 0.0
            for i in range(k, nr):
                a[i, k] = a[i, k] * inv_eta
                s = s + a[i, k] * a[i, k]
            sigma = math.sqrt(s) if s >= 0 else float("nan")
            if a[k, k] < 0:
                sigma = -sigma
            a[k, k] = a[k, k] + sigma
            A1[k] = sigma * a[k, k]
            A2[k] = -eta * sigma
            for j in range(k + 1, nc):
                s2 = 0.0
                for i in range(k, nr):
                    s2 = s2 + a[i, k] * a[i, j]
                tau = s2 / A1[k]
                for i in range(k, nr):
                    a[i, j] = a[i, j] - tau * a[i, k]
        for j in range(nc):
            tau = 0.0
            for i in range(j, nr):
                tau = tau + a[i, j] * b[i]
            tau = tau / A1[j]
            for i in range(j, nr):
                b[i] = b[i] - tau * a[i, j]
        x = np.array(x, D)
        x[nc - 1] = b[nc - 1] / A2[nc - 1]
        for i in range(nc - 2, -1, -1):
            s = 0.0
            for j in range(i + 1, nc):
                s = s + a[i, j] * x[j]
            x[i] = (b[i] - s) / A2[i]
    return x


def gauss_newton(L, rho, betas, steps=5):
    bt = np.array(betas, D)
    x = np.zeros(4)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            A = np.zeros((6, 4)); b = np.zeros(6)
            for i in range(6):
                r = L[i]
                A[i, 0] = 2 * r[0] * bt[0] + r[1] * bt[1] + r[3] * bt[2] + r[6] * bt[3]
                A[i, 1] = r[1] * bt[0] + 2 * r[2] * bt[1] + r[4] * bt[2] + r[7] * bt[3]
                A[i, 2] = r[3] * bt[0] + r[4] * bt[1] + 2 * r[5] * bt[2] + r[8] * bt[3]
                A[i, 3] = r[6] * bt[0] + r[7] * bt[1] + r[8] * bt[2] + 2 * r[9] * bt[3]
                b[i] = rho[i] - (r[0] * bt[0] * bt[0] + r[1] * bt[0] * bt[1] + r[2] * bt[1] * bt[1] + r[3] * bt[0] * bt[2] + r[4] * bt[1] * bt[2] +
                                 r[5] * bt[2] * bt[2] + r[6] * bt[0] * bt[3] + r[7] * bt[1] * bt[3] + r[8] * bt[2] * bt[3] + r[9] * bt[3] * bt[3])
            x = qr_solve(A, b, x)
            bt = bt + x
    return bt


def canonical_signs(V):
    """The principal axes of choose_control_points come out of an SVD with either sign, and EPnP's answer on noisy data depends on it (the
    control points are mirrored, the norm it minimises under changes).  cvSVD's choice is an accident of its rotations; this restatement and
    the kernel both turn every axis so that its component of largest magnitude (the first such) is positive."""
    V = np.array(V, D)
    for i in range(V.shape[1]):
        a = np.abs(V[:, i])
        j = int(np.argmax(a)) if np.isfinite(a).all() else 0
        if V[j, i] < 0:
            V[:, i] = -V[:, i]
    return V


PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


# Wrong readings of PnPsolver.cc that pose_tail(mis={...}) injects; tests/test_pnp_hyp_cpu.py shows that each one moves a tapped quantity of
# some named scene by more than the bound of tests/test_gpu_pnp_hyp.py.
MISREADINGS = ("approx1_cols",        # find_betas_approx_1 on columns 0, 1, 2, 3 of L_6x10 instead of 0, 1, 3, 6 (:677-683)
               "b0_branch_cand0",     # find_betas_approx_1 without its b[0] < 0 branch (:688-693): the signs of betas 1..3 not turned
               "b0_branch_cand12",    # find_betas_approx_2 / _3 without theirs (:721-727, :751-757): betas[1] from b[2] > 0 only
               "no_b1_flip",          # if (b[1] < 0) betas[0] = -betas[0] dropped (:729, :759)
               "b3_undivided",        # betas[2] = b[3] instead of b[3] / betas[0] (:761)
               "gn_4_steps",          # four Gauss-Newton steps instead of five (:849)
               "sign_last_point",     # solve_for_sign on the last point's pcs[2] instead of the first's (:642)
               "det_row0",            # the determinant fix applied to row 0 of R instead of row 2 (:616-620)
               "best_le",             # the best candidate chosen with <= (:522-524)
               "best_02")             # the best candidate chosen from rep_errors[0] and [2] only


def choose_best(err, mis=()):
    """:522-524: N = 1, if (rep_errors[2] < rep_errors[1]) N = 2, ... as the three-way strict comparison it amounts to"""
    lt = (lambda a, b: a <= b) if "best_le" in mis else (lambda a, b: a < b)
    best = 0
    if "best_02" not in mis and lt(err[1], err[0]):
        best = 1
    if lt(err[2], err[best]):
        best = 2
    return best


def control_points(svd, pw):
    """choose_control_points (:379-413) -> cws [4,3]"""
    n = len(pw)
    cws = np.zeros((4, 3))
    cws[0] = pw.sum(0) / n
    pw0 = pw - cws[0]
    _, dc, uc_t = svd(pw0.T @ pw0)
    uc_t = canonical_signs(uc_t)
    for i in range(1, 4):
        cws[i] = cws[0] + math.sqrt(dc[i - 1] / n) * uc_t[:, i - 1] if dc[i - 1] >= 0 else np.nan
    return cws


def barycentric(svd, cws):
    """compute_barycentric_coordinates (:415-437) -> the function p [k,3] -> alphas [k,4]"""
    cc = (cws[1:] - cws[0]).T
    ci = pinv_solve(svd, cc, np.eye(3))

    def alphas_of(p):
        a = np.zeros((len(p), 4))
        d = p - cws[0]
        for j in range(3):
            a[:, 1 + j] = (ci[j, 0] * d[:, 0] + ci[j, 1] * d[:, 1]) + ci[j, 2] * d[:, 2]
        a[:, 0] = ((1.0 - a[:, 1]) - a[:, 2]) - a[:, 3]
        return a
    return alphas_of


def fill_M(al, us, cam):
    """fill_M (:440-455) -> M [2n,12]"""
    fu, fv, uc, vc = (D(F(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    M = np.zeros((2 * len(al), 12))
    for i in range(4):
        M[0::2, 3 * i] = al[:, i] * fu; M[0::2, 3 * i + 2] = al[:, i] * (uc - us[:, 0])
        M[1::2, 3 * i + 1] = al[:, i] * fv; M[1::2, 3 * i + 2] = al[:, i] * (vc - us[:, 1])
    return M


def pose_tail(X, uv, cam, cws, vv, backend="numpy", perm=None, mis=()):
    """Everything of compute_pose after the SVD of MtM (:505-524), as a function of a GIVEN basis: the correspondences X [n,3] float,
    uv [n,2] float, the control points cws [4,3] and the four vectors vv [4,12] (vv[i] = ut + 12 * (11 - i)).  compute_L_6x10, compute_rho,
    the three find_betas_approx, gauss_newton, compute_R_and_t, reprojection_error, the choice.  -> dict(betas0 [3,4] (before
    gauss_newton), betas1 [3,4] (after it), R [3,3,3], t [3,3], err [3], best).  perm as in compute_pose; mis: MISREADINGS."""
    svd = BACKENDS[backend]
    mis = frozenset(mis)
    assert mis <= set(MISREADINGS), mis
    pw = np.asarray(X, F).astype(D); us = np.asarray(uv, F).astype(D)
    n = len(pw)
    first = pw[-1].copy() if "sign_last_point" in mis else pw[0].copy()
    if perm is not None:
        pw = pw[perm]; us = us[perm]
    cws = np.asarray(cws, D); v = [np.asarray(vv[i], D) for i in range(4)]
    fu, fv, uc, vc = (D(F(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    out = dict(betas0=np.zeros((3, 4)), betas1=np.zeros((3, 4)), R=np.zeros((3, 3, 3)), t=np.zeros((3, 3)), err=np.zeros(3))
    with np.errstate(all="ignore"):
        alphas_of = barycentric(svd, cws)
        al = alphas_of(pw)
        # compute_L_6x10, compute_rho
        L = np.zeros((6, 10)); rho = np.zeros(6)
        for i, (a, b) in enumerate(PAIRS):
            dv = [v[k][3 * a:3 * a + 3] - v[k][3 * b:3 * b + 3] for k in range(4)]
            L[i] = [dv[0] @ dv[0], 2.0 * (dv[0] @ dv[1]), dv[1] @ dv[1], 2.0 * (dv[0] @ dv[2]), 2.0 * (dv[1] @ dv[2]), dv[2] @ dv[2],
                    2.0 * (dv[0] @ dv[3]), 2.0 * (dv[1] @ dv[3]), 2.0 * (dv[2] @ dv[3]), dv[3] @ dv[3]]
            rho[i] = ((cws[a] - cws[b]) ** 2).sum()
        a_first = alphas_of(first[None])[0]
        for cand, cols in enumerate(([0, 1, 2, 3] if "approx1_cols" in mis else [0, 1, 3, 6], [0, 1, 2], [0, 1, 2, 3, 4])):
            b = pinv_solve(svd, L[:, cols], rho)
            bt = np.zeros(4)
            neg = b[0] < 0 and ("b0_branch_cand0" if cand == 0 else "b0_branch_cand12") not in mis
            if cand == 0:
                if neg:
                    bt[0] = math.sqrt(-b[0]); bt[1:] = -b[1:] / bt[0]
                else:
                    bt[0] = math.sqrt(b[0]) if b[0] >= 0 else np.nan; bt[1:] = b[1:] / bt[0]
            else:
                if neg:
                    bt[0] = math.sqrt(-b[0]); bt[1] = math.sqrt(-b[2]) if b[2] < 0 else 0.0
                else:
                    bt[0] = math.sqrt(b[0]) if b[0] >= 0 else np.nan; bt[1] = math.sqrt(b[2]) if b[2] > 0 else 0.0
                if b[1] < 0 and "no_b1_flip" not in mis:
                    bt[0] = -bt[0]
                bt[2] = 0.0 if cand == 1 else (b[3] if "b3_undivided" in mis else b[3] / bt[0])
            out["betas0"][cand] = bt
            bt = gauss_newton(L, rho, bt, 4 if "gn_4_steps" in mis else 5)
            out["betas1"][cand] = bt
            # compute_ccs, compute_pcs, solve_for_sign
            ccs = np.zeros((4, 3))
            for i in range(4):
                ccs = ccs + bt[i] * v[i].reshape(4, 3)
            if a_first @ ccs[:, 2] < 0.0:
                ccs = -ccs
            pcs = al @ ccs
            # estimate_R_and_t
            pc0 = pcs.sum(0) / n; pwc = cws[0]
            abt = (pcs - pc0).T @ (pw - pwc)
            U, _, Vv = svd(abt)
            R = U @ Vv.T
            if np.linalg.det(R) < 0 if np.isfinite(R).all() else False:
                k = 0 if "det_row0" in mis else 2
                R[k] = -R[k]
            t = pc0 - R @ pwc
            # reprojection_error
            Pc = pw @ R.T + t
            inv = 1.0 / Pc[:, 2]
            ue = uc + fu * Pc[:, 0] * inv; ve = vc + fv * Pc[:, 1] * inv
            out["R"][cand] = R; out["t"][cand] = t
            out["err"][cand] = np.sqrt((us[:, 0] - ue) ** 2 + (us[:, 1] - ve) ** 2).sum() / n
        out["best"] = choose_best(out["err"], mis)
    return out


def null_basis(X, uv, cam, backend="numpy", perm=None):
    """compute_pose up to the SVD of MtM (:485-503) -> (cws [4,3], vv [4,12], the 12 singular values of MtM descending, M [2n,12])"""
    svd = BACKENDS[backend]
    pw = np.asarray(X, F).astype(D); us = np.asarray(uv, F).astype(D)
    if perm is not None:
        pw = pw[perm]; us = us[perm]
    with np.errstate(all="ignore"):
        cws = control_points(svd, pw)
        M = fill_M(barycentric(svd, cws)(pw), us, cam)
        _, w, V = svd(M.T @ M)
    return cws, np.stack([V[:, 11 - i] for i in range(4)]), w, M


def compute_pose(X, uv, cam, backend="numpy", perm=None):
    """compute_pose (:481-529) on the correspondences X [n,3] float, uv [n,2] float -> (R [3,3], t [3], reprojection error).
    perm: an order of the points for the sums over them (the first point, whose pcs[2] decides the sign, stays the first)."""
    cws, vv, _, _ = null_basis(X, uv, cam, backend, perm)
    o = pose_tail(X, uv, cam, cws, vv, backend, perm)
    return o["R"][o["best"]], o["t"][o["best"]], o["err"][o["best"]]


def pose12(R, t):
    """the float [12] pose a solver returns (:221-227, :298-304)"""
    T = np.zeros((3, 4), F)
    with np.errstate(all="ignore"):
        T[:, :3] = np.asarray(R, D).astype(F); T[:, 3] = np.asarray(t, D).astype(F)
    return T.reshape(12)


# ---- Refine and iterate ------------------------------------------------------------------------------------------------------------------
def refine(X, uv, max_err, cam, best_mask, n_min, backend="numpy", perm=None):
    """-> (success, R, t, mask, count)"""
    idx = np.nonzero(best_mask)[0]
    R, t, _ = compute_pose(X[idx], uv[idx], cam, backend, perm)
    mask, _ = check_inliers(R, t, X, uv, max_err, cam)
    return int(mask.sum()) > n_min, R, t, mask, int(mask.sum())


def replay(X, uv, max_err, cam, n_min, max_its, hyp_masks, hyp_counts, hyp_pose12, backend="numpy", on_refine=None):
    """the bookkeeping of :213-259 over given hypotheses (mask, count and float pose per iteration), with this file's Refine.
    -> dict(pose [12] float or None, mask, ninliers, iterations, refined, best_it)"""
    best = 0; best_it = -1
    failed_for = -2
    for it in range(max_its):
        if hyp_counts[it] >= n_min:
            if hyp_counts[it] > best:
                best = int(hyp_counts[it]); best_it = it
            if failed_for != best_it:                                    # Refine on an unchanged mvbBestInliers repeats itself
                ok, R, t, mask, cnt = refine(X, uv, max_err, cam, hyp_masks[best_it], n_min, backend)
                if on_refine:
                    on_refine(it, ok, R, t, mask)
                if ok:
                    return dict(pose=pose12(R, t), R=R, t=t, mask=mask, ninliers=cnt, iterations=it + 1, refined=True, best_it=best_it)
                failed_for = best_it
    if best >= n_min and best_it >= 0:
        return dict(pose=np.asarray(hyp_pose12[best_it], F), mask=np.asarray(hyp_masks[best_it], bool), ninliers=best, iterations=max_its,
                    refined=False, best_it=best_it)
    return dict(pose=None, mask=np.zeros(len(X), bool), ninliers=0, iterations=max_its, refined=False, best_it=-1)


def solve(X, uv, sigma2, cam, draws, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, backend="numpy"):
    """iterate() run to completion on the correspondences X, uv, sigma2 (in keypoint order) with the rand() values draws [max_iterations, 4]"""
    N = len(X)
    n_min, its, _ = ransac_parameters(N, probability, min_inliers, max_iterations, epsilon)
    if its == 0:
        return dict(pose=None, mask=np.zeros(N, bool), ninliers=0, iterations=0, refined=False, best_it=-1, n_min=n_min, max_its=0)
    me = max_error(sigma2, th2)
    masks, counts, poses = [], [], []
    out = None
    # hypotheses are computed lazily in order; the replay stops at the first successful Refine
    best = 0; best_it = -1; failed_for = -2
    for it in range(its):
        idx = sample_indices(N, draws[it])
        R, t, _ = compute_pose(X[idx], uv[idx], cam, backend)
        m, _ = check_inliers(R, t, X, uv, me, cam)
        masks.append(m); counts.append(int(m.sum())); poses.append(pose12(R, t))
        if counts[it] >= n_min:
            if counts[it] > best:
                best = counts[it]; best_it = it
            if failed_for != best_it:
                ok, R2, t2, m2, c2 = refine(X, uv, me, cam, masks[best_it], n_min, backend)
                if ok:
                    out = dict(pose=pose12(R2, t2), R=R2, t=t2, mask=m2, ninliers=c2, iterations=it + 1, refined=True, best_it=best_it)
                    break
                failed_for = best_it
    if out is None:
        if best >= n_min and best_it >= 0:
            out = dict(pose=poses[best_it], mask=masks[best_it], ninliers=best, iterations=its, refined=False, best_it=best_it)
        else:
            out = dict(pose=None, mask=np.zeros(N, bool), ninliers=0, iterations=its, refined=False, best_it=-1)
    out.update(n_min=n_min, max_its=its)
    return out


def subsets(items, k):
    return itertools.combinations(items, k)
