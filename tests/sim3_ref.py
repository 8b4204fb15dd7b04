"""sim3_ref.py -- plain numpy restatement of Sim3Solver (ORB/src/Sim3Solver.cc) as LoopClosing::ComputeSim3 drives it (test infrastructure
only), line by line: the constructor (:40-115), SetRansacParameters (:117-141), the sampling of :166-180 on given rand() values, ComputeSim3
(:229-340), CheckInliers (:343-367) with Project / FromCameraToImage (:385-426) and the bookkeeping of iterate (:143-210), with the
arithmetic DESIGN.md A-15 freezes (CV_32F products, dot, norm, reduce: double accumulation, one narrowing; M and N float; cv::eigen = the
cyclic two-sided Jacobi below, same pair order and sweep cap as iv_slam_amd/csrc/ivf_sim3.hip; atan2, norm, cv::Rodrigues in double).  It
is the yardstick of ivf_tracker_solve_sim3; OpenCV is not needed.

A keyframe here is dict(kps, n, pose (12 floats, Tcw row-major 3x4), xw [n,3], flags [n]): bit 0 of a flag = the keypoint holds a live
map point.  solve() reports a stage code per KF1 keypoint, an info record per iteration it ran, and the state the next call resumes from.

MISREADINGS names wrong readings of the reference that solve(mis={...}) injects; tests/test_sim3_cpu.py checks that each one is caught by
a named scene of tests/sim3_scenes.py."""
import math

import numpy as np

from ransac_ref import RAND_MAX, draws_for, iteration_count, level_sigma2, random_int, sample_indices as _sample_indices  # noqa: F401  (R.random_int, ...)

D = np.float64
F = np.float32
EPS = 2.0 ** -52
SWEEPS = 30

NO_MATCH, NO_POINT1, NO_POINT2, BAD, INLIER, FAIL_ERR1, FAIL_ERR2 = range(7)
STAGE_NAMES = ("no match", "no point on side 1", "no point on side 2", "bad (i2 names no keypoint of KF2)", "inlier", "failed err1", "failed err2")

MISREADINGS = {
    "float_threshold": "mvnMaxError = 9.21 * sigma2 as a float instead of the truncated integer (:90-91)",
    "best_strict": "the best is replaced on > instead of >= (:186)",
    "success_nonstrict": "success on >= mRansacMinInliers instead of > (:195)",
    "return_best": "the best hypothesis is returned without a success (:209)",
    "no_swap": "the drawn index is erased in order instead of swapped with the back (:178-179)",
    "z_sign": "a point with z <= 0 is refused by Project / FromCameraToImage (:400, :420)",
    "scale_not_fixed": "the scale is estimated under mbFixScale (:295-314)",
    "t21_not_inverted": "mT21i = mT12i (:333-339)",
    "state_not_resumed": "mnIterations and mnBestInliers start from 0 in every call (:41, :161)",
}


def max_error(sigma2, mis=()):
    """mvnMaxError (:87-91): 9.210 * sigmaSquare in double, truncated into a size_t; compared as float (:359)"""
    v = 9.210 * float(F(sigma2))
    return F(v) if "float_threshold" in mis else F(int(v))


def dot3(a, b):
    return (float(a[0]) * float(b[0]) + float(a[1]) * float(b[1])) + float(a[2]) * float(b[2])


def mul_add(R, x, t):
    """Rcw * x + tcw on CV_32F: per row the double sum of the three products plus t, narrowed once"""
    return np.array([F(dot3(R[i], x) + float(t[i])) for i in range(3)], F)


def to_image(Xc, cam, mis=()):
    """FromCameraToImage (:418-424) / the tail of Project (:400-404): invz = 1 / z, no test of its sign, all in float"""
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        if "z_sign" in mis and not Xc[2] > 0:
            return F(np.nan), F(np.nan)
        invz = F(1) / F(Xc[2])
        x = F(Xc[0]) * invz; y = F(Xc[1]) * invz
        return F(F(fx * x) + cx), F(F(fy * y) + cy)


def split_pose(pose12):
    T = np.asarray(pose12, F).reshape(3, 4)
    return T[:, :3].copy(), T[:, 3].copy()


# ---- the constructor (:40-115) -----------------------------------------------------------------------------------------------------------
def construct(kf1, kf2, match12, cam, sigma2, mis=()):
    """-> dict(idx1, idx2, X1, X2 [N,3] float, e1, e2 [N] float (the integer bounds), im1, im2 [N,2] float, stage [n1])"""
    R1, t1 = split_pose(kf1["pose"]); R2, t2 = split_pose(kf2["pose"])
    n1, n2 = kf1["n"], kf2["n"]
    stage = np.full(n1, NO_MATCH, np.int32)
    idx1, idx2, X1, X2, e1, e2, im1, im2 = [], [], [], [], [], [], [], []
    for i1 in range(n1):
        i2 = int(match12[i1])
        if i2 < 0:
            continue
        if i2 >= n2:
            stage[i1] = BAD
            continue
        if not kf1["flags"][i1] & 1:
            stage[i1] = NO_POINT1
            continue
        if not kf2["flags"][i2] & 1:
            stage[i1] = NO_POINT2
            continue
        a = mul_add(R1, kf1["xw"][i1], t1); b = mul_add(R2, kf2["xw"][i2], t2)
        idx1.append(i1); idx2.append(i2); X1.append(a); X2.append(b)
        e1.append(max_error(sigma2[min(max(int(kf1["kps"]["octave"][i1]), 0), len(sigma2) - 1)], mis))
        e2.append(max_error(sigma2[min(max(int(kf2["kps"]["octave"][i2]), 0), len(sigma2) - 1)], mis))
        im1.append(to_image(a, cam, mis)); im2.append(to_image(b, cam, mis))
        stage[i1] = INLIER                                                   # collected; CheckInliers decides below
    arr = lambda v, shape: np.array(v, F).reshape(shape)
    return dict(idx1=np.array(idx1, np.int64), idx2=np.array(idx2, np.int64), X1=arr(X1, (-1, 3)), X2=arr(X2, (-1, 3)), e1=arr(e1, (-1,)),
                e2=arr(e2, (-1,)), im1=arr(im1, (-1, 2)), im2=arr(im2, (-1, 2)), stage=stage)


# ---- SetRansacParameters (:117-141) and the sampling (:166-180) ---------------------------------------------------------------------------
def ransac_iterations(N, probability=0.99, min_inliers=20, max_iterations=300):
    """-> (mRansacMaxIts, x): 0 for the early refusal of iterate (:149-153; also N < 3, where there is no sample to draw); x = the real
    number whose ceil is taken (None where there is none)"""
    if N < min_inliers or N < 3:
        return 0, None
    return iteration_count(probability, F(min_inliers) / F(N), min_inliers == N, max_iterations)


def sample_indices(N, draws3, mis=()):
    """:166-180 (ransac_ref.sample_indices with the three point pairs of a hypothesis)"""
    return _sample_indices(N, draws3, 3, mis)


# ---- ComputeSim3 (:229-340) ----------------------------------------------------------------------------------------------------------------
def jacobi_eigen4(N):
    """cv::eigen of a symmetric 4x4, frozen: cyclic two-sided Jacobi in f64, pairs (p, q), p < q, ascending, at most SWEEPS sweeps; an
    element at or below DBL_EPSILON times the largest magnitude of the input is left alone.  -> (eigenvalues = the diagonal, V)"""
    A = [[float(N[i][j]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    big = 0.0
    for i in range(4):
        for j in range(4):
            if not abs(A[i][j]) <= big:
                big = abs(A[i][j])
    thr = EPS * big
    for _ in range(SWEEPS):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if not abs(apq) > thr:
                    continue
                rotated = True
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                th2 = theta * theta
                tn = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(1.0 + th2))
                c = 1.0 / math.sqrt(1.0 + tn * tn); s = c * tn
                A[p][p] = A[p][p] - tn * apq; A[q][q] = A[q][q] + tn * apq
                A[p][q] = 0.0; A[q][p] = 0.0
                for k in range(4):
                    if k != p and k != q:
                        x, y = A[k][p], A[k][q]
                        A[k][p] = c * x - s * y; A[p][k] = A[k][p]
                        A[k][q] = s * x + c * y; A[q][k] = A[k][q]
                    vx, vy = V[k][p], V[k][q]
                    V[k][p] = c * vx - s * vy; V[k][q] = s * vx + c * vy
        if not rotated:
            break
    return [A[i][i] for i in range(4)], V


def rodrigues(rv):
    """cv::Rodrigues, vector to matrix, in double, narrowed once"""
    r = [float(rv[0]), float(rv[1]), float(rv[2])]
    theta = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if theta < EPS:
        return np.eye(3, dtype=F)
    if theta != theta or math.isinf(theta):
        return np.full((3, 3), np.nan, F)
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c; it = 1.0 / theta
    r = [r[0] * it, r[1] * it, r[2] * it]
    K = [[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]]
    return np.array([[F((c * (1.0 if i == j else 0.0) + c1 * (r[i] * r[j])) + s * K[i][j]) for j in range(3)] for i in range(3)], F)


def compute_sim3(P1, P2, fix_scale, mis=()):
    """P1[k], P2[k] = the k-th sampled point in camera 1 / camera 2 (the columns of P3Dc1i / P3Dc2i) -> (R12 [3,3], t12 [3], s12), float"""
    P1 = np.asarray(P1, F); P2 = np.asarray(P2, F)
    with np.errstate(all="ignore"):
        third = F(1.0 / 3.0)
        O1 = np.array([F(F((float(P1[0][i]) + float(P1[1][i])) + float(P1[2][i])) * third) for i in range(3)], F)
        O2 = np.array([F(F((float(P2[0][i]) + float(P2[1][i])) + float(P2[2][i])) * third) for i in range(3)], F)
        r1 = (P1 - O1).astype(F); r2 = (P2 - O2).astype(F)                   # r[k][i] = Pr.col(k)[i]
        M = np.array([[F(dot3(r2[:, i], r1[:, j])) for j in range(3)] for i in range(3)], F)
        N11 = F(F(M[0, 0] + M[1, 1]) + M[2, 2]); N12 = F(M[1, 2] - M[2, 1]); N13 = F(M[2, 0] - M[0, 2]); N14 = F(M[0, 1] - M[1, 0])
        N22 = F(F(M[0, 0] - M[1, 1]) - M[2, 2]); N23 = F(M[0, 1] + M[1, 0]); N24 = F(M[2, 0] + M[0, 2])
        N33 = F(F(-M[0, 0] + M[1, 1]) - M[2, 2]); N34 = F(M[1, 2] + M[2, 1]); N44 = F(F(-M[0, 0] - M[1, 1]) + M[2, 2])
        Nm = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
        ev, V = jacobi_eigen4(Nm)
        best = 0
        for j in range(1, 4):
            if ev[j] > ev[best]:
                best = j
        e = [F(V[k][best]) for k in range(4)]
        nrm = math.sqrt(dot3(e[1:], e[1:]))
        ang = math.atan2(nrm, float(e[0]))
        alpha = D(2.0 * ang) / D(nrm)                                        # 0 / 0 -> NaN, as the reference's cv::Mat division
        rv = [F(D(float(e[k])) * alpha) for k in (1, 2, 3)]
        R = rodrigues(rv)
        P3 = np.array([[F(dot3(R[i], r2[k])) for i in range(3)] for k in range(3)], F)   # P3[k][i]
        if fix_scale and "scale_not_fixed" not in mis:
            s = F(1.0)
        else:
            nom = 0.0; den = 0.0
            for i in range(3):
                for k in range(3):
                    nom = nom + float(r1[k][i]) * float(P3[k][i])
                    den = den + float(F(P3[k][i] * P3[k][i]))
            s = F(D(nom) / D(den))
        t = np.array([F(float(O1[i]) - float(s) * dot3(R[i], O2)) for i in range(3)], F)
    return R, t, s


def transforms_of(R, t, s, mis=()):
    """Step 8 (:324-339) -> (A12, b12, A21, b21): the upper 3x4 of mT12i and mT21i"""
    with np.errstate(all="ignore"):
        A12 = (F(s) * R).astype(F)
        if "t21_not_inverted" in mis:
            return A12, t, A12, t
        si = F(D(1.0) / D(float(s)))
        A21 = (R.T * si).astype(F)
        b21 = np.array([F(-dot3(A21[i], t)) for i in range(3)], F)
    return A12, t, A21, b21


# ---- CheckInliers (:343-367) ---------------------------------------------------------------------------------------------------------------
def check_inliers(C, T, cam, mis=()):
    """-> (mask, err1, err2 float [N])"""
    A12, b12, A21, b21 = T
    N = len(C["X1"])
    err1 = np.zeros(N, F); err2 = np.zeros(N, F)
    with np.errstate(all="ignore"):
        for i in range(N):
            u, v = to_image(mul_add(A12, C["X2"][i], b12), cam, mis)         # vP2im1
            dx, dy = F(C["im1"][i][0] - u), F(C["im1"][i][1] - v)
            err1[i] = F(float(dx) * float(dx) + float(dy) * float(dy))
            u, v = to_image(mul_add(A21, C["X1"][i], b21), cam, mis)         # vP1im2
            dx, dy = F(u - C["im2"][i][0]), F(v - C["im2"][i][1])
            err2[i] = F(float(dx) * float(dx) + float(dy) * float(dy))
        mask = (err1 < C["e1"]) & (err2 < C["e2"])
    return mask, err1, err2


# ---- iterate (:143-210), run to the first success or to mRansacMaxIts ------------------------------------------------------------------------
def solve(kf1, kf2, match12, cam, sigma2, draws, max_iterations=300, probability=0.99, min_inliers=20, fix_scale=True, state=None, mis=()):
    """draws [max_iterations, 3]; state = (mnIterations, mnBestInliers) on entry or None.  -> dict(N, max_its, ninliers, iterations, sim3
    (16 floats or None), inlier [n1] uint8, state (on return), stage [n1], info = [dict(it, sample, R, t, s, ninliers, err1, err2, mask)])"""
    mis = frozenset(mis)
    C = construct(kf1, kf2, match12, cam, sigma2, mis)
    N = len(C["idx1"])
    its, _ = ransac_iterations(N, probability, min_inliers, max_iterations)
    it0, best = (0, 0) if state is None or "state_not_resumed" in mis else (max(int(state[0]), 0), int(state[1]))
    out = dict(N=N, max_its=its, ninliers=0, iterations=it0, sim3=None, inlier=np.zeros(kf1["n"], np.uint8), state=(it0, best), stage=C["stage"].copy(),
               info=[], C=C)
    if its == 0:
        return out
    done = it0
    best_info = None
    for it in range(it0, its):
        done = it + 1
        info = hypothesis(C, it, draws, cam, fix_scale, mis)
        ni = info["ninliers"]
        out["info"].append(info)
        if (ni > best) if "best_strict" in mis else (ni >= best):
            best = ni; best_info = info
            if (ni >= min_inliers) if "success_nonstrict" in mis else (ni > min_inliers):
                publish(out, C, info)
                break
    if out["sim3"] is None and "return_best" in mis and best_info is not None:
        publish(out, C, best_info)
    out["iterations"] = done
    out["state"] = (done, best)
    return out


def hypothesis(C, it, draws, cam, fix_scale=True, mis=()):
    """iteration `it` on its own, as solve() runs it: the device computes every iteration from the state's to mRansacMaxIts at once"""
    smp = sample_indices(len(C["idx1"]), draws[it], mis)
    R, t, s = compute_sim3(C["X1"][smp], C["X2"][smp], fix_scale, mis)
    mask, err1, err2 = check_inliers(C, transforms_of(R, t, s, mis), cam, mis)
    return dict(it=it, sample=smp, R=R, t=t, s=s, ninliers=int(mask.sum()), err1=err1, err2=err2, mask=mask)


def publish(out, C, info):
    out["ninliers"] = info["ninliers"]
    out["sim3"] = sim3_16(info["R"], info["t"], info["s"])
    out["inlier"][C["idx1"][info["mask"]]] = 1
    ok1 = info["err1"] < C["e1"]
    st = np.where(info["mask"], INLIER, np.where(ok1, FAIL_ERR2, FAIL_ERR1))
    out["stage"][C["idx1"]] = st


def sim3_16(R, t, s):
    o = np.zeros(16, F)
    o[:9] = np.asarray(R, F).reshape(9); o[9:12] = t; o[12] = s
    return o


# ---- an independent statement of the closed form: full f64, numpy.linalg.eigh ----------------------------------------------------------------
def horn_f64(P1, P2, fix_scale):
    """Horn 1987 on three point pairs, nothing narrowed: -> (R12, t12, s12) in double"""
    P1 = np.asarray(P1, D); P2 = np.asarray(P2, D)
    O1 = P1.mean(0); O2 = P2.mean(0)
    r1 = P1 - O1; r2 = P2 - O2
    M = r2.T @ r1
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, U = np.linalg.eigh(N)
    q = U[:, np.argmax(w)]
    q0, qv = q[0], q[1:]
    R = (q0 * q0 - qv @ qv) * np.eye(3) + 2 * np.outer(qv, qv) + 2 * q0 * np.array([[0, -qv[2], qv[1]], [qv[2], 0, -qv[0]], [-qv[1], qv[0], 0]])
    P3 = r2 @ R.T
    s = 1.0 if fix_scale else float((r1 * P3).sum() / (P3 * P3).sum())
    t = O1 - s * (R @ O2)
    return R, t, s
