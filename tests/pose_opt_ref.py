"""pose_opt_ref.py -- TEST-SIDE RESTATEMENT (test infrastructure only) of Optimizer::PoseOptimization (ORB/src/Optimizer.cc:251-503)
and of the pieces of g2o it runs, in IEEE double with numpy, written from the reference's sources and not from the kernel:

  * the edges: EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose (Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:143-202,
    .cpp:37-42, :266-364 -- incl. the FLOAT invz of the stereo cam_project, :299-306), chi2 (core/base_edge.h:58-61);
  * RobustKernelHuber (core/robust_kernel_impl.cpp:65-91) with delta = (double)(float)(deltaMono * qual_score) (Optimizer.cc:286-287,
    :342, :380), H and b weighted by rho[1] only (core/base_unary_edge.hpp:56-63, core/base_edge.h:96-102);
  * OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-189), the iteration loop of
    SparseOptimizer::optimize (core/sparse_optimizer.cpp:354-419), activeRobustChi2 (:100-114);
  * LinearSolverDense (solvers/linear_solver_dense.h:104-112): Eigen::LDLT -- diagonal pivoting, isPositive(), pivots below
    max|D| * eps treated as zero in the solve;
  * SE3Quat (types/se3quat.h): the constructors' normalizeRotation, map, operator*, exp; Eigen's Quaternion(Matrix3), toRotationMatrix,
    quaternion product and quaternion * vector; Converter::toSE3Quat / toCvMat (ORB/src/Converter.cc:37-71);
  * the round loop of Optimizer.cc:415-494: every round restarts from the input pose, level-0 edges only, chi2 of a level-0 edge from
    the state its error was last computed at, float comparison with 5.991f / 7.815f, kernels dropped after round min(2, n - 2),
    break when the graph has fewer than 10 edges.

Edge errors and Jacobians are evaluated per edge (vectorised: one rounding per operation, nothing fused); the ONLY sums over edges are
H (21 entries), b (6) and the robust chi2, taken in edge order or, with `perm`, in that permutation of it.  g2o's own order
(_activeEdges) is an implementation detail of its containers, so results that depend on it are noise of the method itself.
"""
import numpy as np

F = np.float32
D = np.float64

DELTA_MONO = F(np.sqrt(D(5.991)))               # const float deltaMono = sqrt(5.991)  (Optimizer.cc:286)
DELTA_STEREO = F(np.sqrt(D(7.815)))             # :287
CHI2_MONO = F(5.991)                            # :288
CHI2_STEREO = F(7.815)                          # :289


def inv_level_sigma2(scale_factors):
    """mvInvLevelSigma2 as the ORBextractor constructor fills it (ORB/src/ORBextractor.cc:419-431): float sf * sf, then 1.0f / that."""
    sf = np.asarray(scale_factors, F)
    return (F(1.0) / (sf * sf).astype(F)).astype(F)


# ---- Eigen / SE3Quat pieces, plain Python floats ------------------------------------------------------------------------------
def quat_from_rot(m):
    """Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other,3,3>) -> [x, y, z, w]"""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return [D(v) for v in q]


def quat_normalize_rotation(q):
    """SE3Quat::normalizeRotation (se3quat.h:280-285)"""
    if q[3] < 0:
        q = [-v for v in q]
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v / n for v in q]


def quat_mul(a, b):
    """Eigen quaternion product a * b, [x, y, z, w]"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_rotate(q, v):
    """Eigen QuaternionBase::_transformVector: uv = 2 * vec x v; v + w * uv + vec x uv.  v: three scalars or three arrays."""
    x, y, z, w = q
    ux = y * v[2] - z * v[1]; uy = z * v[0] - x * v[2]; uz = x * v[1] - y * v[0]
    ux = ux + ux; uy = uy + uy; uz = uz + uz
    return [v[0] + w * ux + (y * uz - z * uy), v[1] + w * uy + (z * ux - x * uz), v[2] + w * uz + (x * uy - y * ux)]


def quat_to_rot(q):
    """Eigen QuaternionBase::toRotationMatrix"""
    x, y, z, w = q
    tx = 2.0 * x; ty = 2.0 * y; tz = 2.0 * z
    twx = tx * w; twy = ty * w; twz = tz * w
    txx = tx * x; txy = ty * x; txz = tz * x
    tyy = ty * y; tyz = tz * y; tzz = tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def se3_from_pose(pose12):
    """Converter::toSE3Quat (Converter.cc:37-47): float entries widened, Quaterniond(R), normalizeRotation"""
    T = np.asarray(pose12, F).reshape(3, 4)
    R = [[D(T[i, j]) for j in range(3)] for i in range(3)]
    return quat_normalize_rotation(quat_from_rot(R)), [D(T[i, 3]) for i in range(3)]


def pose_from_se3(q, t):
    """Converter::toCvMat(SE3Quat) (Converter.cc:49-71): to_homogeneous_matrix, narrowed to float"""
    R = quat_to_rot(q)
    out = np.zeros((3, 4), F)
    for i in range(3):
        for j in range(3):
            out[i, j] = F(R[i][j])
        out[i, 3] = F(t[i])
    return out.reshape(12)


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257): update = [omega, upsilon]"""
    om = [D(u[0]), D(u[1]), D(u[2])]
    up = [D(u[3]), D(u[4]), D(u[5])]
    theta = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    Om2 = [[Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
    I = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if theta < 0.00001:
        R = [[I[i][j] + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        a = np.sin(theta) / theta
        b = (1.0 - np.cos(theta)) / (theta * theta)
        c = (theta - np.sin(theta)) / (theta * theta * theta)
        R = [[I[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]
        V = [[I[i][j] + b * Om[i][j] + c * Om2[i][j] for j in range(3)] for i in range(3)]
    t = [V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2] for i in range(3)]
    return quat_normalize_rotation(quat_from_rot(R)), t


def se3_mul(a, b):
    """SE3Quat::operator* (se3quat.h:104-110)"""
    qa, ta = a
    qb, tb = b
    r = quat_rotate(qa, tb)
    return quat_normalize_rotation(quat_mul(qa, qb)), [ta[0] + r[0], ta[1] + r[1], ta[2] + r[2]]


def ldlt_solve(A, b):
    """Eigen::LDLT<MatrixXd>::compute / isPositive / solve on a symmetric 6x6: returns (x, positive)"""
    n = len(b)
    M = [[D(A[i][j]) for j in range(n)] for i in range(n)]
    perm = list(range(n))
    neg = False
    for k in range(n):
        p = k
        for i in range(k + 1, n):
            if abs(M[i][i]) > abs(M[p][p]):
                p = i
        if p != k:
            for j in range(n):
                M[k][j], M[p][j] = M[p][j], M[k][j]
            for i in range(n):
                M[i][k], M[i][p] = M[i][p], M[i][k]
            perm[k], perm[p] = perm[p], perm[k]
        d = M[k][k]
        if d < 0:
            neg = True
        if d != 0:
            for i in range(k + 1, n):
                M[i][k] = M[i][k] / d
            for i in range(k + 1, n):
                for j in range(k + 1, i + 1):
                    M[i][j] = M[i][j] - M[i][k] * d * M[j][k]
                    M[j][i] = M[i][j]
    if neg:
        return None, False
    y = [D(b[perm[i]]) for i in range(n)]
    for i in range(n):
        for j in range(i):
            y[i] = y[i] - M[i][j] * y[j]
    dmax = max(abs(M[i][i]) for i in range(n))
    tol = max(dmax * np.finfo(D).eps, 1.0 / np.finfo(D).max)
    for i in range(n):
        y[i] = y[i] / M[i][i] if abs(M[i][i]) > tol else D(0.0)
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] = y[i] - M[j][i] * y[j]
    x = [D(0.0)] * n
    for i in range(n):
        x[perm[i]] = y[i]
    return x, True


# ---- the edges ----------------------------------------------------------------------------------------------------------------
class Edges:
    """the frame's edges in keypoint order, inputs widened to double exactly where the reference does (Optimizer.cc:328-390)"""

    def __init__(self, kps, n, uright, inv_sigma2, fx, fy, cx, cy, bf, xw, has_point, quality):
        has = np.asarray(has_point[:n]) != 0
        self.idx = np.nonzero(has)[0]
        i = self.idx
        self.stereo = ~(np.asarray(uright[:n], F)[i] < 0)                          # mvuRight[i] < 0: monocular (Optimizer.cc:323)
        self.obs = np.stack([np.asarray(kps["x"][:n], F)[i].astype(D), np.asarray(kps["y"][:n], F)[i].astype(D), np.asarray(uright[:n], F)[i].astype(D)], 0)
        self.s = np.asarray(inv_sigma2, F)[np.asarray(kps["octave"][:n])[i]].astype(D)
        q = np.ones(len(i), F) if quality is None else np.asarray(quality[:n], F)[i]
        delta_f = np.where(self.stereo, DELTA_STEREO, DELTA_MONO).astype(F) * q                # float product (:342, :380)
        self.delta = delta_f.astype(F).astype(D)
        self.dsqr = self.delta * self.delta                                        # RobustKernelHuber::setDelta
        self.X = np.asarray(xw, F).reshape(-1, 3)[i].astype(D).T                    # e->Xw[k] = Xw.at<float>(k)
        self.fx, self.fy, self.cx, self.cy, self.bf = D(F(fx)), D(F(fy)), D(F(cx)), D(F(cy)), D(F(bf))
        self.thr = np.where(self.stereo, CHI2_STEREO, CHI2_MONO).astype(F)

    def errors(self, se3):
        """computeError + chi2 of every edge at `se3` -> (P, e [3, n] with e[2] = 0 for mono edges, chi2)"""
        q, t = se3
        r = quat_rotate(q, [self.X[0], self.X[1], self.X[2]])
        P = [r[0] + t[0], r[1] + t[1], r[2] + t[2]]
        with np.errstate(all="ignore"):
            # mono: project2d, then * fx + cx (.cpp:37-42, :290-296)
            m0 = self.obs[0] - ((P[0] / P[2]) * self.fx + self.cx)
            m1 = self.obs[1] - ((P[1] / P[2]) * self.fy + self.cy)
            # stereo: const float invz = 1.0f / trans_xyz[2] (.cpp:299-306)
            invz = (1.0 / P[2]).astype(F).astype(D)
            r0 = P[0] * invz * self.fx + self.cx
            r1 = P[1] * invz * self.fy + self.cy
            r2 = r0 - self.bf * invz
            e0 = np.where(self.stereo, self.obs[0] - r0, m0)
            e1 = np.where(self.stereo, self.obs[1] - r1, m1)
            e2 = np.where(self.stereo, self.obs[2] - r2, 0.0)
            chi2 = e0 * (self.s * e0) + e1 * (self.s * e1)
            chi2 = np.where(self.stereo, chi2 + e2 * (self.s * e2), chi2)
        return P, (e0, e1, e2), chi2

    def robustify(self, chi2, robust):
        """RobustKernelHuber::robustify -> rho[0], rho[1]; no kernel: chi2, 1"""
        if not robust:
            return chi2, np.ones_like(chi2)
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            inl = chi2 <= self.dsqr
            rho0 = np.where(inl, chi2, 2 * sq * self.delta - self.dsqr)
            rho1 = np.where(inl, 1.0, self.delta / sq)
        return rho0, rho1

    def jacobians(self, P):
        """linearizeOplus (.cpp:266-288, :335-364): rows [3][6], row 2 = 0 for mono edges"""
        x, y = P[0], P[1]
        with np.errstate(all="ignore"):
            invz = 1.0 / P[2]
            invz2 = invz * invz
            J0 = [x * y * invz2 * self.fx, -(1 + (x * x * invz2)) * self.fx, y * invz * self.fx, -invz * self.fx, np.zeros_like(x), x * invz2 * self.fx]
            J1 = [(1 + y * y * invz2) * self.fy, -x * y * invz2 * self.fy, -x * invz * self.fy, np.zeros_like(x), -invz * self.fy, y * invz2 * self.fy]
            J2 = [J0[0] - self.bf * y * invz2, J0[1] + self.bf * x * invz2, J0[2], J0[3], np.zeros_like(x), J0[5] - self.bf * invz2]
            J2 = [np.where(self.stereo, v, 0.0) for v in J2]
        return [J0, J1, J2]


def _sum_rows(M, order):
    """the sums over the active edges, in `order`: row after row, one rounding per addition and column"""
    acc = np.zeros(M.shape[1], D)
    with np.errstate(all="ignore"):
        for row in M[order]:
            acc = acc + row
    return acc


def build_system(E, se3, active, robust, order):
    """computeActiveErrors + buildSystem over the level-0 edges: (H 6x6, b 6, robust chi2)"""
    P, e, chi2 = E.errors(se3)
    rho0, rho1 = E.robustify(chi2, robust)
    J = E.jacobians(P)
    w = rho1 * E.s
    order = [k for k in order if active[k]]
    cols = []
    with np.errstate(all="ignore"):
        for j in range(6):
            for k in range(j, 6):
                cols.append(w * (J[0][j] * J[0][k] + J[1][j] * J[1][k] + J[2][j] * J[2][k]))
        for j in range(6):
            cols.append(w * (J[0][j] * e[0] + J[1][j] * e[1] + J[2][j] * e[2]))
        cols.append(rho0)
    acc = _sum_rows(np.stack(cols, 1), order)
    H = [[D(0.0)] * 6 for _ in range(6)]
    c = 0
    for j in range(6):
        for k in range(j, 6):
            H[j][k] = H[k][j] = acc[c]
            c += 1
    b = [-acc[21 + j] for j in range(6)]
    return H, b, acc[27]


def robust_chi2(E, se3, active, robust, order):
    _, _, chi2 = E.errors(se3)
    rho0, _ = E.robustify(chi2, robust)
    return _sum_rows(rho0.reshape(-1, 1), [k for k in order if active[k]])[0]


def pose_optimization(kps, n, uright, inv_sigma2, fx, fy, cx, cy, bf, xw, has_point, quality, n_rounds, pose, perm=None):
    """Optimizer::PoseOptimization for one frame.  kps: structured array with x, y, octave (mvKeysUn), n = keypoints of the frame,
    xw [*, 3] / has_point / quality indexed by keypoint, pose = float32 [12] (mTcw, row-major 3x4).  perm: a permutation of the EDGE
    list (edges in keypoint order) = the order H, b and chi2 are summed in.
    Returns dict(pose float32 [12], outlier uint8 [len(has_point)], ninliers, chi2 float32 [..] or None (mvChi2 of round n_rounds - 1),
    pose64 = (q, t) of the final estimate, chi2_rounds = per executed round the double chi2 of every edge as classified, edges = idx,
    b = the gradient at the final estimate over the last round's level-0 edges, iterations = LM iterations per round)."""
    nk = len(has_point)
    pose = np.asarray(pose, F).reshape(12).copy()
    E = Edges(kps, n, uright, inv_sigma2, fx, fy, cx, cy, bf, xw, has_point, quality)
    ne = len(E.idx)
    out = dict(pose=pose, outlier=np.zeros(nk, np.uint8), ninliers=0, chi2=None, pose64=se3_from_pose(pose), chi2_rounds=[], edges=E.idx,
               b=None, iterations=[], thr=E.thr, stereo=E.stereo)
    if ne < 3:                                                                      # Optimizer.cc:403-404
        return out
    order = list(range(ne)) if perm is None else [int(k) for k in perm]
    assert sorted(order) == list(range(ne))
    outlier = np.zeros(ne, bool)
    robust = True
    nbad = 0
    est = se3_from_pose(pose)
    for it in range(int(n_rounds)):
        est = se3_from_pose(pose)                                                   # :418
        active = ~outlier                                                           # initializeOptimization(0): level-0 edges
        last_eval = est
        lam = D(0.0); ni = D(2.0); n_bad_steps = 0
        x = [D(0.0)] * 6
        iters = 0
        for i in range(10):                                                         # optimize(its[it]), sparse_optimizer.cpp:376-414
            iters += 1
            H, b, cur = build_system(E, est, active, robust, order)                # computeActiveErrors, activeRobustChi2, buildSystem
            last_eval = est
            ini = cur
            if i == 0:
                lam = 1e-5 * max(abs(H[j][j]) for j in range(6))                    # computeLambdaInit: _tau * maxDiagonal
                ni = D(2.0); n_bad_steps = 0
            rho = D(0.0)
            qmax = 0
            while True:
                A = [[H[r][c] + (lam if r == c else 0.0) for c in range(6)] for r in range(6)]   # setLambda
                xs, ok2 = ldlt_solve(A, b)
                if ok2:
                    x = xs
                trial = se3_mul(se3_exp(x), est)                                    # oplusImpl (types_six_dof_expmap.h:73-76)
                tmp = robust_chi2(E, trial, active, robust, order)
                last_eval = trial
                if not ok2:
                    tmp = np.finfo(D).max
                with np.errstate(all="ignore"):
                    scale = D(0.0)
                    for j in range(6):
                        scale = scale + x[j] * (lam * x[j] + b[j])                  # computeScale
                    scale = scale + 1e-3
                    rho = (cur - tmp) / scale
                if rho > 0 and np.isfinite(tmp):
                    y = 2 * rho - 1
                    alpha = 1.0 - y * y * y
                    alpha = min(alpha, 2.0 / 3.0)
                    lam = lam * max(1.0 / 3.0, alpha)
                    ni = D(2.0)
                    cur = tmp
                    est = trial
                else:
                    lam = lam * ni
                    ni = ni * 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                break                                                               # Terminate
            if (ini - cur) * 1e3 < ini:
                n_bad_steps += 1
            else:
                n_bad_steps = 0
            if n_bad_steps >= 3:
                break
        out["iterations"].append(iters)
        # ---- classification (Optimizer.cc:422-490)
        _, _, chi_last = E.errors(last_eval)                                        # level-0 edges: the error they last computed
        _, _, chi_est = E.errors(est)                                               # outliers: e->computeError() at the estimate
        chi = np.where(outlier, chi_est, chi_last)
        with np.errstate(all="ignore"):
            chif = chi.astype(F)                                                    # const float chi2 = e->chi2()
        outlier = chif > E.thr
        nbad = int(outlier.sum())
        out["chi2_rounds"].append(chi.copy())
        if it == min(2, int(n_rounds) - 2):
            robust = False                                                          # e->setRobustKernel(0)
        if it == int(n_rounds) - 1:
            c = np.zeros(nk, F); c[E.idx] = chif
            out["chi2"] = c
        last_active = active
        if ne < 10:                                                                 # optimizer.edges().size() < 10
            break
    _, out["b"], _ = build_system(E, est, last_active, robust, order)
    out["pose64"] = est
    out["pose"] = pose_from_se3(*est)
    out["outlier"][E.idx] = outlier.astype(np.uint8)
    out["ninliers"] = ne - nbad
    return out


def pose_difference(a, b):
    """(rotation angle [rad], translation difference relative to max(|t|, 1)) between two float/double [12] poses"""
    A = np.asarray(a, D).reshape(3, 4); B = np.asarray(b, D).reshape(3, 4)
    dR = A[:, :3] @ B[:, :3].T
    # the angle from the antisymmetric part: well conditioned near zero, where acos of the trace is not
    s = 0.5 * np.sqrt((dR[2, 1] - dR[1, 2]) ** 2 + (dR[0, 2] - dR[2, 0]) ** 2 + (dR[1, 0] - dR[0, 1]) ** 2)
    c = 0.5 * (np.trace(dR) - 1.0)
    ang = float(np.arctan2(s, c))
    dt = float(np.linalg.norm(A[:, 3] - B[:, 3]) / max(np.linalg.norm(B[:, 3]), 1.0))
    return ang, dt
