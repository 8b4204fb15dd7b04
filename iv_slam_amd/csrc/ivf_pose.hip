// ivf_pose.hip -- batched, device-resident Optimizer::PoseOptimization (ORB/src/Optimizer.cc:251-503): the consumer of the two batched
// searches of ivf_track.hip and ivf_track_local.hip, on the same handle (ivf_tracker.h; the points they hand over: ivf_track_points.hip).  g2o's machinery for this call is one 6-dof vertex (VertexSE3Expmap), unary edges
// (EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose, Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp}), a dense 6x6
// system (solvers/linear_solver_dense.h: Eigen::LDLT) and OptimizationAlgorithmLevenberg (core/optimization_algorithm_levenberg.cpp);
// all of it is restated here in double, the arithmetic the reference runs it in.
//
//   k_pose_opt          one workgroup (4 waves) per frame, ONE launch for the whole call: all rounds, LM iterations and trials.
//                       The frame's edges are compacted into LDS once, in keypoint order (32 B per edge: float Xw, float observation,
//                       the float product delta * qual_score, keypoint index | octave | stereo | outlier), and widened to double where
//                       the reference widens them.  An evaluation = every lane walks its edges (error, chi2, Huber rho, and for a
//                       linearisation the 2x6 / 3x6 Jacobian), 21 + 6 + 1 sums are reduced in the wave by xor-butterflies and across
//                       the four waves through LDS in wave order: the summation tree is fixed, two runs are bit-identical.  Lane 0
//                       does the LDLT solve, exp(dx) * estimate, the rho / lambda / nu bookkeeping and the stop tests and publishes
//                       the next pose and the decision through LDS; every branch around a barrier reads that decision.
//                       Loop bounds are compile-time (4 rounds x 10 iterations x 10 trials): NaN input cannot spin the kernel.
// The sums, the ordered compaction, the frame's pointer set and the pose store are ivf_solve.h's, shared with ivf_pnp.hip.
#include "ivf_solve.h"

using namespace ivf;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxRounds = 4, kMaxIters = 10, kMaxTrials = 10;        // Optimizer.cc:411-413, maxTrialsAfterFailure (levenberg.cpp:51)
constexpr int kSums = 28;                                             // H upper triangle (21), b (6), robust chi2
constexpr unsigned kStereoBit = 1u << 16, kOutlierBit = 1u << 17;

struct PoseParams {
    int nf, nRecords;
    size_t recBytes;
    float fx, fy, cx, cy, bf;
    float invSigma2[kMaxLevels];                                      // mvInvLevelSigma2 (ORBextractor.cc:419-431)
};

struct __attribute__((aligned(16))) Edge { float X[3]; float obs[3]; float delta; unsigned bits; };   // bits: keypoint | octave << 12 | flags
static_assert(sizeof(Edge) == 32, "an edge is two 16-byte LDS reads");

struct Se3 { double q[4], t[3]; };                                    // SE3Quat: quaternion [x, y, z, w], translation

// ---- Eigen / SE3Quat pieces (types/se3quat.h) ---------------------------------------------------------------------------------
DEVINL void quat_from_rot(const double m[3][3], double q[4])          // Eigen::Quaterniond(Matrix3d)
{
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        // the three cases of i = argmax of the diagonal, j = i + 1, k = j + 1 (mod 3), spelled out: no dynamic indexing
        if (!(m[1][1] > m[0][0]) && !(m[2][2] > m[0][0])) {
            t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0); q[0] = 0.5 * t; t = 0.5 / t;
            q[3] = (m[2][1] - m[1][2]) * t; q[1] = (m[1][0] + m[0][1]) * t; q[2] = (m[2][0] + m[0][2]) * t;
        } else if (m[1][1] > m[0][0] && !(m[2][2] > m[1][1])) {
            t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0); q[1] = 0.5 * t; t = 0.5 / t;
            q[3] = (m[0][2] - m[2][0]) * t; q[2] = (m[2][1] + m[1][2]) * t; q[0] = (m[0][1] + m[1][0]) * t;
        } else {
            t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0); q[2] = 0.5 * t; t = 0.5 / t;
            q[3] = (m[1][0] - m[0][1]) * t; q[0] = (m[0][2] + m[2][0]) * t; q[1] = (m[1][2] + m[2][1]) * t;
        }
    }
}
DEVINL void normalize_rotation(double q[4])                           // SE3Quat::normalizeRotation (:280-285)
{
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}
DEVINL void quat_rotate(const double q[4], const double v[3], double out[3])   // Eigen QuaternionBase::_transformVector
{
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    out[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
    out[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
    out[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
DEVINL void quat_to_rot(const double q[4], double R[3][3])            // Eigen QuaternionBase::toRotationMatrix
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0][0] = 1.0 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1.0 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1.0 - (txx + tyy);
}
// SE3Quat::exp(update) * estimate (types_six_dof_expmap.h:73-76, se3quat.h:104-110, :223-257); update = [omega, upsilon]
DEVINL Se3 oplus(const double u[6], const Se3& est)
{
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double Om[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    double Om2[3][3], R[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Om2[i][j] = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) { R[i][j] = (i == j ? 1.0 : 0.0) + Om[i][j] + Om2[i][j]; V[i][j] = R[i][j]; }
    } else {
        const double a = sin(theta) / theta, b = (1.0 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / (theta * theta * theta);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                R[i][j] = (i == j ? 1.0 : 0.0) + a * Om[i][j] + b * Om2[i][j];
                V[i][j] = (i == j ? 1.0 : 0.0) + b * Om[i][j] + c * Om2[i][j];
            }
    }
    double qe[4], te[3], r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) te[i] = V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2];
    quat_from_rot(R, qe);
    normalize_rotation(qe);
    Se3 out;
    quat_rotate(qe, est.t, r);
    out.t[0] = te[0] + r[0]; out.t[1] = te[1] + r[1]; out.t[2] = te[2] + r[2];
    const double* a = qe; const double* b = est.q;
    out.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    out.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    out.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    out.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    normalize_rotation(out.q);
    return out;
}

// Eigen::LDLT on the symmetric 6x6 M (diagonal pivoting), isPositive(), solve with pivots below max|D| * eps taken as zero
// (solvers/linear_solver_dense.h:104-112).  bx holds the right-hand side and receives the solution.  Everything lives in LDS (one lane
// works on it): the pivoting indexes dynamically, which registers cannot.
DEVINL bool ldlt_solve(double (*M)[6], double* y, int* perm, double* bx)
{
    for (int i = 0; i < 6; i++) perm[i] = i;
    bool neg = false;
    for (int k = 0; k < 6; k++) {
        int p = k;
        for (int i = k + 1; i < 6; i++) if (fabs(M[i][i]) > fabs(M[p][p])) p = i;
        if (p != k) {
            for (int j = 0; j < 6; j++) { const double v = M[k][j]; M[k][j] = M[p][j]; M[p][j] = v; }
            for (int i = 0; i < 6; i++) { const double v = M[i][k]; M[i][k] = M[i][p]; M[i][p] = v; }
            const int v = perm[k]; perm[k] = perm[p]; perm[p] = v;
        }
        const double d = M[k][k];
        if (d < 0) neg = true;
        if (d != 0) {
            for (int i = k + 1; i < 6; i++) M[i][k] = M[i][k] / d;
            for (int i = k + 1; i < 6; i++)
                for (int j = k + 1; j <= i; j++) { M[i][j] = M[i][j] - M[i][k] * d * M[j][k]; M[j][i] = M[i][j]; }
        }
    }
    if (neg) return false;
    for (int i = 0; i < 6; i++) y[i] = bx[perm[i]];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < i; j++) y[i] = y[i] - M[i][j] * y[j];
    double dmax = 0.0;
    for (int i = 0; i < 6; i++) dmax = fmax(dmax, fabs(M[i][i]));
    const double tol = fmax(dmax * 0x1p-52, 1.0 / 0x1.fffffffffffffp+1023);
    for (int i = 0; i < 6; i++) y[i] = fabs(M[i][i]) > tol ? y[i] / M[i][i] : 0.0;
    for (int i = 5; i >= 0; i--)
        for (int j = i + 1; j < 6; j++) y[i] = y[i] - M[j][i] * y[j];
    for (int i = 0; i < 6; i++) bx[perm[i]] = y[i];
    return true;
}

// ---- one edge -----------------------------------------------------------------------------------------------------------------
struct Cam { double fx, fy, cx, cy, bf; };
// computeError + chi2 (types_six_dof_expmap.h:153-157, :184-188; .cpp:37-42, :290-306; base_edge.h:58-61); P = estimate.map(Xw)
DEVINL double edge_error(const Edge& ed, const Cam& C, const double* q, const double* t, double s, double P[3], double e[3])
{
    const double X[3] = {(double)ed.X[0], (double)ed.X[1], (double)ed.X[2]};
    quat_rotate(q, X, P);
    P[0] = P[0] + t[0]; P[1] = P[1] + t[1]; P[2] = P[2] + t[2];
    if (ed.bits & kStereoBit) {
        const double invz = (double)(float)(1.0 / P[2]);               // const float invz = 1.0f / trans_xyz[2]
        const double r0 = P[0] * invz * C.fx + C.cx, r1 = P[1] * invz * C.fy + C.cy, r2 = r0 - C.bf * invz;
        e[0] = (double)ed.obs[0] - r0; e[1] = (double)ed.obs[1] - r1; e[2] = (double)ed.obs[2] - r2;
        return e[0] * (s * e[0]) + e[1] * (s * e[1]) + e[2] * (s * e[2]);
    }
    e[0] = (double)ed.obs[0] - ((P[0] / P[2]) * C.fx + C.cx);
    e[1] = (double)ed.obs[1] - ((P[1] / P[2]) * C.fy + C.cy);
    e[2] = 0.0;
    return e[0] * (s * e[0]) + e[1] * (s * e[1]);
}

// One evaluation over the level-0 edges at pose (q, t): the robust chi2, and with BUILD the quadratic form (base_unary_edge.hpp:43-72).
// Leaves the per-wave sums in part[wave][]; the caller's barrier makes them visible and lane 0 adds them in wave order (part_sum).
template <bool BUILD>
DEVINL void evaluate(const Edge* s_e, int nE, const Cam& C, const double* s_is2, const double* q, const double* t, bool robust,
                     double (*part)[kSums], int tid)
{
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; k++) acc[k] = 0.0;
    for (int e0 = tid; e0 < nE; e0 += kThreads) {
        const Edge ed = s_e[e0];
        if (ed.bits & kOutlierBit) continue;
        const double s = s_is2[(ed.bits >> 12) & 15u];
        double P[3], e[3];
        const double chi2 = edge_error(ed, C, q, t, s, P, e);
        double rho0 = chi2, rho1 = 1.0;
        if (robust) {                                                  // RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)
            const double delta = (double)ed.delta, dsqr = delta * delta;
            if (!(chi2 <= dsqr)) { const double sq = sqrt(chi2); rho0 = 2 * sq * delta - dsqr; rho1 = delta / sq; }
        }
        acc[27] = acc[27] + rho0;
        if (BUILD) {
            // linearizeOplus (.cpp:266-288, :335-364)
            const double x = P[0], y = P[1], invz = 1.0 / P[2], invz2 = invz * invz;
            double J[3][6];
            J[0][0] = x * y * invz2 * C.fx; J[0][1] = -(1 + (x * x * invz2)) * C.fx; J[0][2] = y * invz * C.fx;
            J[0][3] = -invz * C.fx; J[0][4] = 0.0; J[0][5] = x * invz2 * C.fx;
            J[1][0] = (1 + y * y * invz2) * C.fy; J[1][1] = -x * y * invz2 * C.fy; J[1][2] = -x * invz * C.fy;
            J[1][3] = 0.0; J[1][4] = -invz * C.fy; J[1][5] = y * invz2 * C.fy;
            const bool st = (ed.bits & kStereoBit) != 0;
            J[2][0] = st ? J[0][0] - C.bf * y * invz2 : 0.0; J[2][1] = st ? J[0][1] + C.bf * x * invz2 : 0.0; J[2][2] = st ? J[0][2] : 0.0;
            J[2][3] = st ? J[0][3] : 0.0; J[2][4] = 0.0; J[2][5] = st ? J[0][5] - C.bf * invz2 : 0.0;
            const double w = rho1 * s;                                 // robustInformation: rho[1] * information (base_edge.h:96-102)
            int c = 0;
#pragma unroll
            for (int j = 0; j < 6; j++)
#pragma unroll
                for (int k = j; k < 6; k++, c++) acc[c] = acc[c] + w * (J[0][j] * J[0][k] + J[1][j] * J[1][k] + J[2][j] * J[2][k]);
#pragma unroll
            for (int j = 0; j < 6; j++) acc[21 + j] = acc[21 + j] + w * (J[0][j] * e[0] + J[1][j] * e[1] + J[2][j] * e[2]);
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = BUILD ? 0 : 27; k < kSums; k++) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = v;
    }
}

DEVINL double part_sum(const double (*part)[kSums], int k) { return wave_order_sum<kWaves>(&part[0][k], kSums); }

__global__ __launch_bounds__(kThreads) void k_pose_opt(PoseParams Pm, const uint8_t* __restrict__ records, const int* __restrict__ frames,
                                                       const float* __restrict__ xw, const uint8_t* __restrict__ hasPoint,
                                                       const float* __restrict__ quality, int nRounds, float* __restrict__ poses,
                                                       uint8_t* __restrict__ outlierOut, int* __restrict__ nInliers, float* __restrict__ chi2Out)
{
    extern __shared__ Edge s_e[];
    __shared__ double s_part[kWaves][kSums];
    __shared__ double s_is2[kMaxLevels];
    __shared__ double s_pose[7], s_est[7];                             // the pose of the next evaluation; the estimate (classification)
    __shared__ double s_M[6][6], s_y[6], s_bx[6];
    __shared__ int s_perm[6], s_wcnt[kWaves], s_cont, s_term, s_nbad;
    const int f = blockIdx.x, tid = threadIdx.x, nf = Pm.nf;
    uint8_t* outl = outlierOut + (size_t)f * nf;
    float* chiO = chi2Out ? chi2Out + (size_t)f * nf : nullptr;
    for (int i = tid; i < nf; i += kThreads) { outl[i] = 0; if (chiO) chiO[i] = 0.0f; }
    const FrameObs O = frame_obs(records, Pm.recBytes, nf, Pm.nRecords, frames[f], xw, hasPoint, f);
    if (O.nC < 0) { if (tid == 0) nInliers[f] = -1; return; }
    const float* ql = quality ? quality + (size_t)f * nf : nullptr;
    if (tid < kMaxLevels) s_is2[tid] = (double)Pm.invSigma2[tid];
    if (tid == 0) s_nbad = 0;

    // ---- the edges, in keypoint order (Optimizer.cc:310-399)
    const float deltaMono = (float)sqrt(5.991), deltaStereo = (float)sqrt(7.815);   // :286-287
    const int nE = compact_ordered<kThreads>(O.nC, s_wcnt, tid, [&](int i) { return O.has[i] != 0; }, [&](int i, int slot) {
        const ivf_keypoint kp = O.kps[i];
        const float u = O.uRight[i];
        const bool st = !(u < 0);                                      // mvuRight[i] < 0: monocular (:323)
        const float q = ql ? ql[i] : 1.0f;
        Edge ed;
        ed.X[0] = O.X[3 * i]; ed.X[1] = O.X[3 * i + 1]; ed.X[2] = O.X[3 * i + 2];
        ed.obs[0] = kp.x; ed.obs[1] = kp.y; ed.obs[2] = u;
        ed.delta = (st ? deltaStereo : deltaMono) * q;                 // the float product of :342 / :380
        ed.bits = (unsigned)i | ((unsigned)clamp_octave(kp.octave) << 12) | (st ? kStereoBit : 0u);
        s_e[slot] = ed;
    });
    if (nE < 3) { if (tid == 0) nInliers[f] = 0; return; }            // :403-404 (nE is the same in every thread)

    const Cam C = {(double)Pm.fx, (double)Pm.fy, (double)Pm.cx, (double)Pm.cy, (double)Pm.bf};
    float* T = poses + (size_t)f * 12;
    // lane 0's state
    Se3 in = {}, est, lastEval;
    double H[21], b[6], x[6] = {0, 0, 0, 0, 0, 0}, lam = 0.0, ni = 2.0, cur = 0.0, ini = 0.0, rho = 0.0;
    int nBadSteps = 0, qmax = 0;
    if (tid == 0) {
        // Converter::toSE3Quat (Converter.cc:37-47)
        double R[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) R[i][j] = (double)T[4 * i + j];
            in.t[i] = (double)T[4 * i + 3];
        }
        quat_from_rot(R, in.q);
        normalize_rotation(in.q);
    }
    est = in; lastEval = in;
    auto publish = [&](double* dst, const Se3& p) {
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = p.q[k];
#pragma unroll
        for (int k = 0; k < 3; k++) dst[4 + k] = p.t[k];
    };
    bool robust = true;
#pragma unroll 1
    for (int round = 0; round < kMaxRounds; round++) {
        if (round >= nRounds) break;
        if (tid == 0) {
            est = in;                                                  // vSE3->setEstimate(toSE3Quat(pFrame->mTcw)) (:418)
            publish(s_pose, est);
            s_nbad = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) x[k] = 0.0;
        }
#pragma unroll 1
        for (int it = 0; it < kMaxIters; it++) {
            __syncthreads();
            evaluate<true>(s_e, nE, C, s_is2, s_pose, s_pose + 4, robust, s_part, tid);   // computeActiveErrors + buildSystem (levenberg.cpp:75-87)
            __syncthreads();
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < 21; k++) H[k] = part_sum(s_part, k);
#pragma unroll
                for (int k = 0; k < 6; k++) b[k] = -part_sum(s_part, 21 + k);
                cur = part_sum(s_part, 27);
                lastEval = est;
                ini = cur;
                if (it == 0) {                                         // computeLambdaInit: _tau * max diagonal (:166-180)
                    double md = 0.0;
                    md = fmax(fabs(H[0]), md); md = fmax(fabs(H[6]), md); md = fmax(fabs(H[11]), md);
                    md = fmax(fabs(H[15]), md); md = fmax(fabs(H[18]), md); md = fmax(fabs(H[20]), md);
                    lam = 1e-5 * md; ni = 2.0; nBadSteps = 0;
                }
                rho = 0.0; qmax = 0;
            }
#pragma unroll 1
            for (int trial = 0; trial < kMaxTrials; trial++) {
                bool ok2 = true;
                Se3 tr;
                if (tid == 0) {
                    int c = 0;
                    for (int j = 0; j < 6; j++)
                        for (int k = j; k < 6; k++, c++) { const double v = H[c] + (j == k ? lam : 0.0); s_M[j][k] = v; s_M[k][j] = v; }   // setLambda
#pragma unroll
                    for (int k = 0; k < 6; k++) s_bx[k] = b[k];
                    ok2 = ldlt_solve(s_M, s_y, s_perm, s_bx);
                    if (ok2) {                                         // a failed solve leaves the solver's x as it was
#pragma unroll
                        for (int k = 0; k < 6; k++) x[k] = s_bx[k];
                    }
                    tr = oplus(x, est);
                    publish(s_pose, tr);
                }
                __syncthreads();
                evaluate<false>(s_e, nE, C, s_is2, s_pose, s_pose + 4, robust, s_part, tid);
                __syncthreads();
                if (tid == 0) {
                    double tmp = part_sum(s_part, 27);
                    lastEval = tr;
                    if (!ok2) tmp = 0x1.fffffffffffffp+1023;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale = scale + x[j] * (lam * x[j] + b[j]);   // computeScale (:182-189)
                    scale = scale + 1e-3;
                    rho = (cur - tmp) / scale;
                    if (rho > 0 && isfinite(tmp)) {
                        const double y = 2 * rho - 1;
                        double alpha = 1.0 - y * y * y;
                        alpha = fmin(alpha, 2.0 / 3.0);
                        lam = lam * fmax(1.0 / 3.0, alpha);
                        ni = 2.0; cur = tmp; est = tr;
                    } else {
                        lam = lam * ni; ni = ni * 2;
                    }
                    qmax++;
                    s_cont = (rho < 0 && qmax < kMaxTrials) ? 1 : 0;
                }
                __syncthreads();
                if (!s_cont) break;
            }
            if (tid == 0) {
                int term = 0;
                if (qmax == kMaxTrials || rho == 0) term = 1;          // Terminate (:151-152)
                else {
                    if ((ini - cur) * 1e3 < ini) nBadSteps++; else nBadSteps = 0;   // :154-161
                    if (nBadSteps >= 3) term = 1;
                }
                s_term = term;
                publish(s_pose, est);
            }
            __syncthreads();
            if (s_term) break;
        }
        // ---- classification (Optimizer.cc:422-490): a level-0 edge keeps the error it last computed, an outlier recomputes it
        if (tid == 0) { publish(s_pose, lastEval); publish(s_est, est); }
        __syncthreads();
        int bad = 0;
        const bool logRound = round == nRounds - 1;
        for (int e0 = tid; e0 < nE; e0 += kThreads) {
            Edge ed = s_e[e0];
            const bool wasOut = (ed.bits & kOutlierBit) != 0;
            const double* ps = wasOut ? s_est : s_pose;
            double P[3], e[3];
            const float chi2 = (float)edge_error(ed, C, ps, ps + 4, s_is2[(ed.bits >> 12) & 15u], P, e);
            const bool out = chi2 > ((ed.bits & kStereoBit) ? 7.815f : 5.991f);
            s_e[e0].bits = out ? (ed.bits | kOutlierBit) : (ed.bits & ~kOutlierBit);
            bad += out ? 1 : 0;
            if (logRound && chiO) chiO[ed.bits & 0xfffu] = chi2;
        }
        if (bad) atomicAdd(&s_nbad, bad);
        if (round == min(2, nRounds - 2)) robust = false;              // e->setRobustKernel(0) (:448-450, :483-484)
        __syncthreads();
        if (nE < 10) break;                                            // optimizer.edges().size() < 10 (:492)
    }
    __syncthreads();
    for (int e0 = tid; e0 < nE; e0 += kThreads) { const unsigned bits = s_e[e0].bits; outl[bits & 0xfffu] = (bits & kOutlierBit) ? 1 : 0; }
    if (tid == 0) {
        // Converter::toCvMat(SE3Quat) (Converter.cc:49-71)
        double R[3][3];
        quat_to_rot(est.q, R);
        store_pose(T, &R[0][0], est.t);
        nInliers[f] = nE - s_nbad;
    }
}

PoseParams pose_params(const TrackParams& T, int n_records)
{
    PoseParams P;
    P.nf = T.nf; P.nRecords = n_records; P.recBytes = T.recBytes;
    P.fx = T.fx; P.fy = T.fy; P.cx = T.cx; P.cy = T.cy; P.bf = T.bf;
    level_sigma2(T, P.invSigma2);
    for (int l = 0; l < kMaxLevels; l++) P.invSigma2[l] = 1.0f / P.invSigma2[l];   // mvInvLevelSigma2 = 1.0f / mvLevelSigma2
    return P;
}

}  // namespace

extern "C" {

int ivf_tracker_optimize_pose(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames, int n_frames,
                              const float* d_xw, const uint8_t* d_has_point, const float* d_quality, int n_rounds, float* d_poses,
                              uint8_t* d_outlier, int32_t* d_ninliers, float* d_chi2, void* hip_stream)
{
    if (!t || !d_records || !d_frames || !d_xw || !d_has_point || !d_poses || !d_outlier || !d_ninliers) return fail(IVF_E_INVALID, "null argument");
    if (((size_t)d_records & 15) != 0) return fail(IVF_E_INVALID, "the record block must be 16-byte aligned");
    if (n_rounds < 1 || n_rounds > kMaxRounds) return fail(IVF_E_INVALID, "n_rounds %d outside [1,%d]", n_rounds, kMaxRounds);
    if (n_frames == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_frames, st);
    if (rc != IVF_OK) return rc;
    const size_t lds = (size_t)t->P.nf * sizeof(Edge);
    if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_pose_opt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_pose_opt, dim3(n_frames), dim3(kThreads), lds, st, pose_params(t->P, n_records), d_records, d_frames, d_xw, d_has_point,
                       d_quality, n_rounds, d_poses, d_outlier, d_ninliers, d_chi2);
    return tracker_end(t, st);
}

}  // extern "C"
