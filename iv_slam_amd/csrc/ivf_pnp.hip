// ivf_pnp.hip -- batched, device-resident PnPsolver (ORB/src/PnPsolver.cc): EPnP inside the RANSAC loop of Tracking::Relocalization
// (ORB/src/Tracking.cc:2272-2421), the call between SearchByBoW and PoseOptimization, on the tracker handle (ivf_tracker.h).  Restated
// in double, the arithmetic the reference runs it in: SetRansacParameters (:125-161), the body of iterate (:169-262), Refine (:264-309),
// CheckInliers (:312-343) and compute_pose with everything under it (:379-530, :554-956).  OpenCV's cvSVD / cvInvert / cvSolve(CV_SVD)
// are one cyclic one-sided Jacobi SVD here (jacobi_svd): fixed pair order, at most kSweeps sweeps.
//
//   k_pnp_prepare   one workgroup per frame: the 2D-3D correspondences of the constructor (:71-114) compacted in keypoint order, N,
//                   mRansacMinInliers and mRansacMaxIts; the early refusal N < mRansacMinInliers (:177-181).
//   k_pnp_hyp       one wave per (hypothesis, frame): hypotheses are independent of one another, so all mRansacMaxIts of them run at
//                   once.  The four sample indices come from the caller's rand() values through DUtils::Random::RandomInt and the
//                   swap-with-back removal of :192-205; compute_pose on 4 points; CheckInliers over all N.  Leaves the f64 pose and
//                   mnInliersi of every iteration in the handle's scratch.
//   k_pnp_replay    one workgroup (4 waves) per frame: the bookkeeping of :213-259 in iteration order.  Refine uses mvbBestInliers, so
//                   it can only change its answer at an iteration that raises mnBestInliers: it runs there (compute_pose over up to
//                   nfeatures points as a workgroup reduction) and nowhere else.  The first success returns mRefinedTcw; without one the
//                   best hypothesis is returned when it has mRansacMinInliers inliers.
// ivf_test_pnp_hypotheses (testing hook) runs the first two with k_pnp_hyp<true>, which also leaves the intermediate values of every
// hypothesis (sample, control points, the four vectors, the betas, every candidate's pose and error) in a buffer of doubles.
// compute_pose is one text for both sizes (template on the thread count).  The sums over points go through xor-butterflies in the wave and
// through LDS in wave order: the tree is fixed, two runs are bit-identical.  The 12x12 MtM, its vectors and every small matrix live in
// LDS; a Jacobi rotation is spread over lanes (one matrix row each).  Every loop has a compile-time bound: NaN cannot spin a kernel.
// The sums, the ordered compaction, the frame's pointer set and the pose I/O are ivf_solve.h's, shared with ivf_pose.hip; so are the
// sampler and the iteration count, shared with ivf_sim3.hip (their cap, argument checks and scratch allocation: ivf_tracker.h).
#include "ivf_solve.h"

using namespace ivf;

namespace {

constexpr int kRefThreads = 256;
constexpr int kSumCap = 80;                                           // the widest reduction: the 78 sums of MtM's upper triangle

struct PnpParams {
    int nf, nRecords;
    size_t recBytes;
    double fu, fv, uc, vc;                                            // PnPsolver's double members, set from the float F.fx ... (:108-111)
    float sigma2[kMaxLevels];                                         // mvLevelSigma2
    int maxIterations, minInliers;
    double probability;
    float epsilon, th2;
};

struct __attribute__((aligned(16))) Corr { float X[3]; float u, v, maxErr; int kp, pad; };   // mvP3Dw, mvP2D, mvMaxError, mvKeyPointIndices
static_assert(sizeof(Corr) == 32, "a correspondence is two 16-byte loads");

struct Ws {                                                           // LDS of one compute_pose
    double part[kRefThreads / 64][kSumCap], sum[kSumCap];
    double A[144], V[144], w[12];                                     // MtM (rotated in place), its right vectors, singular values
    double sA[30], sV[25], sw[5];                                     // the small SVDs: 3x3, 6x3, 6x4, 6x5
    double cws[4][3], ci[9], vv[4][12], L[60], rho[6], betas[4], ccs[4][3], pc0[3];
    double Rs[3][9], ts[3][3], err[3], R[9], t[3];
    double qa[24], qb[6], qx[4], q1[4], q2[4];
    int ord[12], sord[5];
};

// the K sums of acc[] over the workgroup -> S.sum[0..K)
template <int NT, int K>
DEVINL void block_sum(Ws& S, const double* acc, int tid)
{
    static_assert(K <= kSumCap, "S.sum");
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) S.part[wave][k] = v;
    }
    __syncthreads();
    for (int k = tid; k < K; k += NT) S.sum[k] = wave_order_sum<NT / 64>(&S.part[0][k], kSumCap);
    __syncthreads();
}

// One-sided cyclic Jacobi SVD of the m x n matrix A (row-major, m <= 12, n <= 12) in LDS: on return A = U diag(w), V holds the right
// vectors in its columns, w[j] the norm of column j, ord[] the columns by descending w.  The pairs (p, q) are visited in one fixed
// order; every lane computes the same rotation from the same LDS words, lane r < m turns row r of A, lane m + r row r of V.
template <int NT>
DEVINL void jacobi_svd(double* A, int m, int n, double* V, double* w, int* ord, int tid)
{
    for (int i = tid; i < n * n; i += NT) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    __syncthreads();
    double* row = tid < m ? A + tid * n : (tid < m + n ? V + (tid - m) * n : nullptr);
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        bool rotated = false;
#pragma unroll 1
        for (int p = 0; p < n - 1; p++)
#pragma unroll 1
            for (int q = p + 1; q < n; q++) {
                double a = 0.0, b = 0.0, g = 0.0;
                for (int k = 0; k < m; k++) { const double x = A[k * n + p], y = A[k * n + q]; a = a + x * x; b = b + y * y; g = g + x * y; }
                double c, s;
                if (!jacobi_rotation(a, b, g, c, s)) continue;         // orthogonal already (or NaN): the same answer in every lane
                rotated = true;
                double x = 0.0, y = 0.0;
                if (row) { x = row[p]; y = row[q]; }
                __syncthreads();                                       // every lane has read both columns
                if (row) { row[p] = c * x - s * y; row[q] = s * x + c * y; }
                __syncthreads();
            }
        if (!rotated) break;
    }
    if (tid < n) {
        double a = 0.0;
        for (int k = 0; k < m; k++) { const double x = A[k * n + tid]; a = a + x * x; }
        w[tid] = sqrt(a);
    }
    __syncthreads();
    if (tid == 0) {
        for (int j = 0; j < n; j++) ord[j] = j;
        for (int j = 1; j < n; j++)                                    // insertion sort, descending, stable
            for (int k = j; k > 0 && w[ord[k]] > w[ord[k - 1]]; k--) { const int v = ord[k]; ord[k] = ord[k - 1]; ord[k - 1] = v; }
    }
    __syncthreads();
}

// x = pinv(A0) b for the 6 x nc system whose jacobi_svd is (A, V, w): SVD::backSubst, singular values at or below 2 eps sum(w) dropped
DEVINL void svd_solve(const double* A, int nc, const double* V, const double* w, const double* b, double* x)
{
    double thr = 0.0;
    for (int j = 0; j < nc; j++) thr = thr + w[j];
    thr = thr * (2.0 * kEps);
    for (int i = 0; i < nc; i++) x[i] = 0.0;
    for (int j = 0; j < nc; j++) {
        if (!(w[j] > thr)) continue;
        double d = 0.0;
        for (int k = 0; k < 6; k++) d = d + A[k * nc + j] * b[k];
        d = d / w[j] / w[j];
        for (int i = 0; i < nc; i++) x[i] = x[i] + V[i * nc + j] * d;
    }
}

// qr_solve on the 6x4 system (:864-954), as written there: the pivot scale eta looks at rows k .. 4 of column k
DEVINL void qr_solve(double* a, double* b, double* x, double* A1, double* A2)
{
    const int nr = 6, nc = 4;
    for (int k = 0; k < nc; k++) {
        double eta = fabs(a[k * nc + k]);
        for (int i = k + 1; i < nr; i++) { const double elt = fabs(a[(i - 1) * nc + k]); if (eta < elt) eta = elt; }
        if (eta == 0) { A1[k] = 0.0; A2[k] = 0.0; return; }
        const double inv_eta = 1. / eta;
        double sum = 0.0;
        for (int i = k; i < nr; i++) { a[i * nc + k] = a[i * nc + k] * inv_eta; sum = sum + a[i * nc + k] * a[i * nc + k]; }
        double sigma = sqrt(sum);
        if (a[k * nc + k] < 0) sigma = -sigma;
        a[k * nc + k] = a[k * nc + k] + sigma;
        A1[k] = sigma * a[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s2 = 0.0;
            for (int i = k; i < nr; i++) s2 = s2 + a[i * nc + k] * a[i * nc + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < nr; i++) a[i * nc + j] = a[i * nc + j] - tau * a[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {                                     // b <- Qt b
        double tau = 0.0;
        for (int i = j; i < nr; i++) tau = tau + a[i * nc + j] * b[i];
        tau = tau / A1[j];
        for (int i = j; i < nr; i++) b[i] = b[i] - tau * a[i * nc + j];
    }
    x[nc - 1] = b[nc - 1] / A2[nc - 1];                                // X = R-1 b
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0.0;
        for (int j = i + 1; j < nc; j++) sum = sum + a[i * nc + j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
}

// gauss_newton (:844-862) with compute_A_and_b_gauss_newton (:816-842): 5 steps on S.betas
DEVINL void gauss_newton(Ws& S)
{
    double* bt = S.betas;
    for (int k = 0; k < 4; k++) S.qx[k] = 0.0;
    for (int it = 0; it < 5; it++) {
        for (int i = 0; i < 6; i++) {
            const double* r = S.L + 10 * i;
            double* ra = S.qa + 4 * i;
            ra[0] = 2 * r[0] * bt[0] + r[1] * bt[1] + r[3] * bt[2] + r[6] * bt[3];
            ra[1] = r[1] * bt[0] + 2 * r[2] * bt[1] + r[4] * bt[2] + r[7] * bt[3];
            ra[2] = r[3] * bt[0] + r[4] * bt[1] + 2 * r[5] * bt[2] + r[8] * bt[3];
            ra[3] = r[6] * bt[0] + r[7] * bt[1] + r[8] * bt[2] + 2 * r[9] * bt[3];
            S.qb[i] = S.rho[i] - (r[0] * bt[0] * bt[0] + r[1] * bt[0] * bt[1] + r[2] * bt[1] * bt[1] + r[3] * bt[0] * bt[2] + r[4] * bt[1] * bt[2] +
                                  r[5] * bt[2] * bt[2] + r[6] * bt[0] * bt[3] + r[7] * bt[1] * bt[3] + r[8] * bt[2] * bt[3] + r[9] * bt[3] * bt[3]);
        }
        qr_solve(S.qa, S.qb, S.qx, S.q1, S.q2);
        for (int i = 0; i < 4; i++) bt[i] = bt[i] + S.qx[i];
    }
}

struct Alpha { double cw0[3], ci[9]; };
DEVINL Alpha load_alpha(const Ws& S)
{
    Alpha a;
#pragma unroll
    for (int j = 0; j < 3; j++) a.cw0[j] = S.cws[0][j];
#pragma unroll
    for (int j = 0; j < 9; j++) a.ci[j] = S.ci[j];
    return a;
}
// compute_barycentric_coordinates (:427-437) of one point
DEVINL void alphas_of(const Alpha& B, const Corr& c, double a[4])
{
    const double d0 = (double)c.X[0] - B.cw0[0], d1 = (double)c.X[1] - B.cw0[1], d2 = (double)c.X[2] - B.cw0[2];
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = B.ci[3 * j] * d0 + B.ci[3 * j + 1] * d1 + B.ci[3 * j + 2] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// CheckInliers (:316-342) of one correspondence under [R | t]: Xc, Yc, invZc, distX, distY, error2 are float, ue, ve double
DEVINL bool is_inlier(const double* R, const double* t, double fu, double fv, double uc, double vc, const Corr& c)
{
    const float Xc = (float)(R[0] * c.X[0] + R[1] * c.X[1] + R[2] * c.X[2] + t[0]);
    const float Yc = (float)(R[3] * c.X[0] + R[4] * c.X[1] + R[5] * c.X[2] + t[1]);
    const float invZc = (float)(1 / (R[6] * c.X[0] + R[7] * c.X[1] + R[8] * c.X[2] + t[2]));
    const double ue = uc + fu * Xc * invZc;
    const double ve = vc + fv * Yc * invZc;
    const float distX = (float)(c.u - ue);
    const float distY = (float)(c.v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < c.maxErr;
}

// The record of doubles ivf_test_pnp_hypotheses receives per hypothesis (include/ivfront.h)
constexpr int kTapSample = 0, kTapCws = 4, kTapVv = 16, kTapW = 64, kTapCand = 76, kTapCandStride = 21, kTapBest = 139, kTapDoubles = IVF_PNP_TAP_DOUBLES;
static_assert(kTapCand + 3 * kTapCandStride == kTapBest && kTapBest + 1 == kTapDoubles, "the record of include/ivfront.h");

// compute_pose (:481-529) over the n correspondences corr[list[0 .. n)] -> S.R, S.t.  Called by all NT threads of the workgroup.
// TAP: the testing hook's instantiation also leaves its intermediate values in tap[0 .. kTapDoubles); the product's has no such code.
template <int NT, bool TAP = false>
DEVINL void compute_pose(Ws& S, const PnpParams& P, const Corr* __restrict__ corr, const unsigned short* list, int n, int tid, double* tap = nullptr)
{
    const double fu = P.fu, fv = P.fv, uc = P.uc, vc = P.vc, dn = (double)n;
    // ---- choose_control_points (:379-413)
    {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = tid; j < n; j += NT) {
            const Corr c = corr[list[j]];
#pragma unroll
            for (int k = 0; k < 3; k++) acc[k] = acc[k] + (double)c.X[k];
        }
        block_sum<NT, 3>(S, acc, tid);
        if (tid < 3) S.cws[0][tid] = S.sum[tid] / dn;
        __syncthreads();
    }
    {
        const double c0 = S.cws[0][0], c1 = S.cws[0][1], c2 = S.cws[0][2];
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = tid; j < n; j += NT) {
            const Corr c = corr[list[j]];
            const double x = (double)c.X[0] - c0, y = (double)c.X[1] - c1, z = (double)c.X[2] - c2;
            acc[0] = acc[0] + x * x; acc[1] = acc[1] + x * y; acc[2] = acc[2] + x * z;
            acc[3] = acc[3] + y * y; acc[4] = acc[4] + y * z; acc[5] = acc[5] + z * z;
        }
        block_sum<NT, 6>(S, acc, tid);
        if (tid == 0) {
            S.sA[0] = S.sum[0]; S.sA[1] = S.sum[1]; S.sA[2] = S.sum[2];
            S.sA[3] = S.sum[1]; S.sA[4] = S.sum[3]; S.sA[5] = S.sum[4];
            S.sA[6] = S.sum[2]; S.sA[7] = S.sum[4]; S.sA[8] = S.sum[5];
        }
        __syncthreads();
        jacobi_svd<NT>(S.sA, 3, 3, S.sV, S.sw, S.sord, tid);          // PW0tPW0 is symmetric: its SVD is its eigen-decomposition
        if (tid == 0) {
            for (int i = 1; i < 4; i++) {
                const int col = S.sord[i - 1];
                // the sign of a principal axis is the SVD's accident, and on noisy data the pose depends on it (mirrored control points):
                // every axis is turned so that its component of largest magnitude (the first such) is positive
                int big = 0;
                for (int j = 1; j < 3; j++) if (fabs(S.sV[3 * j + col]) > fabs(S.sV[3 * big + col])) big = j;
                const double sg = S.sV[3 * big + col] < 0 ? -1.0 : 1.0;
                const double k = sqrt(S.sw[col] / dn);
                for (int j = 0; j < 3; j++) S.cws[i][j] = S.cws[0][j] + k * (sg * S.sV[3 * j + col]);
            }
            // ---- compute_barycentric_coordinates (:415-425): CC and its inverse by SVD
            for (int i = 0; i < 3; i++)
                for (int j = 1; j < 4; j++) S.sA[3 * i + j - 1] = S.cws[j][i] - S.cws[0][i];
        }
        __syncthreads();
        jacobi_svd<NT>(S.sA, 3, 3, S.sV, S.sw, S.sord, tid);
        if (tid == 0) {
            const double thr = (S.sw[0] + S.sw[1] + S.sw[2]) * (2.0 * kEps);
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) {
                    double v = 0.0;
                    for (int j = 0; j < 3; j++)
                        if (S.sw[j] > thr) v = v + S.sV[3 * r + j] * (S.sA[3 * c + j] / S.sw[j] / S.sw[j]);
                    S.ci[3 * r + c] = v;
                }
        }
        __syncthreads();
    }
    const Alpha B = load_alpha(S);
    // ---- fill_M (:440-455) and MtM (:496): the 78 sums of the upper triangle
    {
        double acc[78];
#pragma unroll
        for (int k = 0; k < 78; k++) acc[k] = 0.0;
        for (int j = tid; j < n; j += NT) {
            const Corr c = corr[list[j]];
            double a[4], M1[12], M2[12];
            alphas_of(B, c, a);
            const double du = uc - (double)c.u, dv = vc - (double)c.v;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                M1[3 * i] = a[i] * fu; M1[3 * i + 1] = 0.0; M1[3 * i + 2] = a[i] * du;
                M2[3 * i] = 0.0; M2[3 * i + 1] = a[i] * fv; M2[3 * i + 2] = a[i] * dv;
            }
            int k = 0;
#pragma unroll
            for (int r = 0; r < 12; r++)
#pragma unroll
                for (int cc = r; cc < 12; cc++, k++) { acc[k] = acc[k] + M1[r] * M1[cc]; acc[k] = acc[k] + M2[r] * M2[cc]; }
        }
        block_sum<NT, 78>(S, acc, tid);
        for (int i = tid; i < 144; i += NT) {
            const int r0 = i / 12, c0 = i % 12, r = r0 < c0 ? r0 : c0, c = r0 < c0 ? c0 : r0;
            S.A[i] = S.sum[r * 12 - (r * (r - 1)) / 2 + (c - r)];
        }
        __syncthreads();
        jacobi_svd<NT>(S.A, 12, 12, S.V, S.w, S.ord, tid);
    }
    // ---- the four vectors of the smallest singular values (ut + 12 * (11 - i)), compute_L_6x10 (:764-804), compute_rho (:806-814)
    if (tid < 48) { const int i = tid / 12, e = tid % 12; S.vv[i][e] = S.V[e * 12 + S.ord[11 - i]]; }
    __syncthreads();
    if constexpr (TAP) {
        if (tid < 12) { tap[kTapCws + tid] = S.cws[tid / 3][tid % 3]; tap[kTapW + tid] = S.w[S.ord[tid]]; }
        if (tid < 48) tap[kTapVv + tid] = S.vv[tid / 12][tid % 12];
    }
    if (tid == 0) {
        for (int i = 0; i < 6; i++) {
            // pair i of (a, b): (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
            const int a = i < 3 ? 0 : (i < 5 ? 1 : 2), b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
            double dv[4][3];
            for (int v = 0; v < 4; v++)
                for (int k = 0; k < 3; k++) dv[v][k] = S.vv[v][3 * a + k] - S.vv[v][3 * b + k];
            auto dot = [&](int x, int y) { return dv[x][0] * dv[y][0] + dv[x][1] * dv[y][1] + dv[x][2] * dv[y][2]; };
            double* row = S.L + 10 * i;
            row[0] = dot(0, 0); row[1] = 2.0 * dot(0, 1); row[2] = dot(1, 1); row[3] = 2.0 * dot(0, 2); row[4] = 2.0 * dot(1, 2);
            row[5] = dot(2, 2); row[6] = 2.0 * dot(0, 3); row[7] = 2.0 * dot(1, 3); row[8] = 2.0 * dot(2, 3); row[9] = dot(3, 3);
            const double* p1 = S.cws[a]; const double* p2 = S.cws[b];
            S.rho[i] = (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
        }
    }
    __syncthreads();
    // ---- the three candidates (:510-520)
#pragma unroll 1
    for (int cand = 0; cand < 3; cand++) {
        const int nc = cand == 0 ? 4 : (cand == 1 ? 3 : 5);
        if (tid == 0) {
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < nc; j++) {
                    const int col = cand == 0 ? (j == 0 ? 0 : (j == 1 ? 1 : (j == 2 ? 3 : 6))) : j;   // approx_1: B11 B12 B13 B14
                    S.sA[i * nc + j] = S.L[10 * i + col];
                }
        }
        __syncthreads();
        jacobi_svd<NT>(S.sA, 6, nc, S.sV, S.sw, S.sord, tid);
        if (tid == 0) {
            double b[5];
            double* bt = S.betas;
            svd_solve(S.sA, nc, S.sV, S.sw, S.rho, b);
            if (cand == 0) {                                           // find_betas_approx_1 (:671-698)
                if (b[0] < 0) { bt[0] = sqrt(-b[0]); bt[1] = -b[1] / bt[0]; bt[2] = -b[2] / bt[0]; bt[3] = -b[3] / bt[0]; }
                else { bt[0] = sqrt(b[0]); bt[1] = b[1] / bt[0]; bt[2] = b[2] / bt[0]; bt[3] = b[3] / bt[0]; }
            } else {                                                   // find_betas_approx_2 / _3 (:703-762)
                if (b[0] < 0) { bt[0] = sqrt(-b[0]); bt[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0; }
                else { bt[0] = sqrt(b[0]); bt[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0; }
                if (b[1] < 0) bt[0] = -bt[0];
                bt[2] = cand == 1 ? 0.0 : b[3] / bt[0];
                bt[3] = 0.0;
            }
            if constexpr (TAP)
                for (int k = 0; k < 4; k++) tap[kTapCand + kTapCandStride * cand + k] = bt[k];
            gauss_newton(S);
            if constexpr (TAP)
                for (int k = 0; k < 4; k++) tap[kTapCand + kTapCandStride * cand + 4 + k] = bt[k];
            // compute_ccs (:457-468), and solve_for_sign (:640-653) on the first point's pcs[2]
            for (int j = 0; j < 4; j++)
                for (int k = 0; k < 3; k++) S.ccs[j][k] = 0.0;
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++)
                    for (int k = 0; k < 3; k++) S.ccs[j][k] = S.ccs[j][k] + bt[i] * S.vv[i][3 * j + k];
            double a[4];
            alphas_of(B, corr[list[0]], a);
            const double z0 = a[0] * S.ccs[0][2] + a[1] * S.ccs[1][2] + a[2] * S.ccs[2][2] + a[3] * S.ccs[3][2];
            if (z0 < 0.0)
                for (int j = 0; j < 4; j++)
                    for (int k = 0; k < 3; k++) S.ccs[j][k] = -S.ccs[j][k];
        }
        __syncthreads();
        // ---- estimate_R_and_t (:573-631); compute_pcs (:470-479) per point, not stored
        double cc[4][3];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) cc[j][k] = S.ccs[j][k];
        {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int j = tid; j < n; j += NT) {
                double a[4];
                alphas_of(B, corr[list[j]], a);
#pragma unroll
                for (int k = 0; k < 3; k++) acc[k] = acc[k] + (a[0] * cc[0][k] + a[1] * cc[1][k] + a[2] * cc[2][k] + a[3] * cc[3][k]);
            }
            block_sum<NT, 3>(S, acc, tid);
            if (tid < 3) S.pc0[tid] = S.sum[tid] / dn;
            __syncthreads();
        }
        {
            const double pc0[3] = {S.pc0[0], S.pc0[1], S.pc0[2]};
            double acc[9];
#pragma unroll
            for (int k = 0; k < 9; k++) acc[k] = 0.0;
            for (int j = tid; j < n; j += NT) {
                const Corr c = corr[list[j]];
                double a[4];
                alphas_of(B, c, a);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double pc = a[0] * cc[0][k] + a[1] * cc[1][k] + a[2] * cc[2][k] + a[3] * cc[3][k];
#pragma unroll
                    for (int l = 0; l < 3; l++) acc[3 * k + l] = acc[3 * k + l] + (pc - pc0[k]) * ((double)c.X[l] - B.cw0[l]);   // pw0 is cws[0]
                }
            }
            block_sum<NT, 9>(S, acc, tid);
            if (tid < 9) S.sA[tid] = S.sum[tid];
            __syncthreads();
            jacobi_svd<NT>(S.sA, 3, 3, S.sV, S.sw, S.sord, tid);
            if (tid == 0) {
                // R = U Vt with U = the normalised columns of the rotated matrix; a vanishing third singular value leaves its column to
                // the cross product of the other two
                double U[9];
                const double thr = (S.sw[0] + S.sw[1] + S.sw[2]) * (2.0 * kEps);
                for (int k = 0; k < 3; k++)
                    for (int i = 0; i < 3; i++) U[3 * i + k] = S.sA[3 * i + k] / S.sw[k];
                const int k0 = S.sord[0], k1 = S.sord[1], k2 = S.sord[2];
                if (!(S.sw[k2] > thr)) {
                    U[k2] = U[3 + k0] * U[6 + k1] - U[6 + k0] * U[3 + k1];
                    U[3 + k2] = U[6 + k0] * U[k1] - U[k0] * U[6 + k1];
                    U[6 + k2] = U[k0] * U[3 + k1] - U[3 + k0] * U[k1];
                }
                double* R = S.Rs[cand];
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * S.sV[3 * j] + U[3 * i + 1] * S.sV[3 * j + 1] + U[3 * i + 2] * S.sV[3 * j + 2];
                const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
                if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
                for (int i = 0; i < 3; i++) S.ts[cand][i] = S.pc0[i] - (R[3 * i] * B.cw0[0] + R[3 * i + 1] * B.cw0[1] + R[3 * i + 2] * B.cw0[2]);
            }
            __syncthreads();
        }
        // ---- reprojection_error (:554-571)
        {
            double R[9], t[3];
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = S.Rs[cand][k];
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = S.ts[cand][k];
            double acc[1] = {0.0};
            for (int j = tid; j < n; j += NT) {
                const Corr c = corr[list[j]];
                const double X = (double)c.X[0], Y = (double)c.X[1], Z = (double)c.X[2];
                const double Xc = R[0] * X + R[1] * Y + R[2] * Z + t[0], Yc = R[3] * X + R[4] * Y + R[5] * Z + t[1];
                const double inv_Zc = 1.0 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]);
                const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc, u = (double)c.u, v = (double)c.v;
                acc[0] = acc[0] + sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
            }
            block_sum<NT, 1>(S, acc, tid);
            if (tid == 0) S.err[cand] = S.sum[0] / dn;
            __syncthreads();
        }
    }
    if (tid == 0) {
        int best = 0;                                                  // :522-524
        if (S.err[1] < S.err[0]) best = 1;
        if (S.err[2] < S.err[best]) best = 2;
        for (int k = 0; k < 9; k++) S.R[k] = S.Rs[best][k];
        for (int k = 0; k < 3; k++) S.t[k] = S.ts[best][k];
        if constexpr (TAP) {
            for (int c = 0; c < 3; c++) {
                double* o = tap + kTapCand + kTapCandStride * c + 8;
                for (int k = 0; k < 9; k++) o[k] = S.Rs[c][k];
                for (int k = 0; k < 3; k++) o[9 + k] = S.ts[c][k];
                o[12] = S.err[c];
            }
            tap[kTapBest] = (double)best;
        }
    }
    __syncthreads();
}
// its result, in registers
DEVINL void load_solution(const Ws& S, double* R, double* t)
{
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = S.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = S.t[k];
}

// mnInliersi of the pose (R, t) in registers over corr[0 .. N); with `list`, also the indices of the inliers in order (NT == kRefThreads)
template <int NT>
DEVINL int count_inliers(const PnpParams& P, const double* R, const double* t, const Corr* __restrict__ corr, int N, int tid, int* s_wcnt,
                         unsigned short* list)
{
    return compact_ordered<NT>(N, s_wcnt, tid, [&](int i) { return is_inlier(R, t, P.fu, P.fv, P.uc, P.vc, corr[i]); },
                               [&](int i, int slot) { if (list) list[slot] = (unsigned short)i; });
}

// ---- the correspondences and the RANSAC parameters of every frame --------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pnp_prepare(PnpParams P, const uint8_t* __restrict__ records, const int* __restrict__ frames,
                                                     const float* __restrict__ xw, const uint8_t* __restrict__ hasPoint, Corr* __restrict__ corrAll,
                                                     int4* __restrict__ head, uint8_t* __restrict__ inlierOut, int* __restrict__ nInliers,
                                                     int* __restrict__ iterations)
{
    __shared__ int s_wcnt[4];
    const int f = blockIdx.x, tid = threadIdx.x, nf = P.nf;
    const FrameObs O = frame_obs(records, P.recBytes, nf, P.nRecords, frames[f], xw, hasPoint, f);
    if (O.nC < 0) {                                                    // nothing of this frame is touched
        if (tid == 0) { nInliers[f] = -1; head[f] = make_int4(0, 0, 0, 0); }
        return;
    }
    uint8_t* inl = inlierOut + (size_t)f * nf;
    for (int i = tid; i < nf; i += 256) inl[i] = 0;
    Corr* corr = corrAll + (size_t)f * nf;
    const int N = compact_ordered<256>(O.nC, s_wcnt, tid, [&](int i) { return O.has[i] != 0; }, [&](int i, int slot) {
        const ivf_keypoint kp = O.kps[i];
        Corr c;
        c.X[0] = O.X[3 * i]; c.X[1] = O.X[3 * i + 1]; c.X[2] = O.X[3 * i + 2];
        c.u = kp.x; c.v = kp.y;
        c.maxErr = P.sigma2[clamp_octave(kp.octave)] * P.th2;          // mvMaxError[i] = mvSigma2[i] * th2, in float (:160)
        c.kp = i; c.pad = 0;
        corr[slot] = c;
    });
    if (tid == 0) {
        // SetRansacParameters (:137-156)
        float eps = P.epsilon;
        int nMin = (int)((float)N * eps);
        if (nMin < P.minInliers) nMin = P.minInliers;
        if (nMin < 4) nMin = 4;                                        // minSet
        int its = 0;
        if (N >= nMin) {                                               // else :177-181: no pose, no iteration
            if (eps < (float)nMin / (float)N) eps = (float)nMin / (float)N;
            its = ransac_iterations(P.probability, eps, nMin == N, P.maxIterations);
        }
        head[f] = make_int4(N, nMin, its, 0);
        if (its == 0) { nInliers[f] = 0; if (iterations) iterations[f] = 0; }
    }
}

// ---- one hypothesis ------------------------------------------------------------------------------------------------------------------
// TAP (ivf_test_pnp_hypotheses): also one record of taps per hypothesis it runs; the product launches k_pnp_hyp<false>, taps == nullptr
template <bool TAP>
__global__ __launch_bounds__(64) void k_pnp_hyp(PnpParams P, const Corr* __restrict__ corrAll, const int4* __restrict__ head,
                                                const uint32_t* __restrict__ draws, double* __restrict__ hypPose, int* __restrict__ hypN,
                                                float* __restrict__ outPoses, int* __restrict__ outN, double* __restrict__ taps)
{
    __shared__ Ws S;
    __shared__ unsigned short s_list[4];
    __shared__ int s_wcnt[1];
    const int it = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int4 h = head[f];
    if (it >= h.z) return;
    const int N = h.x;
    const Corr* corr = corrAll + (size_t)f * P.nf;
    const size_t slot = (size_t)f * P.maxIterations + it;
    if (tid == 0) {
        int smp[4];
        ransac_sample<4>(draws + slot * 4, N, smp);                    // :192-205
#pragma unroll
        for (int k = 0; k < 4; k++) s_list[k] = (unsigned short)smp[k];
    }
    __syncthreads();
    double* tap = TAP ? taps + slot * kTapDoubles : nullptr;
    if constexpr (TAP)
        if (tid < 4) tap[kTapSample + tid] = (double)s_list[tid];
    compute_pose<64, TAP>(S, P, corr, s_list, 4, tid, tap);
    double R[9], t[3];
    load_solution(S, R, t);
    const int ni = count_inliers<64>(P, R, t, corr, N, tid, s_wcnt, nullptr);
    if (tid == 0) {
        store_pose(hypPose + slot * 12, R, t);
        hypN[slot] = ni;
        if (outN) outN[slot] = ni;
        if (outPoses) store_pose(outPoses + slot * 12, R, t);
    }
}

// ---- the sequential bookkeeping of iterate(), Refine where it can change its answer ------------------------------------------------------
__global__ __launch_bounds__(kRefThreads) void k_pnp_replay(PnpParams P, const Corr* __restrict__ corrAll, const int4* __restrict__ head,
                                                            const double* __restrict__ hypPose, const int* __restrict__ hypN,
                                                            float* __restrict__ poses, uint8_t* __restrict__ inlierOut, int* __restrict__ nInliers,
                                                            int* __restrict__ iterations)
{
    extern __shared__ unsigned short s_list[];                         // [nf] the inlier indices Refine solves on, then those it returns
    __shared__ Ws S;
    __shared__ int s_wcnt[kRefThreads / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int4 h = head[f];
    const int N = h.x, minInl = h.y, maxIts = h.z;
    if (maxIts < 1) return;                                            // k_pnp_prepare has answered
    const Corr* corr = corrAll + (size_t)f * P.nf;
    uint8_t* inl = inlierOut + (size_t)f * P.nf;
    float* T = poses + (size_t)f * 12;
    int best = 0, bestIt = -1;
    double R[9], t[3];
    // the answer: the pose (R, t) with its n inliers s_list[0 .. n)
    auto publish = [&](int n) {
        for (int j = tid; j < n; j += kRefThreads) inl[corr[s_list[j]].kp] = 1;
        if (tid == 0) { store_pose(T, R, t); nInliers[f] = n; }
    };
#pragma unroll 1
    for (int it = 0; it < kRansacMaxIterations; it++) {
        if (it >= maxIts) break;
        const size_t slot = (size_t)f * P.maxIterations + it;
        const int ni = hypN[slot];
        if (!(ni >= minInl && ni > best)) continue;                    // Refine on an unchanged mvbBestInliers fails as it did before
        best = ni; bestIt = it;
        load_hyp(hypPose + slot * 12, R, t);
        const int nb = count_inliers<kRefThreads>(P, R, t, corr, N, tid, s_wcnt, s_list);   // mvbBestInliers (nb == ni)
        compute_pose<kRefThreads>(S, P, corr, s_list, nb, tid);        // Refine (:264-309)
        load_solution(S, R, t);
        const int nr = count_inliers<kRefThreads>(P, R, t, corr, N, tid, s_wcnt, s_list);   // mvbRefinedInliers
        if (nr > minInl) {                                             // strict (:296)
            publish(nr);
            if (tid == 0 && iterations) iterations[f] = it + 1;
            return;
        }
    }
    if (tid == 0 && iterations) iterations[f] = maxIts;
    if (bestIt < 0) { if (tid == 0) nInliers[f] = 0; return; }         // mnBestInliers < mRansacMinInliers: cv::Mat()
    load_hyp(hypPose + ((size_t)f * P.maxIterations + bestIt) * 12, R, t);
    publish(count_inliers<kRefThreads>(P, R, t, corr, N, tid, s_wcnt, s_list));
}

}  // namespace

// What the two entry points below share: the argument checks, the handle's scratch at its first use, the uniform arguments, and the first
// launch.  inlier / nInliers / iterations are k_pnp_prepare's outputs.
static int pnp_begin(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, int n_frames, int max_iterations, double probability,
                     int min_inliers, float epsilon, float th2, hipStream_t st, PnpParams& P)
{
    const int ra = ransac_args_ok(d_records, max_iterations, probability, min_inliers);
    if (ra != IVF_OK) return ra;
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(IVF_E_INVALID, "epsilon %g outside [0,1]", (double)epsilon);
    if (!(th2 > 0.0f)) return fail(IVF_E_INVALID, "min_inliers must be >= 0 and th2 positive");
    if (n_frames == 0) return IVF_OK;
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_frames, st);
    if (rc != IVF_OK) return rc;
    if (!t->pnp.corr) {                                                // first use: the scratch of ONE call, sized by max_pairs
        const size_t np = (size_t)t->cfg.max_pairs, nf = (size_t)t->P.nf;
        if (!t->replace({{t->pnp.corr, np * nf * sizeof(Corr)}, {t->pnp.head, np * sizeof(int4)},
                         {t->pnp.hypPose, np * kRansacMaxIterations * 12 * sizeof(double)}, {t->pnp.hypN, np * kRansacMaxIterations * sizeof(int)}}))
            return fail(IVF_E_NO_DEVICE, "device allocation failed for the PnP scratch of %d frames x %d features", t->cfg.max_pairs, t->P.nf);
    }
    P.nf = t->P.nf; P.nRecords = n_records; P.recBytes = t->P.recBytes;
    P.fu = (double)t->P.fx; P.fv = (double)t->P.fy; P.uc = (double)t->P.cx; P.vc = (double)t->P.cy;
    level_sigma2(t->P, P.sigma2);
    P.maxIterations = max_iterations; P.minInliers = min_inliers; P.probability = probability; P.epsilon = epsilon; P.th2 = th2;
    return IVF_OK;
}

extern "C" {

int ivf_tracker_solve_pnp(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames, int n_frames,
                          const float* d_xw, const uint8_t* d_has_point, const uint32_t* d_draws, int max_iterations, double probability,
                          int min_inliers, float epsilon, float th2, float* d_poses, uint8_t* d_inlier, int32_t* d_ninliers, int32_t* d_iterations,
                          float* d_hyp_poses, int32_t* d_hyp_ninliers, void* hip_stream)
{
    if (!t || !d_records || !d_frames || !d_xw || !d_has_point || !d_draws || !d_poses || !d_inlier || !d_ninliers) return fail(IVF_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)hip_stream;
    PnpParams P;
    const int rc = pnp_begin(t, d_records, record_bytes, n_records, n_frames, max_iterations, probability, min_inliers, epsilon, th2, st, P);
    if (rc != IVF_OK || n_frames == 0) return rc;
    Corr* corr = (Corr*)t->pnp.corr;
    int4* head = (int4*)t->pnp.head;
    hipLaunchKernelGGL(k_pnp_prepare, dim3(n_frames), dim3(256), 0, st, P, d_records, d_frames, d_xw, d_has_point, corr, head, d_inlier, d_ninliers,
                       d_iterations);
    hipLaunchKernelGGL(k_pnp_hyp<false>, dim3(max_iterations, n_frames), dim3(64), 0, st, P, (const Corr*)corr, (const int4*)head, d_draws, t->pnp.hypPose,
                       t->pnp.hypN, d_hyp_poses, d_hyp_ninliers, (double*)nullptr);
    hipLaunchKernelGGL(k_pnp_replay, dim3(n_frames), dim3(kRefThreads), (size_t)P.nf * sizeof(unsigned short), st, P, (const Corr*)corr,
                       (const int4*)head, (const double*)t->pnp.hypPose, (const int*)t->pnp.hypN, d_poses, d_inlier, d_ninliers, d_iterations);
    return tracker_end(t, st);
}

// testing hook (see include/ivfront.h).  k_pnp_prepare's vbInliers reset and nInliers have no caller here: they go to the scratch that
// k_pnp_hyp, the next launch on the stream, fills afterwards (hypPose holds 300 * 96 bytes per frame, hypN 300 ints).
int ivf_test_pnp_hypotheses(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames, int n_frames,
                            const float* d_xw, const uint8_t* d_has_point, const uint32_t* d_draws, int max_iterations, double probability,
                            int min_inliers, float epsilon, float th2, double* d_taps, float* d_hyp_poses, int32_t* d_hyp_ninliers, void* hip_stream)
{
    static_assert((size_t)kMaxTrackFeatures <= (size_t)kRansacMaxIterations * 12 * sizeof(double), "nfeatures flags fit a frame's hypPose rows");
    if (!t || !d_records || !d_frames || !d_xw || !d_has_point || !d_draws || !d_taps || !d_hyp_poses || !d_hyp_ninliers)
        return fail(IVF_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)hip_stream;
    PnpParams P;
    const int rc = pnp_begin(t, d_records, record_bytes, n_records, n_frames, max_iterations, probability, min_inliers, epsilon, th2, st, P);
    if (rc != IVF_OK || n_frames == 0) return rc;
    Corr* corr = (Corr*)t->pnp.corr;
    int4* head = (int4*)t->pnp.head;
    hipLaunchKernelGGL(k_pnp_prepare, dim3(n_frames), dim3(256), 0, st, P, d_records, d_frames, d_xw, d_has_point, corr, head, (uint8_t*)t->pnp.hypPose,
                       t->pnp.hypN, (int*)nullptr);
    hipLaunchKernelGGL(k_pnp_hyp<true>, dim3(max_iterations, n_frames), dim3(64), 0, st, P, (const Corr*)corr, (const int4*)head, d_draws, t->pnp.hypPose,
                       t->pnp.hypN, d_hyp_poses, d_hyp_ninliers, d_taps);
    return tracker_end(t, st);
}

}  // extern "C"
