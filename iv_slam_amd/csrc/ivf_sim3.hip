// ivf_sim3.hip -- batched, device-resident Sim3Solver (ORB/src/Sim3Solver.cc): Horn's closed form on three point pairs inside the RANSAC
// loop of LoopClosing::ComputeSim3 (ORB/src/LoopClosing.cc:279-306), the call between SearchByBoW(KF, KF) and SearchBySim3, on the
// tracker handle (ivf_tracker.h).  Restated with the arithmetic DESIGN.md A-15 freezes: the constructor (:40-115), SetRansacParameters
// (:117-141), the body of iterate (:143-210), ComputeSim3 (:229-340), CheckInliers (:343-367), Project and FromCameraToImage (:385-426).
//
//   k_sim3_prepare  one workgroup per pair: the 3D-3D correspondences of the constructor compacted in i1 order (both camera-frame points,
//                   both image points, both integer error bounds: three 16-byte loads each), N, the effective mRansacMaxIts, the state on
//                   entry and the early refusal N < mRansacMinInliers (:149-153).
//   k_sim3_hyp      one wave per (iteration, pair), from the state's mnIterations on: hypotheses are independent of one another.  The
//                   three sample indices come from the caller's rand() values through DUtils::Random::RandomInt and the swap-with-back
//                   removal of :169-180; ComputeSim3 is a few hundred flops and runs the same in every lane, in registers; CheckInliers
//                   is the parallel part, lanes stride over N and count by ballot.  Leaves (mR12i, mt12i, ms12i) and mnInliersi of every
//                   iteration in the handle's scratch, no mask.
//   k_sim3_replay   one wave per pair: the bookkeeping of :186-203 in iteration order (>= replaces the best, > mRansacMinInliers
//                   succeeds); the mask of the one iteration that succeeds is computed again from its stored transform (the same text,
//                   the same bits), written by i1, with the state the next call resumes from.
// cv::eigen of the symmetric 4x4 N is a cyclic two-sided Jacobi in f64 (jacobi_eigen4): fixed pair order, at most kSweeps sweeps, so a
// NaN cannot spin a kernel; a degenerate sample (norm(vec) == 0, e.g. a pure translation whose N is diagonal) gives NaN, no inlier, and
// falls through like any other hypothesis.  The ordered compaction, the pose I/O and the level table are ivf_solve.h's; so are the
// sampler and the iteration count, shared with ivf_pnp.hip (their cap, argument checks and scratch allocation: ivf_tracker.h).
#include "ivf_solve.h"

using namespace ivf;

namespace {

struct Sim3Params {
    int nf, nRecords;
    size_t recBytes;
    float fx, fy, cx, cy;                                             // mK1 == mK2: both keyframes are the handle's camera (:108-109)
    float sigma2[kMaxLevels];                                         // mvLevelSigma2
    int maxIterations, minInliers, fixScale;
    double probability;
};

// mvX3Dc1 / mvX3Dc2, mvnMaxError1 / 2 (integers, kept as the float they are compared as), mvP1im1, mvP2im2 of one correspondence
struct __attribute__((aligned(16))) Corr3 { float X1[3], e1; float X2[3], e2; float u1, v1, u2, v2; };
static_assert(sizeof(Corr3) == 48, "a correspondence is three 16-byte loads");

struct Sim3 { float R[9], t[3], s; };                                 // mR12i, mt12i, ms12i
struct Sim3T { float A12[9], b12[3], A21[9], b21[3]; };               // the upper 3x4 of mT12i and mT21i

// cv::Mat product row: (float) of the double sum of three CV_32F products, then + c
DEVINL double dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

// FromCameraToImage (:418-424) and the tail of Project (:400-404): invz = 1 / z with no test of its sign, everything in float
DEVINL void to_image(const Sim3Params& P, const float* Xc, float& u, float& v)
{
    const float invz = 1 / Xc[2];
    const float x = Xc[0] * invz, y = Xc[1] * invz;
    u = P.fx * x + P.cx; v = P.fy * y + P.cy;
}

// cv::eigen of a symmetric 4x4: cyclic two-sided Jacobi.  On return the diagonal of A holds the eigenvalues, the columns of V the
// vectors.  Every index is a compile-time constant after unrolling: both matrices stay in registers.  An element at or below
// DBL_EPSILON times the largest magnitude of the input is left alone; a sweep that turns nothing ends the iteration.
DEVINL void jacobi_eigen4(double (&A)[4][4], double (&V)[4][4])
{
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            V[i][j] = i == j ? 1.0 : 0.0;
            if (!(fabs(A[i][j]) <= big)) big = fabs(A[i][j]);           // a NaN makes the threshold NaN: nothing turns
        }
    const double thr = kEps * big;
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                if (!(fabs(apq) > thr)) continue;
                rotated = true;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double tn = copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
                A[p][p] = A[p][p] - tn * apq; A[q][q] = A[q][q] + tn * apq;
                A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k != p && k != q) {
                        const double x = A[k][p], y = A[k][q];
                        A[k][p] = c * x - s * y; A[p][k] = A[k][p];
                        A[k][q] = s * x + c * y; A[q][k] = A[k][q];
                    }
                    const double vx = V[k][p], vy = V[k][q];
                    V[k][p] = c * vx - s * vy; V[k][q] = s * vx + c * vy;
                }
            }
        if (!rotated) break;
    }
}

// ComputeSim3 (:229-319) on the sample p1[k] = P1.col(k), p2[k] = P2.col(k)
DEVINL Sim3 compute_sim3(const float (&p1)[3][3], const float (&p2)[3][3], bool fixScale)
{
    Sim3 S;
    // Step 1 (:218-227): cv::reduce sums in double; C / P.cols is the float product with (float)(1. / 3)
    const float third = (float)(1.0 / 3.0);
    float O1[3], O2[3], r1[3][3], r2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        O1[i] = (float)(((double)p1[0][i] + (double)p1[1][i]) + (double)p1[2][i]) * third;
        O2[i] = (float)(((double)p2[0][i] + (double)p2[1][i]) + (double)p2[2][i]) * third;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) { r1[k][i] = p1[k][i] - O1[i]; r2[k][i] = p2[k][i] - O2[i]; }
    // Step 2 (:246): M = Pr2 * Pr1.t(), a float matrix
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (float)dot3(r2[0][i], r2[1][i], r2[2][i], r1[0][j], r1[1][j], r1[2][j]);
    // Step 3 (:250-268): the sums are float expressions, and N is a float matrix
    const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
    const float N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
    const float N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}}, V[4][4];
    // Step 4 (:273-287): the vector of the largest eigenvalue (the first such), narrowed to float like evec
    jacobi_eigen4(A, V);
    int best = 0;
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const double dj = A[j][j], db = best == 0 ? A[0][0] : (best == 1 ? A[1][1] : A[2][2]);
        if (dj > db) best = j;
    }
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; k++) e[k] = (float)(best == 0 ? V[k][0] : (best == 1 ? V[k][1] : (best == 2 ? V[k][2] : V[k][3])));
    const double nrm = sqrt(dot3(e[1], e[2], e[3], e[1], e[2], e[3]));
    const double ang = atan2(nrm, (double)e[0]);
    const double alpha = 2.0 * ang / nrm;                              // vec = 2 * ang * vec / norm(vec): 0 / 0 for a vanishing vec
    const float rv[3] = {(float)((double)e[1] * alpha), (float)((double)e[2] * alpha), (float)((double)e[3] * alpha)};
    // cv::Rodrigues, vector to matrix: R = cos I + (1 - cos) r r^T + sin [r]x in double, narrowed once
    {
        double r[3] = {(double)rv[0], (double)rv[1], (double)rv[2]};
        const double theta = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        if (theta < kEps) {
#pragma unroll
            for (int i = 0; i < 9; i++) S.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        } else {
            const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
            r[0] = r[0] * it; r[1] = r[1] * it; r[2] = r[2] * it;
            const double K[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) S.R[3 * i + j] = (float)((c * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j])) + s * K[3 * i + j]);
        }
    }
    // Step 5 (:291): P3 = mR12i * Pr2
    float P3[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) P3[k][i] = (float)dot3(S.R[3 * i], S.R[3 * i + 1], S.R[3 * i + 2], r2[k][0], r2[k][1], r2[k][2]);
    // Step 6 (:295-314): nom = Pr1.dot(P3) and den = the sum of the float squares, both in double over the elements in row-major order
    if (!fixScale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                nom = nom + (double)r1[k][i] * (double)P3[k][i];
                den = den + (double)(P3[k][i] * P3[k][i]);
            }
        S.s = (float)(nom / den);
    } else
        S.s = 1.0f;
    // Step 7 (:319): mt12i = O1 - ms12i * mR12i * O2, one product with alpha = -ms12i and beta = 1
#pragma unroll
    for (int i = 0; i < 3; i++) S.t[i] = (float)((double)O1[i] - (double)S.s * dot3(S.R[3 * i], S.R[3 * i + 1], S.R[3 * i + 2], O2[0], O2[1], O2[2]));
    return S;
}

// Step 8 (:324-339): mT12i = [ms12i * mR12i | mt12i], mT21i = [sRinv | -sRinv * mt12i] with sRinv = (1.0 / ms12i) * mR12i.t()
DEVINL Sim3T transforms_of(const Sim3& S)
{
    Sim3T T;
    const float si = (float)(1.0 / (double)S.s);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) { T.A12[3 * i + j] = S.s * S.R[3 * i + j]; T.A21[3 * i + j] = S.R[3 * j + i] * si; }
        T.b12[i] = S.t[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) T.b21[i] = (float)(-dot3(T.A21[3 * i], T.A21[3 * i + 1], T.A21[3 * i + 2], S.t[0], S.t[1], S.t[2]));
    return T;
}

// CheckInliers (:343-367) of one correspondence: Project (:385-406) both ways, err = dist.dot(dist) in double narrowed to float
DEVINL bool is_inlier(const Sim3Params& P, const Sim3T& T, const Corr3& c)
{
    float q[3], u, v;
    mul_add(T.A12, c.X2, T.b12, q);                                    // vP2im1
    to_image(P, q, u, v);
    const float dx1 = c.u1 - u, dy1 = c.v1 - v;
    mul_add(T.A21, c.X1, T.b21, q);                                    // vP1im2
    to_image(P, q, u, v);
    const float dx2 = u - c.u2, dy2 = v - c.v2;
    const float err1 = (float)((double)dx1 * (double)dx1 + (double)dy1 * (double)dy1);
    const float err2 = (float)((double)dx2 * (double)dx2 + (double)dy2 * (double)dy2);
    return err1 < c.e1 && err2 < c.e2;
}

DEVINL void store_sim3(float* out, const Sim3& S)
{
#pragma unroll
    for (int i = 0; i < 9; i++) out[i] = S.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) out[9 + i] = S.t[i];
    out[12] = S.s; out[13] = 0.0f; out[14] = 0.0f; out[15] = 0.0f;
}
DEVINL Sim3 load_sim3(const float* in)
{
    Sim3 S;
#pragma unroll
    for (int i = 0; i < 9; i++) S.R[i] = in[i];
#pragma unroll
    for (int i = 0; i < 3; i++) S.t[i] = in[9 + i];
    S.s = in[12];
    return S;
}

// ---- the correspondences and the RANSAC parameters of every pair -----------------------------------------------------------------------
// head[p] = {N, mRansacMaxIts (0: the pair is answered here), mnIterations on entry, mnBestInliers on entry}
__global__ __launch_bounds__(256) void k_sim3_prepare(Sim3Params P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                      const int* __restrict__ select, const float* __restrict__ poses, const float* __restrict__ kfXw,
                                                      const uint8_t* __restrict__ flags, const int* __restrict__ match12, const int* __restrict__ state,
                                                      Corr3* __restrict__ corrAll, unsigned short* __restrict__ idxAll, int4* __restrict__ head,
                                                      uint8_t* __restrict__ inlierOut, int* __restrict__ nInliers, int* __restrict__ iterations)
{
    __shared__ int s_wcnt[4];
    const int p = blockIdx.x, tid = threadIdx.x, nf = P.nf;
    const int2 pr = pairs[p];
    const bool off = select && select[p] == 0;
    if (off || !rec_ok(P.nRecords, pr.x) || !rec_ok(P.nRecords, pr.y)) {   // nothing else of this pair is touched
        if (tid == 0) { nInliers[p] = off ? -2 : -1; head[p] = make_int4(0, 0, 0, 0); }
        return;
    }
    uint8_t* inl = inlierOut + (size_t)p * nf;
    for (int i = tid; i < nf; i += 256) inl[i] = 0;                    // vbInliers = vector<bool>(mN1, false) (:146)
    const uint8_t* rec1 = records + (size_t)pr.x * P.recBytes;
    const uint8_t* rec2 = records + (size_t)pr.y * P.recBytes;
    const ivf_keypoint* kps1 = rec_kps(rec1);
    const ivf_keypoint* kps2 = rec_kps(rec2);
    const int n1 = rec_count(rec1, nf), n2 = rec_count(rec2, nf);
    const float* xw1 = kfXw + (size_t)pr.x * nf * 3;
    const float* xw2 = kfXw + (size_t)pr.y * nf * 3;
    const uint8_t* f1 = flags + (size_t)pr.x * nf;
    const uint8_t* f2 = flags + (size_t)pr.y * nf;
    const int* m12 = match12 + (size_t)p * nf;
    float R1[9], t1[3], R2[9], t2[3];
    load_pose(poses + (size_t)pr.x * 12, R1, t1);
    load_pose(poses + (size_t)pr.y * 12, R2, t2);
    Corr3* corr = corrAll + (size_t)p * nf;
    unsigned short* idx = idxAll + (size_t)p * nf;
    const int N = compact_ordered<256>(n1, s_wcnt, tid,
        [&](int i1) { const int i2 = m12[i1]; return i2 >= 0 && i2 < n2 && (f1[i1] & 1) != 0 && (f2[i2] & 1) != 0; },
        [&](int i1, int slot) {
            const int i2 = m12[i1];
            Corr3 c;
            mul_add(R1, xw1 + 3 * i1, t1, c.X1);                       // mvX3Dc1 = Rcw1 * X3D1w + tcw1 (:97-101)
            mul_add(R2, xw2 + 3 * i2, t2, c.X2);
            // mvnMaxError is a vector<size_t>: 9.210 * sigmaSquare in double, truncated (:90-91); compared as float (:359)
            c.e1 = (float)(unsigned long long)(9.210 * (double)P.sigma2[clamp_octave(kps1[i1].octave)]);
            c.e2 = (float)(unsigned long long)(9.210 * (double)P.sigma2[clamp_octave(kps2[i2].octave)]);
            to_image(P, c.X1, c.u1, c.v1);                             // mvP1im1, mvP2im2 (:111-112)
            to_image(P, c.X2, c.u2, c.v2);
            corr[slot] = c;
            idx[slot] = (unsigned short)i1;                            // mvnIndices1
        });
    if (tid == 0) {
        const int it0 = state ? state[2 * p] : 0, best0 = state ? state[2 * p + 1] : 0;
        int its = 0;
        if (N >= P.minInliers && N >= 3)                               // else :149-153 (below three points the reference has no sample to draw)
            its = ransac_iterations(P.probability, (float)P.minInliers / (float)N, P.minInliers == N, P.maxIterations);   // :128-138
        head[p] = make_int4(N, its, it0 < 0 ? 0 : it0, best0);
        if (its == 0) { nInliers[p] = 0; if (iterations) iterations[p] = it0; }   // mnIterations is not advanced, the state stays
    }
}

// ---- one hypothesis --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sim3_hyp(Sim3Params P, const Corr3* __restrict__ corrAll, const int4* __restrict__ head,
                                                 const uint32_t* __restrict__ draws, float* __restrict__ hyp, int* __restrict__ hypN,
                                                 float* __restrict__ outSim3, int* __restrict__ outN)
{
    const int it = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const int4 h = head[p];
    if (it < h.z || it >= h.y) return;
    const int N = h.x;
    const Corr3* corr = corrAll + (size_t)p * P.nf;
    const size_t slot = (size_t)p * P.maxIterations + it;
    int smp[3];
    ransac_sample<3>(draws + slot * 3, N, smp);                        // :166-180, the same in every lane
    float p1[3][3], p2[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const Corr3 c = corr[smp[k]];
#pragma unroll
        for (int i = 0; i < 3; i++) { p1[k][i] = c.X1[i]; p2[k][i] = c.X2[i]; }
    }
    const Sim3 S = compute_sim3(p1, p2, P.fixScale != 0);
    const Sim3T T = transforms_of(S);
    int ni = 0;
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        ni += __popcll(__ballot(i < N && is_inlier(P, T, corr[i])));
    }
    if (lane == 0) {
        store_sim3(hyp + slot * 16, S);
        hypN[slot] = ni;
        if (outN) outN[slot] = ni;
        if (outSim3) store_sim3(outSim3 + slot * 16, S);
    }
}

// ---- the sequential bookkeeping of iterate() ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sim3_replay(Sim3Params P, const Corr3* __restrict__ corrAll, const unsigned short* __restrict__ idxAll,
                                                    const int4* __restrict__ head, const float* __restrict__ hyp, const int* __restrict__ hypN,
                                                    int* __restrict__ state, float* __restrict__ sim3, uint8_t* __restrict__ inlierOut,
                                                    int* __restrict__ nInliers, int* __restrict__ iterations)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const int4 h = head[p];
    const int N = h.x, maxIts = h.y, it0 = h.z;
    if (maxIts < 1) return;                                            // k_sim3_prepare has answered
    int best = h.w, done = it0, won = -1;
#pragma unroll 1
    for (int it = 0; it < kRansacMaxIterations; it++) {                  // while (mnIterations < mRansacMaxIts ...) (:161)
        if (it < it0) continue;
        if (it >= maxIts) break;
        done = it + 1;
        const int ni = hypN[(size_t)p * P.maxIterations + it];
        if (ni >= best) {                                              // :186
            best = ni;
            if (ni > P.minInliers) { won = it; break; }                // :195, strict
        }
    }
    if (lane == 0) {
        if (iterations) iterations[p] = done;
        if (state) { state[2 * p] = done; state[2 * p + 1] = best; }
        nInliers[p] = won < 0 ? 0 : hypN[(size_t)p * P.maxIterations + won];   // without a success: cv::Mat(), the best is not returned
    }
    if (won < 0) return;
    const float* hs = hyp + ((size_t)p * P.maxIterations + won) * 16;
    const Sim3 S = load_sim3(hs);
    const Sim3T T = transforms_of(S);
    const Corr3* corr = corrAll + (size_t)p * P.nf;
    const unsigned short* idx = idxAll + (size_t)p * P.nf;
    uint8_t* inl = inlierOut + (size_t)p * P.nf;
    for (int i = lane; i < N; i += 64)
        if (is_inlier(P, T, corr[i])) inl[idx[i]] = 1;                 // vbInliers[mvnIndices1[i]] = true (:198-200)
    if (lane < 16) sim3[(size_t)p * 16 + lane] = hs[lane];
}

}  // namespace

extern "C" {

int ivf_tracker_solve_sim3(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                           const int32_t* d_select, const float* d_poses, const float* d_kf_xw, const uint8_t* d_point_flags,
                           const int32_t* d_match12, const uint32_t* d_draws, int max_iterations, double probability, int min_inliers,
                           int fix_scale, int32_t* d_state, float* d_sim3, uint8_t* d_inlier, int32_t* d_ninliers, int32_t* d_iterations,
                           float* d_hyp_sim3, int32_t* d_hyp_ninliers, void* hip_stream)
{
    if (!t || !d_records || !d_pairs || !d_poses || !d_kf_xw || !d_point_flags || !d_match12 || !d_draws || !d_sim3 || !d_inlier || !d_ninliers)
        return fail(IVF_E_INVALID, "null argument");
    const int ra = ransac_args_ok(d_records, max_iterations, probability, min_inliers);
    if (ra != IVF_OK) return ra;
    if (n_pairs == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_pairs, st);
    if (rc != IVF_OK) return rc;
    if (!t->sim3.corr) {                                               // first use: the scratch of ONE call, sized by max_pairs
        const size_t np = (size_t)t->cfg.max_pairs, nf = (size_t)t->P.nf;
        if (!t->replace({{t->sim3.corr, np * nf * sizeof(Corr3)}, {t->sim3.idx, np * nf * sizeof(unsigned short)}, {t->sim3.head, np * sizeof(int4)},
                         {t->sim3.hyp, np * kRansacMaxIterations * 16 * sizeof(float)}, {t->sim3.hypN, np * kRansacMaxIterations * sizeof(int)}}))
            return fail(IVF_E_NO_DEVICE, "device allocation failed for the Sim3 scratch of %d pairs x %d features", t->cfg.max_pairs, t->P.nf);
    }
    Sim3Params P;
    P.nf = t->P.nf; P.nRecords = n_records; P.recBytes = t->P.recBytes;
    P.fx = t->P.fx; P.fy = t->P.fy; P.cx = t->P.cx; P.cy = t->P.cy;
    level_sigma2(t->P, P.sigma2);
    P.maxIterations = max_iterations; P.minInliers = min_inliers; P.fixScale = fix_scale != 0; P.probability = probability;
    Corr3* corr = (Corr3*)t->sim3.corr;
    int4* head = (int4*)t->sim3.head;
    hipLaunchKernelGGL(k_sim3_prepare, dim3(n_pairs), dim3(256), 0, st, P, d_records, (const int2*)d_pairs, d_select, d_poses, d_kf_xw, d_point_flags,
                       d_match12, (const int*)d_state, corr, t->sim3.idx, head, d_inlier, d_ninliers, d_iterations);
    hipLaunchKernelGGL(k_sim3_hyp, dim3(max_iterations, n_pairs), dim3(64), 0, st, P, (const Corr3*)corr, (const int4*)head, d_draws, t->sim3.hyp,
                       t->sim3.hypN, d_hyp_sim3, d_hyp_ninliers);
    hipLaunchKernelGGL(k_sim3_replay, dim3(n_pairs), dim3(64), 0, st, P, (const Corr3*)corr, (const unsigned short*)t->sim3.idx, (const int4*)head,
                       (const float*)t->sim3.hyp, (const int*)t->sim3.hypN, d_state, d_sim3, d_inlier, d_ninliers, d_iterations);
    return tracker_end(t, st);
}

}  // extern "C"
