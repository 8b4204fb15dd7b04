// ivf_solve.h -- what the two solvers of the batched tracker share, ivf_pose.hip (PoseOptimization) and ivf_pnp.hip (PnPsolver), and
// the searches do not need: the fixed-tree sums, the ordered compaction, a frame's pointer set, the octave clamp, the pose I/O, the
// Jacobi rotation and the level sigma2 table.  ivf_track_create.hip (CreateNewMapPoints) takes the compaction, the clamp, the rotation
// and the table; ivf_sim3.hip (Sim3Solver) the compaction, the clamp, the sweep cap and the table.  ivf_pnp.hip and ivf_sim3.hip share the
// RANSAC sampler and iteration count below; their cap, argument checks and scratch allocation (alloc_all) are ivf_tracker.h's.
#pragma once
#include "ivf_tracker.h"

namespace ivf {

// ---- sums with a fixed tree: two runs are bit-identical
DEVINL double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);        // a + b == b + a: every lane ends with the same bits
    return v;
}
// the per-wave partials part[0], part[stride], ... of NW waves, summed in wave order: ((p0 + p1) + p2) + p3
template <int NW>
DEVINL double wave_order_sum(const double* part, int stride)
{
    double v = part[0];
#pragma unroll
    for (int w = 1; w < NW; w++) v = v + part[w * stride];
    return v;
}

// ---- the workgroup-wide compaction of the items i < n with keep(i), in item order; called by all NT threads, s_wcnt [NT / 64] in LDS.
// Item i gets slot = the number of kept items before it and runs store(i, slot) between the two barriers of its chunk of NT items:
// what store() wrote to LDS is visible to the workgroup at the return.  Returns the number kept (the same in every thread).
template <int NT, class Keep, class Store>
DEVINL int compact_ordered(int n, int* s_wcnt, int tid, Keep keep, Store store)
{
    const int wave = tid >> 6, lane = tid & 63;
    int total = 0;
    for (int i0 = 0; i0 < n; i0 += NT) {
        const int i = i0 + tid;
        const bool on = i < n && keep(i);
        const unsigned long long m = __ballot(on);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int base = total;
#pragma unroll
        for (int w = 0; w < NT / 64; w++) { const int c = s_wcnt[w]; if (w < wave) base += c; total += c; }
        if (on) store(i, base + __popcll(m & ((1ull << lane) - 1ull)));
        __syncthreads();
    }
    return total;
}

// ---- what a solver reads of frame f: the keypoints of record ri, the points and flags the caller assigned to them.  nC < 0: ri is
// outside the block of this call, and the kernel refuses the frame in its own way
struct FrameObs { const ivf_keypoint* kps; const float* uRight; const float* X; const uint8_t* has; int nC; };
DEVINL FrameObs frame_obs(const uint8_t* records, size_t recBytes, int nf, int nRecords, int ri, const float* xw, const uint8_t* hasPoint, int f)
{
    if (!rec_ok(nRecords, ri)) return FrameObs{nullptr, nullptr, nullptr, nullptr, -1};
    const uint8_t* rec = records + (size_t)ri * recBytes;
    return FrameObs{rec_kps(rec), rec_uright(rec, nf), xw + (size_t)f * nf * 3, hasPoint + (size_t)f * nf, rec_count(rec, nf)};
}

// a keypoint's octave as an index of the level tables
DEVINL int clamp_octave(int o) { return o < 0 ? 0 : (o > kMaxLevels - 1 ? kMaxLevels - 1 : o); }

// ---- a row-major 3x4 pose [R | t] from / to double R[9], t[3]: the float result, or an f64 hypothesis slot of PnpScratch
template <class T>
DEVINL void store_pose(T* out, const double* R, const double* t)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[4 * i + j] = (T)R[3 * i + j];
        out[4 * i + 3] = (T)t[i];
    }
}
DEVINL void load_hyp(const double* hp, double* R, double* t)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = hp[4 * i + j];
        t[i] = hp[4 * i + 3];
    }
}

// ---- the cyclic one-sided Jacobi SVD both of its forms share: ivf_pnp.hip's (the matrix in LDS, a rotation spread over lanes) and
// ivf_track_create.hip's (a 4x4 per lane in registers).  The pairs (p, q), p < q, are visited in ascending order, at most kSweeps
// sweeps; a sweep that turns nothing ends the iteration.
constexpr int kSweeps = 30;                                           // cap of the Jacobi sweeps (convergence takes 6..10)
constexpr double kEps = 0x1p-52;                                      // DBL_EPSILON
// the rotation that makes columns p and q orthogonal, from a = |p|^2, b = |q|^2, g = p.q: false when they are already (or on a NaN)
DEVINL bool jacobi_rotation(double a, double b, double g, double& c, double& s)
{
    if (!(fabs(g) > kEps * sqrt(a * b))) return false;
    const double zeta = (b - a) / (2.0 * g);
    const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    c = 1.0 / sqrt(1.0 + tn * tn); s = c * tn;
    return true;
}

// ---- RANSAC, ivf_pnp.hip (K = 4) and ivf_sim3.hip (K = 3): the K sample indices of one iteration from its rand() values dr[K], N >= K
// (PnPsolver.cc:192-205, Sim3Solver.cc:166-180).  vAvailableIndices = mvAllIndices, then K times DUtils::Random::RandomInt(0, size - 1) and
// the swap with the back; the vector is the identity but for the at most K - 1 positions a removal rewrote (pos[] / val[]), in registers
template <int K>
DEVINL void ransac_sample(const uint32_t* dr, int N, int* smp)
{
    int size = N, pos[K], val[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t r = dr[k] & 0x7fffffffu;                       // a value rand() can return
        const int randi = (int)(((double)r / 2147483648.0) * size);
        int idx = randi, back = size - 1;
#pragma unroll
        for (int j = 0; j < k; j++) { if (pos[j] == randi) idx = val[j]; if (pos[j] == size - 1) back = val[j]; }
        smp[k] = idx;
        pos[k] = randi; val[k] = back; size--;
    }
}
// mRansacMaxIts, the tail of SetRansacParameters (PnPsolver.cc:148-156, Sim3Solver.cc:130-138): one iteration when nMin == N, else
// ceil(log(1 - p) / log(1 - eps^3)), not above the caller's maxIterations (a NaN or an infinity ends there too) and not below 1
DEVINL int ransac_iterations(double probability, float eps, bool allInliers, int maxIterations)
{
    int its = 1;
    if (!allInliers) {
        const double x = ceil(log(1 - probability) / log(1 - pow((double)eps, 3.0)));
        its = !(x < (double)maxIterations) ? maxIterations : (x < 1.0 ? 1 : (int)x);
    }
    if (its > maxIterations) its = maxIterations;
    return its < 1 ? 1 : its;
}

// mvLevelSigma2 (ORBextractor.cc:419-431) of the handle's scale factors; mvInvLevelSigma2 is 1.0f / s2[l]
inline void level_sigma2(const TrackParams& T, float* s2)
{
    for (int l = 0; l < kMaxLevels; l++) s2[l] = T.scale[l] * T.scale[l];
}

}  // namespace ivf
