// ivf_track_sim3.hip -- ivf_tracker_search_by_sim3: ORBmatcher::SearchBySim3 (ORB/src/ORBmatcher.cc:1145-1369) as LoopClosing::ComputeSim3
// runs it behind a successful Sim3Solver (ORB/src/LoopClosing.cc:318-328), for many (current keyframe, candidate) pairs of gather records at
// once, on the batched tracker handle (ivf_tracker.h): the inlier filter of LoopClosing.cc:318-323, vbAlreadyMatched1 / 2 (:1175-1185), BOTH
// projection loops (:1191-1268, :1271-1348) and the agreement check (:1350-1366).  Nothing crosses PCIe and nothing is replayed on the host;
// nothing in this search is greedy, so there are no candidate lists: every query keeps the first minimum of its window.
//
// Arithmetic: matrix * vector accumulates in double and narrows once, R * x + t is mul_add (ivf_device.h);
// sR12[k] = (float)((double)s12 * R12[k]), sR21[k] = (float)((1.0 / (double)s12) * R12^T[k]), t21 = -(sR21 * t12) accumulated in double;
// invz = 1.0 / z in double, narrowed once; u = fx * (x * invz) + cx in float, unfused, with the HANDLE's intrinsics in both directions (the
// reference uses KF1's for both); dist3D = the camera-frame norm of the transformed point, accumulated in double, sqrt, narrowed.
//
// Kernels (gfx950, wave = 64; every loop is bounded by nfeatures or by the grid, so a NaN pose or a NaN similarity cannot hang a launch):
//   k_sim3_prepare  one workgroup per slot s = 2 * pair + side (side 0: KF1's points into KF2, side 1: KF2's into KF1): the grid of the
//                   target record (ivf_grid.h), the already-matched set of the source side in LDS, then one thread per source keypoint:
//                   projection -> query + radius
//   k_sim3_window   one wave per (slot, source keypoint): first_min_in_window (ivf_search.h) with an always-true admission on octaves
//                   [level - 1, level], accepted at <= TH_HIGH -> vnMatch1 / vnMatch2
//   k_sim3_agree    one workgroup per pair: the agreement check and the outputs
// The scratch is the handle's: two grids per pair (tracker_grow_grids) and this call's own queries, radii and vnMatch (Sim3SearchScratch,
// ivf_tracker.h), both made at the first call, which therefore waits on the host for the handle's previous call; later calls do not.
#include "ivf_search.h"

using namespace ivf;

namespace {

static_assert(sizeof(ivf_local_point) == 80, "ivf_local_point is read as five 16-byte pieces");
constexpr int kThHigh = 100;                      // ORBmatcher::TH_HIGH

// KeyFrame::IsInImage (KeyFrame.cc:647-650): >= min and < max, strictly -- not Frame's inclusive test (in_image, ivf_search.h)
DEVINL bool keyframe_is_in_image(const TrackParams& P, float u, float v) { return u >= P.minX && u < P.maxX && v >= P.minY && v < P.maxY; }

// vpMatches12[i1] on entry: the match where the solver's inlier flag keeps it (LoopClosing.cc:318-323), else none
DEVINL int match_in(const int* __restrict__ m12, const uint8_t* __restrict__ inl, int i1)
{
    const int m = m12[i1];
    return (m >= 0 && (!inl || inl[i1] != 0)) ? m : -1;
}

__global__ __launch_bounds__(256) void k_sim3_prepare(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                     const int* __restrict__ select, const float* __restrict__ poses,
                                                     const ivf_local_point* __restrict__ kfPoints, const float* __restrict__ sim3,
                                                     const int* __restrict__ match12, const uint8_t* __restrict__ inlier, float th,
                                                     int* __restrict__ gStart, unsigned short* __restrict__ gIdx, Query* __restrict__ queries,
                                                     float* __restrict__ radii)
{
    __shared__ int cnt[kGC * kGR];
    __shared__ int part[256];
    __shared__ int blk[256];
    __shared__ uint8_t s_am[kMaxTrackFeatures];               // vbAlreadyMatched of the source side
    const int s = blockIdx.x, p = s >> 1, side = s & 1, tid = threadIdx.x;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p)) return;
    const int rSrc = side ? pr.y : pr.x, rTgt = side ? pr.x : pr.y;
    const uint8_t* rec1 = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recS = records + (size_t)rSrc * P.recBytes;
    const uint8_t* recT = records + (size_t)rTgt * P.recBytes;
    const int n1 = rec_count(rec1, P.nf), nS = rec_count(recS, P.nf), nT = rec_count(recT, P.nf);
    grid_build(geom_of(P), rec_kps(recT), nT, gStart + (size_t)s * (kGC * kGR + 1), gIdx + (size_t)s * P.nf, cnt, part, blk, tid);

    // :1175-1185: GetIndexInKeyFrame(pKF2) is the keypoint index itself; one outside KF2's count marks nothing there
    const int* m12 = match12 + (size_t)p * P.nf;
    const uint8_t* inl = inlier ? inlier + (size_t)p * P.nf : nullptr;
    for (int i = tid; i < P.nf; i += 256) s_am[i] = 0;
    __syncthreads();
    for (int i1 = tid; i1 < n1; i1 += 256) {
        const int m = match_in(m12, inl, i1);
        if (m < 0) continue;
        if (!side) s_am[i1] = 1;
        else if (m < nS) s_am[m] = 1;                         // side 1: the source is KF2, nS = N2
    }
    __syncthreads();

    float Rs[9], ts[3], sR[9], tt[3];
    load_pose(poses + (size_t)rSrc * 12, Rs, ts);
    {
        const float* S = sim3 + (size_t)p * 16;               // R12 (9), t12 (3), s12
        const float s12 = S[12];
        if (side) {                                           // sR12, t12 (:1160)
#pragma unroll
            for (int k = 0; k < 9; k++) sR[k] = (float)((double)s12 * (double)S[k]);
#pragma unroll
            for (int k = 0; k < 3; k++) tt[k] = S[9 + k];
        } else {                                              // sR21 = (1.0 / s12) * R12.t(), t21 = -sR21 * t12 (:1161-1162)
            const double inv = 1.0 / (double)s12;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) sR[3 * i + j] = (float)(inv * (double)S[3 * j + i]);
#pragma unroll
            for (int i = 0; i < 3; i++)
                tt[i] = (float)(-((double)sR[3 * i] * (double)S[9] + (double)sR[3 * i + 1] * (double)S[10] + (double)sR[3 * i + 2] * (double)S[11]));
        }
    }
    const ivf_local_point* pts = kfPoints + (size_t)rSrc * P.nf;
    Query* Q = queries + (size_t)s * P.nf;
    float* Rd = radii + (size_t)s * P.nf;
    for (int i = tid; i < P.nf; i += 256) {
        Query q; q.u = 0; q.v = 0; q.ur = 0; q.bits = 0;
        float radius = 0.0f;
        const ivf_local_point mp = pts[i];
        if (i < nS && !(mp.flags & 1) && !s_am[i]) {                                  // :1195-1203
            float xs[3], xc[3];
            mul_add(Rs, mp.pos, ts, xs);                                              // p3Dc1 = R1w * p3Dw + t1w (:1205-1206)
            mul_add(sR, xs, tt, xc);                                                  // p3Dc2 = sR21 * p3Dc1 + t21 (:1207)
            if (!(xc[2] < 0.0f)) {                                                    // :1210: a zero depth goes on, its projection fails below
                const float invz = (float)(1.0 / (double)xc[2]);                      // :1213
                const float x = xc[0] * invz, y = xc[1] * invz;                       // :1214-1215: the quotient first,
                const float u = P.fx * x + P.cx, v = P.fy * y + P.cy;                 // then u = fx * x + cx (:1217-1218)
                if (keyframe_is_in_image(P, u, v)) {                                  // :1221
                    const double n2 = (double)xc[0] * (double)xc[0] + (double)xc[1] * (double)xc[1] + (double)xc[2] * (double)xc[2];
                    const float dist3D = (float)sqrt(n2);                             // cv::norm(p3Dc2) (:1226)
                    int lv;
                    if (range_level(P, mp, dist3D, lv)) {                             // :1229-1233
                        radius = th * P.scale[lv];                                    // :1236
                        q.u = u; q.v = v;
                        q.bits = (unsigned)lv | (1u << 24);
                    }
                }
            }
        }
        Q[i] = q; Rd[i] = radius;
    }
}

// one wave per (slot, source keypoint): :1238-1267 / :1318-1347
__global__ __launch_bounds__(256) void k_sim3_window(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                    const int* __restrict__ select, const ivf_local_point* __restrict__ kfPoints,
                                                    const int* __restrict__ gStart, const unsigned short* __restrict__ gIdx,
                                                    const Query* __restrict__ queries, const float* __restrict__ radii, int* __restrict__ vnMatch)
{
    const int s = blockIdx.y, p = s >> 1, side = s & 1;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p) || i >= P.nf) return;
    const int rSrc = side ? pr.y : pr.x, rTgt = side ? pr.x : pr.y;
    const uint8_t* recT = records + (size_t)rTgt * P.recBytes;
    const Query q = queries[(size_t)s * P.nf + i];
    int bestDist = 256, bestIdx = -1;
    if ((q.bits >> 24) & 1) {
        const int lv = q.bits & 0xff;
        const uint4* qd = (const uint4*)kfPoints[(size_t)rSrc * P.nf + i].desc;       // pMP->GetDescriptor() (:1245)
        first_min_in_window(geom_of(P), rec_kps(recT), rec_desc(recT, P.nf), gStart + (size_t)s * (kGC * kGR + 1), gIdx + (size_t)s * P.nf,
                            q.u, q.v, radii[(size_t)s * P.nf + i], lv - 1, lv, qd[0], qd[1], lane, [](int) { return true; }, bestDist, bestIdx);
    }
    if (lane == 0) vnMatch[(size_t)s * P.nf + i] = (bestIdx >= 0 && bestDist <= kThHigh) ? bestIdx : -1;   // :1264
}

// one workgroup per pair: :1350-1366
__global__ __launch_bounds__(256) void k_sim3_agree(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                   const int* __restrict__ select, const int* __restrict__ match12,
                                                   const uint8_t* __restrict__ inlier, const int* __restrict__ vnMatch,
                                                   int* __restrict__ matches, int* __restrict__ nfound, int* __restrict__ match1Out,
                                                   int* __restrict__ match2Out)
{
    __shared__ int s_found;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p)) {
        if (tid == 0) nfound[p] = (select && select[p] == 0) ? -2 : -1;
        return;
    }
    const int n1 = rec_count(records + (size_t)pr.x * P.recBytes, P.nf);
    const int* vn1 = vnMatch + (size_t)(2 * p) * P.nf;
    const int* vn2 = vn1 + P.nf;
    const int* m12 = match12 + (size_t)p * P.nf;
    const uint8_t* inl = inlier ? inlier + (size_t)p * P.nf : nullptr;
    if (tid == 0) s_found = 0;
    __syncthreads();
    int found = 0;
    for (int i1 = tid; i1 < P.nf; i1 += 256) {
        int out = i1 < n1 ? match_in(m12, inl, i1) : -1;
        const int idx2 = vn1[i1];
        if (idx2 >= 0 && vn2[idx2] == i1) { out = idx2; found++; }                    // :1357-1364
        matches[(size_t)p * P.nf + i1] = out;
        if (match1Out) match1Out[(size_t)p * P.nf + i1] = idx2;
        if (match2Out) match2Out[(size_t)p * P.nf + i1] = vn2[i1];
    }
    if (found) atomicAdd(&s_found, found);
    __syncthreads();
    if (tid == 0) nfound[p] = s_found;
}

}  // namespace

extern "C" {

int ivf_tracker_search_by_sim3(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                               const int32_t* d_select, const float* d_poses, const ivf_local_point* d_kf_points, const float* d_sim3,
                               const int32_t* d_match12, const uint8_t* d_inlier, float th, int32_t* d_matches, int32_t* d_nfound,
                               int32_t* d_match1, int32_t* d_match2, void* hip_stream)
{
    const int ra = search_args_ok(t, d_records, d_pairs, true, d_kf_points, d_matches, d_nfound, n_pairs, nullptr, nullptr);
    if (ra != IVF_OK) return ra;
    if (!d_poses || !d_sim3 || !d_match12) return fail(IVF_E_INVALID, "null argument");
    if (d_matches == d_match12) return fail(IVF_E_INVALID, "d_matches may not alias d_match12");
    if (!(th > 0)) return fail(IVF_E_INVALID, "th must be positive");
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_pairs, st);
    if (rc != IVF_OK) return rc;
    if (n_pairs == 0) return IVF_OK;
    const int rg = tracker_grow_grids(t, 2);
    if (rg != IVF_OK) return rg;
    Sim3SearchScratch& W = t->sim3s;
    const size_t nq = 2 * (size_t)t->cfg.max_pairs * (size_t)t->P.nf;
    if (!W.q && !t->replace({{W.q, nq * sizeof(Query)}, {W.rad, nq * sizeof(float)}, {W.vn, nq * sizeof(int)}}))
        return fail(IVF_E_NO_DEVICE, "device allocation failed for the queries of %d pairs", t->cfg.max_pairs);
    TrackParams P = t->P;
    P.nRecords = n_records;
    const int2* pairs = (const int2*)d_pairs;
    hipLaunchKernelGGL(k_sim3_prepare, dim3(2 * n_pairs), dim3(256), 0, st, P, d_records, pairs, d_select, d_poses, d_kf_points, d_sim3, d_match12,
                       d_inlier, th, t->dStart, t->dIdx, W.q, W.rad);
    hipLaunchKernelGGL(k_sim3_window, dim3((P.nf + 3) / 4, 2 * n_pairs), dim3(256), 0, st, P, d_records, pairs, d_select, d_kf_points, t->dStart,
                       t->dIdx, W.q, W.rad, W.vn);
    hipLaunchKernelGGL(k_sim3_agree, dim3(n_pairs), dim3(256), 0, st, P, d_records, pairs, d_select, d_match12, d_inlier, W.vn, d_matches,
                       d_nfound, d_match1, d_match2);
    return tracker_end(t, st);
}

}  // extern "C"
