// ivf_track_reloc.hip -- ivf_tracker_search_reloc and ivf_tracker_filter_assign: what Tracking::Relocalization (ORB/src/Tracking.cc:2272-2421)
// does after its first pose, for many lost frames at once, on the batched tracker handle (ivf_tracker.h).
//   * ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORB/src/ORBmatcher.cc:1520-1652), the search of
//     Tracking.cc:2375 (th 10, ORBdist 100) and :2391 (3, 64): projection of the keyframe's map points under the frame's pose with NO test
//     on the sign of the depth, the distance-invariance range, MapPoint::PredictScale (ivf_tracker.h), windows on levels
//     [level - 1, level + 1], the FIRST minimum among the keypoints that hold no point, accepted at <= ORBdist, the rotation histogram
//     against the keyframe keypoint's angle, UpdateQualityScores(CurrentFrame);
//   * the set bookkeeping around it (Tracking.cc:2351-2370, :2386-2389, :2398-2400): keep PnP's inliers / drop the optimiser's outliers
//     in the assignment, and write sFound.
// Nothing crosses PCIe and nothing is replayed on the host.
//
// Kernels (all hand-written for gfx950; wave = 64; every loop is bounded by nfeatures or by the grid, so a NaN pose cannot hang a launch):
//   k_reloc_prepare  one workgroup per (keyframe, current) pair: the grid of the current record (ivf_grid.h, unsigned short indices), the
//                    found set in LDS, then one thread per keyframe keypoint: projection -> query + radius
//   k_reloc_window   one wave per (pair, keyframe keypoint): ordered candidate list, entry = index | distance << 16
//   k_reloc_greedy   one wave per pair: walks the keyframe keypoints in order against the occupancy state in LDS; the first minimum is a
//                    DPP minimum reduction of (distance << 6 | list position)
//   k_filter_assign  one workgroup per frame
// Pair liveness, the map-point gates, the ordered list, the first minimum (of a list and of an overflowed window) and the prefetched walk
// over the lists are ivf_search.h's; the candidate scratch is the handle's one set (ivf_track.hip: tracker_grow_queries).
#include "ivf_search.h"

using namespace ivf;

namespace {

static_assert(sizeof(ivf_local_point) == 80, "ivf_local_point is read as five 16-byte pieces");
constexpr int kRelocEntry = 1 << 24;              // s_assign: the keypoint held this point before the call (occupied, never changed)
constexpr int kRelocIdMask = 0xffff;              // s_assign: keyframe keypoint | rotation bin << 16 | kRelocEntry

// one workgroup per pair: grid of the current record, sAlreadyFound, then ORBmatcher.cc:1537-1575 of every keyframe keypoint
__global__ __launch_bounds__(256) void k_reloc_prepare(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                      const int* __restrict__ select, const float* __restrict__ poses,
                                                      const ivf_local_point* __restrict__ kfPoints, const uint8_t* __restrict__ found,
                                                      const int* __restrict__ assignIn, float th, int* __restrict__ gStart,
                                                      unsigned short* __restrict__ gIdx, Query* __restrict__ queries, float* __restrict__ radii)
{
    __shared__ int cnt[kGC * kGR];
    __shared__ int part[256];
    __shared__ int blk[256];
    __shared__ uint8_t s_found[kMaxTrackFeatures];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p)) return;
    const uint8_t* recK = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recC = records + (size_t)pr.y * P.recBytes;
    const int nK = rec_count(recK, P.nf), nC = rec_count(recC, P.nf);
    grid_build(geom_of(P), rec_kps(recC), nC, gStart + (size_t)p * (kGC * kGR + 1), gIdx + (size_t)p * P.nf, cnt, part, blk, tid);

    // sAlreadyFound by keyframe keypoint: the caller's, or the points the frame holds on entry (Tracking.cc:2386-2389)
    if (found) {
        for (int i = tid; i < P.nf; i += 256) s_found[i] = found[(size_t)p * P.nf + i];
    } else {
        for (int i = tid; i < P.nf; i += 256) s_found[i] = 0;
        __syncthreads();
        for (int i = tid; i < P.nf; i += 256) { const int a = assignIn[(size_t)p * P.nf + i]; if (a >= 0 && a < P.nf) s_found[a] = 1; }
    }
    __syncthreads();

    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, Ow[3];
    if (poses) load_pose(poses + (size_t)p * 12, R, t);
    neg_rt_mul(R, t, Ow);                                                             // :1527
    const ivf_local_point* pts = kfPoints + (size_t)pr.x * P.nf;
    Query* Q = queries + (size_t)p * P.nf;
    float* Rd = radii + (size_t)p * P.nf;
    for (int i = tid; i < nK; i += 256) {
        Query q; q.u = 0; q.v = 0; q.ur = 0; q.bits = 0;
        float radius = 0.0f;
        const ivf_local_point mp = pts[i];
        if (!(mp.flags & 1) && !s_found[i]) {                                         // :1541-1543
            float xc[3];
            mul_add(R, mp.pos, t, xc);                                                // :1547
            const float invzc = (float)(1.0 / (double)xc[2]);                         // :1551; no test on its sign
            const float u = P.fx * xc[0] * invzc + P.cx, v = P.fy * xc[1] * invzc + P.cy;
            float dist3D; int lv;
            if (in_image(P, u, v) && point_range_level(P, mp, Ow, dist3D, lv)) {      // :1556-1559, :1563-1572
                radius = th * P.scale[lv];                                            // :1575
                q.u = u; q.v = v;
                q.bits = (unsigned)lv | (1u << 24);
            }
        }
        Q[i] = q; Rd[i] = radius;
    }
}

// one wave per (pair, keyframe keypoint): the ordered candidate list of GetFeaturesInArea(u, v, radius, level - 1, level + 1) (:1577)
// with the distance of :1595 beside every index; the occupancy test of :1590 is the greedy walk's
__global__ __launch_bounds__(256) void k_reloc_window(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                     const int* __restrict__ select, const ivf_local_point* __restrict__ kfPoints,
                                                     const int* __restrict__ gStart, const unsigned short* __restrict__ gIdx,
                                                     const Query* __restrict__ queries, const float* __restrict__ radii,
                                                     int* __restrict__ count, unsigned* __restrict__ lists)
{
    const int p = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p)) return;
    const uint8_t* recK = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recC = records + (size_t)pr.y * P.recBytes;
    if (i >= rec_count(recK, P.nf)) return;
    const Query q = queries[(size_t)p * P.nf + i];
    int total = 0;
    if ((q.bits >> 24) & 1) {
        const int lv = q.bits & 0xff;
        const float r = radii[(size_t)p * P.nf + i];
        const uint4* qd = (const uint4*)kfPoints[(size_t)pr.x * P.nf + i].desc;       // pMP->GetDescriptor() (:1582)
        const uint4 qa = qd[0], qb = qd[1];
        unsigned* L = lists + ((size_t)p * P.nf + i) * kListCap;
        grid_walk(geom_of(P), rec_kps(recC), rec_desc(recC, P.nf), gStart + (size_t)p * (kGC * kGR + 1), gIdx + (size_t)p * P.nf,
                  q.u, q.v, r, lv - 1, lv + 1, qa, qb, lane, [&](bool ok, int i2, int d) { list_append(ok, lane, total, L, (unsigned)i2 | ((unsigned)d << 16)); });
    }
    if (lane == 0) count[(size_t)p * P.nf + i] = total;
}

// one wave per pair: the greedy walk of :1537-1620 over the keyframe's keypoints, the rotation filter (:1626-1645) and
// UpdateQualityScores(CurrentFrame) (:1647-1649).  The best of :1587-1602 is the first candidate of minimal distance among the
// keypoints that hold no point (`dist < bestDist` is strict): the minimum of (distance << 6 | list position).
__global__ __launch_bounds__(64) void k_reloc_greedy(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                    const int* __restrict__ select, const ivf_local_point* __restrict__ kfPoints,
                                                    const int* __restrict__ gStart, const unsigned short* __restrict__ gIdx,
                                                    const Query* __restrict__ queries, const float* __restrict__ radii, int orbDist,
                                                    int checkOri, const int* __restrict__ count, const unsigned* __restrict__ lists,
                                                    float* __restrict__ pointQuality, float* __restrict__ keyQuality,
                                                    int* __restrict__ assign, int* __restrict__ nmatchesOut)
{
    extern __shared__ int s_mem[];
    __shared__ int s_hist[32];                                // rotHist[b].size()
    const int p = blockIdx.x, lane = threadIdx.x;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p)) {
        if (lane == 0) nmatchesOut[p] = (select && select[p] == 0) ? -2 : -1;
        return;
    }
    int* s_assign = s_mem;                                    // [nf]: -1 free, -2 held on entry by something that is no keyframe keypoint,
                                                              // else keyframe keypoint | bin << 16 (| kRelocEntry: held on entry)
    const uint8_t* recK = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recC = records + (size_t)pr.y * P.recBytes;
    const int nK = rec_count(recK, P.nf), nC = rec_count(recC, P.nf);
    const ivf_keypoint* kK = rec_kps(recK);
    const ivf_keypoint* kc = rec_kps(recC);
    int* io = assign + (size_t)p * P.nf;
    for (int i = lane; i < nC; i += 64) { const int a = io[i]; s_assign[i] = a < 0 ? -1 : (a < P.nf ? (a | kRelocEntry) : -2); }   // :1590
    if (lane < 32) s_hist[lane] = 0;
    wave_sync_lds();
    const Query* Q = queries + (size_t)p * P.nf;
    const float* Rd = radii + (size_t)p * P.nf;
    const int* C = count + (size_t)p * P.nf;
    const unsigned* Lp = lists + (size_t)p * P.nf * kListCap;
    int nm = 0;

    auto free = [&](int i2) { return s_assign[i2] == -1; };                             // :1590
    // vIndices2.empty() (:1579) is the walk's cnt == 0
    walk_lists_prefetched(nK, C, Lp, lane, [&](int i) { return kK[i].angle; }, [&](int i, int cnt, unsigned e, auto angK) {
        int bestDist = 256, bestIdx2 = -1;
        if (cnt <= kListCap) {
            first_min_in_list(lane < cnt, (int)(e >> 16), (int)(e & 0xffff), lane, free, bestDist, bestIdx2);
        } else {
            // the window overflowed its list: walk it again against the live occupancy state, 64 candidates at a time
            const Query q = Q[i];
            const int lv = q.bits & 0xff;
            const uint4* qd = (const uint4*)kfPoints[(size_t)pr.x * P.nf + i].desc;
            first_min_in_window(geom_of(P), kc, rec_desc(recC, P.nf), gStart + (size_t)p * (kGC * kGR + 1), gIdx + (size_t)p * P.nf, q.u, q.v, Rd[i],
                                lv - 1, lv + 1, qd[0], qd[1], lane, free, bestDist, bestIdx2);
        }
        if (bestIdx2 < 0 || bestDist > orbDist) return;                                 // :1604
        const int bin = checkOri ? rot_bin(angK() - kc[bestIdx2].angle) : 0;              // :1611-1616
        if (lane == 0) { s_assign[bestIdx2] = i | (bin << 16); if (checkOri) s_hist[bin]++; }      // :1606, :1618
        nm++;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    });
    wave_sync_lds();
    // ComputeThreeMaxima (:1654-1695): the matches of every other bin are taken back; their keypoints were occupied while the walk ran
    if (checkOri) {
        const RotKeep keep = rot_three_maxima(s_hist);
        int removed = 0;
        for (int i0 = 0; i0 < nC; i0 += 64) {
            const int i = i0 + lane;
            bool rm = false;
            if (i < nC) {
                const int a = s_assign[i];
                rm = a >= 0 && !(a & kRelocEntry) && !keep.keeps((a >> 16) & 31);
                if (rm) s_assign[i] = -1;                                               // :1640
            }
            removed += __popcll(__ballot(rm));
        }
        nm -= removed;
        wave_sync_lds();
    }
    for (int i = lane; i < nC; i += 64) { const int a = s_assign[i]; if (a >= 0 && !(a & kRelocEntry)) io[i] = a & kRelocIdMask; }
    // UpdateQualityScores(CurrentFrame) (:1647-1649) over every keypoint that holds a keyframe point now
    if (pointQuality && keyQuality) update_quality_scores(s_assign, nC, kRelocIdMask, lane, 64, pointQuality + (size_t)p * P.nf, keyQuality + (size_t)p * P.nf);
    if (lane == 0) nmatchesOut[p] = nm;
}

// one workgroup per frame: Tracking.cc:2351-2361 (keep_when_set = 1 on PnP's inliers, found = sFound) and :2368-2370 / :2398-2400
// (keep_when_set = 0 on mvbOutlier)
__global__ __launch_bounds__(256) void k_filter_assign(int nf, int* __restrict__ assign, const uint8_t* __restrict__ mask, int keepWhenSet,
                                                      uint8_t* __restrict__ found)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    int* A = assign + (size_t)f * nf;
    if (found) {
        for (int i = tid; i < nf; i += 256) found[(size_t)f * nf + i] = 0;
        __syncthreads();
    }
    for (int i = tid; i < nf; i += 256) {
        int a = A[i];
        if (mask && ((mask[(size_t)f * nf + i] != 0) != (keepWhenSet != 0)) && a != -1) { a = -1; A[i] = -1; }
        if (found && a >= 0 && a < nf) found[(size_t)f * nf + a] = 1;
    }
}

}  // namespace

extern "C" {

int ivf_tracker_search_reloc(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                             const int32_t* d_select, const float* d_poses, const ivf_local_point* d_kf_points, const uint8_t* d_found, float th,
                             int orb_dist, int check_orientation, float* d_point_quality, float* d_key_quality, int32_t* d_assign,
                             int32_t* d_nmatches, void* hip_stream)
{
    const int ra = search_args_ok(t, d_records, d_pairs, true, d_kf_points, d_assign, d_nmatches, n_pairs, d_point_quality, d_key_quality);
    if (ra != IVF_OK) return ra;
    if (!(th > 0)) return fail(IVF_E_INVALID, "th must be positive");
    if (orb_dist < 0 || orb_dist > 255) return fail(IVF_E_INVALID, "orb_dist %d outside [0,255]", orb_dist);
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_pairs, st);
    if (rc != IVF_OK) return rc;
    if (n_pairs == 0) return IVF_OK;
    TrackParams P = t->P;
    P.nRecords = n_records;
    const int2* pairs = (const int2*)d_pairs;
    hipLaunchKernelGGL(k_reloc_prepare, dim3(n_pairs), dim3(256), 0, st, P, d_records, pairs, d_select, d_poses, d_kf_points, d_found, d_assign, th,
                       t->dStart, t->dIdx, t->dQ, t->dLRad);
    hipLaunchKernelGGL(k_reloc_window, dim3((P.nf + 3) / 4, n_pairs), dim3(256), 0, st, P, d_records, pairs, d_select, d_kf_points, t->dStart, t->dIdx,
                       t->dQ, t->dLRad, t->dCount, t->dLists);
    hipLaunchKernelGGL(k_reloc_greedy, dim3(n_pairs), dim3(64), (size_t)P.nf * sizeof(int), st, P, d_records, pairs, d_select, d_kf_points, t->dStart,
                       t->dIdx, t->dQ, t->dLRad, orb_dist, check_orientation ? 1 : 0, t->dCount, t->dLists, d_point_quality, d_key_quality,
                       d_assign, d_nmatches);
    return tracker_end(t, st);
}

int ivf_tracker_filter_assign(ivf_tracker* t, int32_t* d_assign, int n_frames, const uint8_t* d_mask, int keep_when_set, uint8_t* d_found,
                              void* hip_stream)
{
    if (!t || !d_assign) return fail(IVF_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, false, 0, 0, n_frames, st);
    if (rc != IVF_OK) return rc;
    if (n_frames == 0 || (!d_mask && !d_found)) return IVF_OK;
    hipLaunchKernelGGL(k_filter_assign, dim3(n_frames), dim3(256), 0, st, t->P.nf, d_assign, d_mask, keep_when_set, d_found);
    return tracker_end(t, st);
}

}  // extern "C"
