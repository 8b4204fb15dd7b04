// ivf_track_local.hip -- ivf_tracker_search_local: the second matcher call of a tracked frame, Tracking::SearchLocalPoints
// (ORB/src/Tracking.cc:2088-2132), for many frames at once, on the batched tracker handle (ivf_tracker.h).  Frame::isInFrustum of every
// local map point (Frame.cc:557-613, MapPoint::PredictScale MapPoint.cc:407-422 with glibc's logf restated) and
// ORBmatcher::SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:45-135): windows on levels [level - 1, level], stereo check, best /
// second best in candidate order, the ratio test between candidates of the same octave, and the ORDER-DEPENDENT occupancy rule (a
// keypoint taken by a point with observations is skipped by later points).
//
// Kernels (all hand-written for gfx950; wave = 64):
//   k_local_prepare  one workgroup per frame: the frame grid (ivf_grid.h, unsigned short indices), then one thread per map point:
//                    projection -> query + radius
//   k_local_window   one wave per (frame, map point): ordered candidate list, entry = index | octave << 12 | distance << 16
//   k_local_greedy   one wave per frame: walks the points in order against the occupancy state in LDS; best and second best are
//                    two DPP minimum reductions of (distance << 12 | list position)
// The map-point gates, the right-coordinate gate, the ordered list and the prefetched walk over the lists are ivf_search.h's; the candidate
// scratch is the handle's one set (ivf_track.hip: tracker_grow_queries), here with max_points_per_frame queries per frame.
#include "ivf_search.h"

using namespace ivf;

namespace {

static_assert(sizeof(ivf_local_point) == 80, "ivf_local_point is read as five 16-byte pieces");
constexpr int kLocalNoBlock = 0x40000000;         // assignment made by a point without observations: later points may replace it (:87-89)

// one workgroup per frame: grid, then Frame::isInFrustum + the window radius of every local map point
__global__ __launch_bounds__(256) void k_local_prepare(TrackParams P, const uint8_t* __restrict__ records, const int* __restrict__ frames,
                                                      const float* __restrict__ poses, const ivf_local_point* __restrict__ points,
                                                      const int* __restrict__ offsets, float th, float cosLimit, int maxM,
                                                      int* __restrict__ gStart, unsigned short* __restrict__ gIdx,
                                                      Query* __restrict__ queries, float* __restrict__ radii)
{
    __shared__ int cnt[kGC * kGR];
    __shared__ int part[256];
    __shared__ int blk[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int ri = frames[f];
    if (!rec_ok(P.nRecords, ri) || offsets[f + 1] < offsets[f] || offsets[f] < 0) return;
    const uint8_t* recC = records + (size_t)ri * P.recBytes;
    const int nC = rec_count(recC, P.nf);
    grid_build(geom_of(P), rec_kps(recC), nC, gStart + (size_t)f * (kGC * kGR + 1), gIdx + (size_t)f * P.nf, cnt, part, blk, tid);

    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, Ow[3];
    if (poses) load_pose(poses + (size_t)f * 12, R, t);                               // the pose of frame SLOT f (a record may appear in two slots)
    neg_rt_mul(R, t, Ow);                                                             // mOw (Frame.cc:554)
    const int m0 = offsets[f], M = min(offsets[f + 1] - m0, maxM);
    Query* Q = queries + (size_t)f * maxM;
    float* Rd = radii + (size_t)f * maxM;
    for (int m = tid; m < M; m += 256) {
        const ivf_local_point mp = points[m0 + m];
        Query q; q.u = 0; q.v = 0; q.ur = 0; q.bits = 0;
        float radius = 0.0f;
        if (!(mp.flags & 1)) {                                                        // isBad() / mnLastFrameSeen == mnId (Tracking.cc:2114-2115)
            float Pc[3];
            mul_add(R, mp.pos, t, Pc);                                                // Frame.cc:565
            if (!(Pc[2] < 0.0f)) {                                                    // :571
                const float invz = 1.0f / Pc[2];
                const float u = P.fx * Pc[0] * invz + P.cx, v = P.fy * Pc[1] * invz + P.cy;
                float dist; int lv;
                if (in_image(P, u, v) && point_range_level(P, mp, Ow, dist, lv)) {     // :579-582, :588-590
                    const float PO[3] = {mp.pos[0] - Ow[0], mp.pos[1] - Ow[1], mp.pos[2] - Ow[2]};   // P - Ow again: the same bits
                    const double dt = (double)PO[0] * (double)mp.normal[0] + (double)PO[1] * (double)mp.normal[1] + (double)PO[2] * (double)mp.normal[2];
                    const float viewCos = (float)(dt / (double)dist);                 // :596
                    if (!(viewCos < cosLimit)) {                                      // :598
                        float r = ((double)viewCos > 0.998) ? 2.5f : 4.0f;            // RadiusByViewingCos (ORBmatcher.cc:137-143)
                        if (th != 1.0f) r *= th;                                      // :65-66
                        radius = r * P.scale[lv];                                     // :69
                        q.u = u; q.v = v; q.ur = u - P.bf * invz;                     // :606-608
                        q.bits = (unsigned)lv | (1u << 24) | ((unsigned)((mp.flags >> 1) & 1) << 25);
                    }
                }
            }
        }
        Q[m] = q; Rd[m] = radius;
    }
}

// one wave per (frame, map point): the ordered candidate list of ORBmatcher.cc:68-100 minus the occupancy test
__global__ __launch_bounds__(256) void k_local_window(TrackParams P, const uint8_t* __restrict__ records, const int* __restrict__ frames,
                                                     const ivf_local_point* __restrict__ points, const int* __restrict__ offsets, int maxM,
                                                     const int* __restrict__ gStart, const unsigned short* __restrict__ gIdx,
                                                     const Query* __restrict__ queries, const float* __restrict__ radii,
                                                     int* __restrict__ count, unsigned* __restrict__ lists)
{
    const int f = blockIdx.y;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int m0 = offsets[f], M = min(offsets[f + 1] - m0, maxM);
    if (m >= M || m0 < 0 || !rec_ok(P.nRecords, frames[f])) return;
    const uint8_t* recC = records + (size_t)frames[f] * P.recBytes;
    const Query q = queries[(size_t)f * maxM + m];
    int total = 0;
    if ((q.bits >> 24) & 1) {
        const int lv = q.bits & 0xff;
        const float r = radii[(size_t)f * maxM + m];
        const uint4* qd = (const uint4*)points[m0 + m].desc;
        const uint4 qa = qd[0], qb = qd[1];
        const float* urC = rec_uright(recC, P.nf);
        const ivf_keypoint* kc = rec_kps(recC);
        unsigned* L = lists + ((size_t)f * maxM + m) * kListCap;
        grid_walk(geom_of(P), kc, rec_desc(recC, P.nf), gStart + (size_t)f * (kGC * kGR + 1), gIdx + (size_t)f * P.nf,
                  q.u, q.v, r, lv - 1, lv, qa, qb, lane, [&](bool ok, int i2, int d) {
                      if (ok) ok = ur_admits(urC[i2], q.ur, r);                           // :91-96
                      list_append(ok, lane, total, L, (unsigned)i2 | ((unsigned)kc[i2].octave << 12) | ((unsigned)d << 16));
                  });
    }
    if (lane == 0) count[(size_t)f * maxM + m] = total;
}

// top two of (key = distance << 12 | ordinal) pairs: a (best, second) pair merged with another one
DEVINL void merge_top2(unsigned& kb, unsigned& eb, unsigned& ks, unsigned& es, unsigned k1, unsigned e1, unsigned k2, unsigned e2)
{
    if (k1 < kb) {
        if (kb < k2) { ks = kb; es = eb; } else { ks = k2; es = e2; }
        kb = k1; eb = e1;
    } else if (k1 < ks) { ks = k1; es = e1; }
}

// one wave per frame: the greedy walk of ORBmatcher.cc:51-126 over the frame's map points.
// Best / second best (:102-114) are updated sequentially in the reference: `dist < bestDist` demotes the best to second, otherwise
// `dist < bestDist2` replaces the second.  That equals "first and second of the candidates ordered by (distance, position)":
//   * the best is the first candidate of minimal distance (a later equal one fails the strict `<`);
//   * a demoted best was the (distance, position)-minimum of everything before the new best, a directly inserted second is the first
//     of its distance among the non-best seen so far, and a later candidate of the same distance never replaces either (strict `<`):
//     by induction the second is the (distance, position)-minimum of all candidates but the best.
// So two minimum reductions of (distance << 12 | position) -- the second with the winner's lane masked -- give both, with their octaves.
__global__ __launch_bounds__(64) void k_local_greedy(TrackParams P, const uint8_t* __restrict__ records, const int* __restrict__ frames,
                                                    const ivf_local_point* __restrict__ points, const int* __restrict__ offsets, int maxM,
                                                    const int* __restrict__ gStart, const unsigned short* __restrict__ gIdx,
                                                    const Query* __restrict__ queries, const float* __restrict__ radii,
                                                    const uint8_t* __restrict__ occupied, float nnRatio, const int* __restrict__ count,
                                                    const unsigned* __restrict__ lists, float* __restrict__ pointQuality,
                                                    float* __restrict__ keyQuality, int* __restrict__ assignOut,
                                                    int* __restrict__ nmatchesOut)
{
    extern __shared__ int s_mem[];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (!rec_ok(P.nRecords, frames[f]) || offsets[f + 1] < offsets[f] || offsets[f] < 0) {
        for (int i = lane; i < P.nf; i += 64) assignOut[(size_t)f * P.nf + i] = -1;
        if (lane == 0) nmatchesOut[f] = -1;
        return;
    }
    int* s_assign = s_mem;                                    // [nf]: -1 free, -2 held by a point with observations before the call,
                                                              // >= 0 local point index (| kLocalNoBlock) assigned by this call
    const uint8_t* recC = records + (size_t)frames[f] * P.recBytes;
    const int nC = rec_count(recC, P.nf);
    const int m0 = offsets[f], M = min(offsets[f + 1] - m0, maxM);
    const uint8_t* occ = occupied ? occupied + (size_t)f * P.nf : nullptr;
    for (int i = lane; i < nC; i += 64) s_assign[i] = (occ && occ[i]) ? -2 : -1;
    wave_sync_lds();
    const Query* Q = queries + (size_t)f * maxM;
    const float* Rd = radii + (size_t)f * maxM;
    const int* C = count + (size_t)f * maxM;
    const unsigned* Lp = lists + (size_t)f * maxM * kListCap;
    int nm = 0;
    auto blocked = [&](int i2) { const int a = s_assign[i2]; return a == -2 || (a >= 0 && !(a & kLocalNoBlock)); };   // :87-89

    walk_lists_prefetched(M, C, Lp, lane, [&](int m) { return Q[m].bits; }, [&](int m, int cnt, unsigned e, auto aux) {
        const unsigned bits = aux();
        unsigned kb = 0xffffffffu, eb = 0, ks = 0xffffffffu, es = 0;               // best / second: key = dist << 12 | ordinal, entry
        if (cnt <= kListCap) {
            const bool ok = lane < cnt && !blocked((int)(e & 0xfff));
            const unsigned key = ok ? ((e >> 16) << 12) | (unsigned)lane : 0xffffffffu;
            kb = wave_min_u32(key);
            if (kb != 0xffffffffu) {
                const int bl = (int)(kb & 63);
                eb = (unsigned)__builtin_amdgcn_readlane((int)e, bl);
                ks = wave_min_u32(lane == bl ? 0xffffffffu : key);
                if (ks != 0xffffffffu) es = (unsigned)__builtin_amdgcn_readlane((int)e, (int)(ks & 63));
            }
        } else {
            // the window overflowed its list: walk it again against the live occupancy state, 64 candidates at a time
            const Query q = Q[m];
            const float r = Rd[m];
            const int lv = bits & 0xff;
            const uint4* qd = (const uint4*)points[m0 + m].desc;
            const uint4 qa = qd[0], qb = qd[1];
            const float* urC = rec_uright(recC, P.nf);
            const ivf_keypoint* kc = rec_kps(recC);
            int ordinal = 0;
            grid_walk(geom_of(P), kc, rec_desc(recC, P.nf), gStart + (size_t)f * (kGC * kGR + 1), gIdx + (size_t)f * P.nf, q.u, q.v, r,
                      lv - 1, lv, qa, qb, lane, [&](bool ok, int i2, int d) {
                          if (ok) ok = ur_admits(urC[i2], q.ur, r);
                          const unsigned pos = (unsigned)list_ordinal(ok, lane, ordinal);
                          if (ok && blocked(i2)) ok = false;
                          const unsigned ew = ok ? ((unsigned)i2 | ((unsigned)kc[i2].octave << 12) | ((unsigned)d << 16)) : 0u;
                          const unsigned key = ok ? ((unsigned)d << 12) | pos : 0xffffffffu;
                          const unsigned k1 = wave_min_u32(key);
                          if (k1 == 0xffffffffu) return;
                          const unsigned long long w1 = __ballot(key == k1);
                          const int l1 = __ffsll((long long)w1) - 1;
                          const unsigned e1 = (unsigned)__builtin_amdgcn_readlane((int)ew, l1);
                          const unsigned k2 = wave_min_u32(lane == l1 ? 0xffffffffu : key);
                          unsigned e2 = 0;
                          if (k2 != 0xffffffffu) {
                              const unsigned long long w2 = __ballot(key == k2 && lane != l1);
                              e2 = (unsigned)__builtin_amdgcn_readlane((int)ew, __ffsll((long long)w2) - 1);
                          }
                          merge_top2(kb, eb, ks, es, k1, e1, k2, e2);
                      });
        }
        if (kb == 0xffffffffu) return;
        const int bestDist = (int)(kb >> 12), bestIdx = (int)(eb & 0xfff), bestLevel = (int)((eb >> 12) & 15);
        if (bestDist > 100) return;                                                 // TH_HIGH (:118)
        if (ks != 0xffffffffu) {
            const int bestDist2 = (int)(ks >> 12), bestLevel2 = (int)((es >> 12) & 15);
            // a candidate AT 256 never becomes second best: bestDist2 starts at 256 and `dist < bestDist2` is strict (:78, :110), so
            // bestLevel2 stays -1 and no ratio test is made
            if (bestDist2 < 256 && bestLevel == bestLevel2 && (float)bestDist > nnRatio * (float)bestDist2) return;   // :120-121
        }
        if (lane == 0) s_assign[bestIdx] = ((bits >> 25) & 1) ? m : (m | kLocalNoBlock);          // :123
        nm++;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    });
    __builtin_amdgcn_wave_barrier();
    int* out = assignOut + (size_t)f * P.nf;
    for (int i = lane; i < P.nf; i += 64) { const int a = i < nC ? s_assign[i] : -1; out[i] = a < 0 ? -1 : (a & ~kLocalNoBlock); }
    // UpdateQualityScores(F) (:128-132) for the keypoints that received a point in THIS call.  Keypoints that held a point before the call
    // went through the same update at the end of the search that gave it to them, and the update is idempotent: min(q_mp, q_kp) == q_kp
    // afterwards.
    if (pointQuality && keyQuality) update_quality_scores(s_assign, nC, ~kLocalNoBlock, lane, 64, pointQuality + m0, keyQuality + (size_t)f * P.nf);
    if (lane == 0) nmatchesOut[f] = nm;
}

}  // namespace

extern "C" int ivf_tracker_search_local(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames,
                                        int n_frames, const float* d_poses, const ivf_local_point* d_points, const int32_t* d_point_offsets,
                                        int max_points_per_frame, const uint8_t* d_occupied, float th, float nn_ratio, float cos_limit,
                                        float* d_point_quality, float* d_key_quality, int32_t* d_assign, int32_t* d_nmatches, void* hip_stream)
{
    if (!d_point_offsets) return fail(IVF_E_INVALID, "null argument");
    const int ra = search_args_ok(t, d_records, d_frames, true, d_points, d_assign, d_nmatches, n_frames, d_point_quality, d_key_quality);
    if (ra != IVF_OK || n_frames == 0) return ra;
    if (max_points_per_frame < 1 || max_points_per_frame >= kLocalNoBlock) return fail(IVF_E_INVALID, "max_points_per_frame %d out of range", max_points_per_frame);
    if (!(th > 0) || !(nn_ratio > 0)) return fail(IVF_E_INVALID, "th and nn_ratio must be positive");
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_frames, st);
    if (rc != IVF_OK) return rc;
    const int rg = tracker_grow_queries(t, max_points_per_frame);
    if (rg != IVF_OK) return rg;
    TrackParams P = t->P;
    P.nRecords = n_records;
    const int M = max_points_per_frame;
    hipLaunchKernelGGL(k_local_prepare, dim3(n_frames), dim3(256), 0, st, P, d_records, d_frames, d_poses, d_points, d_point_offsets, th, cos_limit, M,
                       t->dStart, t->dIdx, t->dQ, t->dLRad);
    hipLaunchKernelGGL(k_local_window, dim3((M + 3) / 4, n_frames), dim3(256), 0, st, P, d_records, d_frames, d_points, d_point_offsets, M,
                       t->dStart, t->dIdx, t->dQ, t->dLRad, t->dCount, t->dLists);
    hipLaunchKernelGGL(k_local_greedy, dim3(n_frames), dim3(64), (size_t)P.nf * 4, st, P, d_records, d_frames, d_points, d_point_offsets, M,
                       t->dStart, t->dIdx, t->dQ, t->dLRad, d_occupied, nn_ratio, t->dCount, t->dLists, d_point_quality, d_key_quality,
                       d_assign, d_nmatches);
    return tracker_end(t, st);
}
