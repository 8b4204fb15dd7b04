// ivf_tracker.h -- the batched tracker handle and what its thirteen translation units share (not part of the public C-ABI):
// ivf_track.hip (the handle's life cycle and the TrackWithMotionModel search), ivf_track_local.hip (SearchLocalPoints),
// ivf_track_bow.hip (TrackReferenceKeyFrame and loop closing's SearchByBoW(KF, KF)), ivf_track_sim3.hip (loop closing's SearchBySim3),
// ivf_track_reloc.hip (Relocalization's SearchByProjection and the set bookkeeping around
// it), ivf_track_db.hip (Relocalization's first two lines: mBowVec and KeyFrameDatabase::DetectRelocalizationCandidates),
// ivf_track_loop.hip (LoopClosing::DetectLoop: minScore, KeyFrameDatabase::DetectLoopCandidates and the consistency groups; what the two
// database queries repeat is ivf_db.h's),
// ivf_track_map.hip (UpdateLocalMap: the local keyframes and points of a frame from a device-resident map),
// ivf_track_points.hip (the points a search hands to a solver and the tail of TrackLocalMap), ivf_track_create.hip
// (LocalMapping::CreateNewMapPoints: new map points for a batch of keyframes), ivf_pose.hip
// (PoseOptimization), ivf_pnp.hip (Relocalization's PnPsolver) and ivf_sim3.hip (loop closing's Sim3Solver).  One definition of struct ivf_tracker, one host statement of the
// camera and record constants (TrackParams), and the device pieces searches and solvers both read (the query record, the pose algebra,
// PredictScale, UpdateQualityScores); what only the projection searches repeat is ivf_search.h's, what only the solvers repeat
// ivf_solve.h's, what the BoW units (ivf_track_bow.hip, ivf_track_db.hip and the per-call transform) repeat ivf_bow.h's.  Of the two
// RANSAC solvers: the cap kRansacMaxIterations, the checks ransac_args_ok; the rest is ivf_solve.h's.  How the handle's scratch is
// allocated, grown and kept through a failed growth is stated once, in ivf_scratch.h (host-only): every unit goes through ivf_tracker::replace.
#pragma once
#include "ivf_bow.h"
#include "ivf_scratch.h"

namespace ivf {

constexpr int kListCap = 64;                      // candidates listed per query (one per lane of the greedy wave)
constexpr int kPrefetch = 16;                     // queries whose lists are in registers ahead of the greedy walk
constexpr int kMaxTrackFeatures = 4096;           // LDS state of k_track_greedy: 20 B per keypoint
constexpr int kRansacMaxIterations = 300;         // ivf_tracker_solve_pnp / _sim3: the cap of max_iterations (Tracking.cc:2317, LoopClosing.cc:280 pass 300)

// The handle's scratch of ivf_tracker_solve_pnp (ivf_pnp.hip), allocated at its first call for max_pairs frames: the compacted
// correspondences [max_pairs][nfeatures] (32 B each), per frame {N, mRansacMinInliers, mRansacMaxIts}, and the f64 pose and inlier count
// of every hypothesis [max_pairs][kRansacMaxIterations]
struct PnpScratch { void* corr; void* head; double* hypPose; int* hypN; };

// The handle's scratch of ivf_tracker_solve_sim3 (ivf_sim3.hip), allocated at its first call for max_pairs pairs: the compacted
// correspondences [max_pairs][nfeatures] (48 B each) and their KF1 keypoint, per pair {N, mRansacMaxIts, mnIterations and mnBestInliers on
// entry}, and (mR12i, mt12i, ms12i) as 16 floats and the inlier count of every hypothesis [max_pairs][kRansacMaxIterations]
struct Sim3Scratch { void* corr; unsigned short* idx; void* head; float* hyp; int* hypN; };

// The handle's scratch of ivf_tracker_reloc_candidates (ivf_track_db.hip), grown on demand to cap >= n_frames * n_keyframes cells and
// frameCap >= n_frames: per (frame, keyframe) mnRelocWords, the smallest shared word, this query's score, accScore, pBestKF, the place
// (smallest shared word << 32 | keyframe) of the first retained entry that names the keyframe as its pBestKF, and the frame's compacted
// candidate list (keyframe and place); per frame maxCommonWords
struct DbScratch {
    int *common, *minWord; float* score; float* acc; int* best; unsigned long long* place; int* list; unsigned long long* listKey; int* maxCommon;
    size_t cap; int frameCap;
};

// The handle's scratch of ivf_tracker_loop_consistency (ivf_track_loop.hip), one buffer of cap 4-byte words grown on demand and carved by
// the call: per candidate of ONE query the bitmap of its covisibility group over the keyframes, its size, flags and first new entry; per
// (candidate, previous group) whether they share a keyframe; per previous group its first consistent candidate; per new entry its
// candidate and counter
struct LoopScratch { unsigned* buf; size_t cap; };

// The handle's scratch of ivf_tracker_update_local_map (ivf_track_map.hip), grown on demand: the vote rows [n_frames][n_keyframes] of the
// calls whose n_keyframes exceeds the LDS row (voteCap ints), and per frame the hash set of the de-duplication, `slots` point ids
// followed by `slots` first positions (hashCap words of 4 bytes in all)
struct MapScratch { int* vote; unsigned* hash; size_t voteCap, hashCap; };

struct TrackParams {                               // uniform kernel arguments
    int nf, nlevels;
    float scale[kMaxLevels];
    float fx, fy, cx, cy, invfx, invfy, bf, b;
    float minX, minY, maxX, maxY, invW, invH;     // image bounds and mfGridElementWidthInv / HeightInv (Frame.cc:208-209)
    float thDepth;                                // > 0: UpdateLastFrame's close-point rule
    float logScale;                               // mfLogScaleFactor = logf(mfScaleFactor) (Frame.cc:106)
    int checkOri, defaultBlocks;
    int nRecords;                                 // records in the block of THIS call: every index read from a pair / frame table is checked against it
    size_t recBytes;
};
// a pair / frame table built for another block (a different world size or batch) must not read outside this one: such an entry
// gets nmatches = -1, assign = -1 and is otherwise skipped
__device__ __forceinline__ bool rec_ok(int nRecords, int r) { return (unsigned)r < (unsigned)nRecords; }
// the grid geometry of grid_build / grid_walk (ivf_grid.h), by value: the fields keep their place in the kernel arguments
__device__ __forceinline__ GridGeom geom_of(const TrackParams& P) { return GridGeom{P.minX, P.minY, P.invW, P.invH}; }

// glibc >= 2.27 logf (oracle/ivf_oracle.c:orc_logf is the same arithmetic, checked against libm for every positive
// normal float): what MapPoint::PredictScale's log(ratio) resolves to.  Positive normal arguments only (a distance ratio); any other
// bit pattern still indexes inside the table and returns some finite or non-finite float.
static __constant__ double c_logfT[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
    {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
    {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
    {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
    {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
    {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2}};
__device__ __forceinline__ float glibc_logf(float x)
{
    const unsigned ix = __builtin_bit_cast(unsigned, x);
    if (ix == 0x3f800000u) return 0.0f;
    const unsigned tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) & 15u);
    const int k = (int)tmp >> 23;
    const double z = (double)__builtin_bit_cast(float, ix - (tmp & 0xff800000u)), invc = c_logfT[i][0], logc = c_logfT[i][1];
    const double r = z * invc - 1.0;
    const double y0 = logc + (double)k * 0x1.62e42fefa39efp-1;
    const double r2 = r * r;
    double y = 0x1.5575b0be00b6ap-2 * r + -0x1.ffffef20a4123p-2;
    y = -0x1.00ea348b88334p-2 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}
// MapPoint::PredictScale (MapPoint.cc:407-422) as compiled: logf, a float quotient, std::ceil(float), the clamp to [0, nlevels - 1].
// The one statement of it, behind point_range_level (ivf_search.h): SearchLocalPoints and Relocalization's SearchByProjection.
__device__ __forceinline__ int predict_scale(const TrackParams& P, float maxDistance, float dist)
{
    const float ratio = maxDistance / dist;
    const int lv = (int)ceilf(glibc_logf(ratio) / P.logScale);
    return lv < 0 ? 0 : (lv >= P.nlevels ? P.nlevels - 1 : lv);
}

// per-query record written by k_track_prepare / k_local_prepare / k_reloc_prepare: projection (u, v), ur = u - bf * invzc, and the packed
// {octave, minLevel + 1, maxLevel + 1, flags: bit 0 valid, bit 1 blocks}
struct __attribute__((aligned(16))) Query { float u, v, ur; unsigned bits; };
// The handle's scratch of ivf_tracker_search_by_sim3 (ivf_track_sim3.hip), allocated at its first call for max_pairs pairs, two slots
// (direction 1 -> 2, 2 -> 1) per pair: the queries and radii [2 * max_pairs][nfeatures] and vnMatch1 / vnMatch2.  Its own, not the
// candidate scratch of the projection searches: that one carries kListCap list entries per query, which this search never writes.
struct Sim3SearchScratch { Query* q; float* rad; int* vn; };
__device__ __forceinline__ unsigned pack_bits(int oct, int lo, int hi, int valid, int blocks)
{ return (unsigned)oct | ((unsigned)(lo + 1) << 8) | ((unsigned)(hi + 1) << 16) | ((unsigned)valid << 24) | ((unsigned)blocks << 25); }

// a row-major 3x4 pose [R | t] (cv::Mat mTcw without its last row)
__device__ __forceinline__ void load_pose(const float* __restrict__ T, float* R, float* t)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = T[4 * i + j];
        t[i] = T[4 * i + 3];
    }
}

// Frame::UnprojectStereo (Frame.cc:958-972) of keypoint kp at depth z under the frame's pose [Rl | tl]: mRwc * x3Dc + mOw with
// mRwc = mRcw.t() and mOw = -mRcw.t() * mtcw.  The one statement of it: ivf_tracker_run projects these points (k_track_prepare) and
// ivf_tracker_points_from_pairs hands the same bits to the solvers.
__device__ __forceinline__ void unproject_stereo(const TrackParams& P, const float* Rl, const float* tl, const ivf_keypoint& kp, float z, float* xw)
{
    float Rwl[9], Owl[3], x3[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rwl[3 * i + j] = Rl[3 * j + i];
    neg_rt_mul(Rl, tl, Owl);
    x3[0] = (kp.x - P.cx) * z * P.invfx; x3[1] = (kp.y - P.cy) * z * P.invfy; x3[2] = z;
    mul_add(Rwl, x3, Owl, xw);
}

// ORBmatcher::UpdateQualityScores (ORBmatcher.cc:1108-1121) at the end of a search, for the keypoints i = tid, tid + stride, ... < n of one
// frame: assign[i] < 0: no point, else point (assign[i] & idMask).  A point ends on at most one keypoint of the frame, so the
// reference's sequential loop has no cross-iteration dependence here.
constexpr float kDeltaThresh = 0.01f;
__device__ __forceinline__ void update_quality_scores(const int* assign, int n, int idMask, int tid, int stride, float* pq, float* kq)
{
    for (int i = tid; i < n; i += stride) {
        const int a = assign[i];
        if (a < 0) continue;
        const int m = a & idMask;
        const float mq = pq[m], upd = fminf(mq, kq[i]);
        if (fabsf(upd - mq) > kDeltaThresh) pq[m] = upd;
        kq[i] = upd;
    }
}

}  // namespace ivf

struct ivf_tracker {
    ivf_track_config cfg;
    ivf::TrackParams P;                   // nRecords is the one per-call field: every entry point sets it in its own copy
    // the device grids (ivf_grid.h), [max_pairs * gridCap] of them: gridCap is 1 (one grid per pair: the record every projection search
    // looks into) until ivf_tracker_search_by_sim3, which searches both records of a pair, grows it to 2 (tracker_grow_grids)
    int *dStart = nullptr, *dRetry = nullptr;
    unsigned short* dIdx = nullptr;
    int gridCap = 0;
    // the candidate scratch of the three projection searches, [max_pairs][queryCap] queries, radii (search_local, search_reloc),
    // counts, lists: queryCap starts at nfeatures (run and search_reloc index it with that stride) and grows on demand
    // (tracker_grow_queries) to search_local's max_points_per_frame, its stride
    ivf::Query* dQ = nullptr; float* dLRad = nullptr; int* dCount = nullptr; unsigned* dLists = nullptr; int queryCap = 0;
    ivf::TrackerBowScratch bow{nullptr, nullptr, nullptr, nullptr, nullptr};   // ivf_tracker_search_by_bow: [2 * max_pairs] slots
    ivf::PnpScratch pnp{nullptr, nullptr, nullptr, nullptr};
    ivf::Sim3Scratch sim3{nullptr, nullptr, nullptr, nullptr, nullptr};
    ivf::Sim3SearchScratch sim3s{nullptr, nullptr, nullptr};
    ivf::DbScratch db{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    ivf::MapScratch map{nullptr, nullptr, 0, 0};
    ivf::LoopScratch loop{nullptr, 0};
    size_t ldsBytes = 0;
    hipEvent_t evDone = nullptr;          // end of the previous call: the scratch above belongs to ONE call at a time
    bool ran = false;
    std::vector<void*> owned;             // the members above that hold a device buffer (ivf_scratch.h): ivf_tracker_destroy frees these
    // ivf_scratch.h's device: a refused allocation also consumes the runtime's last-error word, so that the failure is reported once, by
    // the call that caused it, and not again by the next call's tracker_end.  Every scratch set of the handle is allocated and grown
    // through replace(), as {member, bytes} entries: all of them are replaced, or (false) none
    struct Device {
        ivf_tracker* t;
        void* alloc(size_t bytes) { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : ((void)hipGetLastError(), nullptr); }
        void free(void* p) { (void)hipFree(p); }
        bool wait() { return !t->ran || hipEventSynchronize(t->evDone) == hipSuccess; }
    };
    bool replace(std::initializer_list<ivf::ScratchSlot> set) { return ivf::scratch_replace(Device{this}, owned, set); }
};

namespace ivf {
// tracker_begin: the argument checks every tracker entry point shares, hipSetDevice and the wait for the handle's previous call;
// tracker_begin_with_vocabulary: the same for the entry points that take a vocabulary (ivf_track_bow.hip, ivf_track_db.hip) -- its view
// first, then tracker_begin, then that both live on one device;
// tracker_end: the event the next call waits for;
// search_args_ok: what the three projection searches check alike -- the pointers (points: the array of search_local / search_reloc),
// the 16-byte alignment of what the kernels read as uint4 and, in a call of n_items != 0, that the quality arrays come together;
// ransac_args_ok: what ivf_pnp.hip and ivf_sim3.hip check alike -- the record block's alignment, max_iterations, probability, min_inliers;
// tracker_grow_queries: the candidate scratch (dQ, dLRad, dCount, dLists) for at least `cap` queries per frame / pair;
// tracker_grow_grids: the grid scratch (dStart, dIdx) for at least `per_pair` grids per pair
int tracker_begin(ivf_tracker* t, bool reads_records, size_t record_bytes, int n_records, int n_items, hipStream_t st);
int tracker_begin_with_vocabulary(ivf_tracker* t, const ivf_vocabulary* voc, VocabularyView* V, bool reads_records, size_t record_bytes, int n_records,
                                  int n_items, hipStream_t st);
int tracker_end(ivf_tracker* t, hipStream_t st);
int search_args_ok(const ivf_tracker* t, const void* records, const void* items, bool has_points, const void* points, const void* assign,
                   const void* nmatches, int n_items, const float* point_quality, const float* key_quality);
int ransac_args_ok(const void* records, int max_iterations, double probability, int min_inliers);
int tracker_grow_queries(ivf_tracker* t, int cap);
int tracker_grow_grids(ivf_tracker* t, int per_pair);
}  // namespace ivf
