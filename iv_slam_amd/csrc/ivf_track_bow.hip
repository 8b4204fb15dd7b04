// ivf_track_bow.hip -- batched, device-resident matcher part of Tracking::TrackReferenceKeyFrame (ORB/src/Tracking.cc:1154-1250), the
// fallback of a frame that ivf_tracker_run could not track: for every (reference keyframe, current frame) pair of gather records
//   * Frame::ComputeBoW (Tracking.cc:1168, ORB/src/Frame.cc:683-694) reduced to what the search reads of it: mFeatVec, the node at level
//     L - levelsup of every keypoint's descriptor (TemplatedVocabulary.h:1217-1259), features of a node in ascending order
//     (FeatureVector.cpp:31-45); mBowVec is not computed;
//   * ORBmatcher(nn_ratio, check_orientation).SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches) (ORB/src/ORBmatcher.cc:165-294);
//   * ORBmatcher::UpdateQualityScores(mCurrentFrame) (Tracking.cc:1174-1176, ORBmatcher.cc:1108-1121) when the quality arrays are given.
// and, on the same kernel body, loop closing's ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORB/src/ORBmatcher.cc:528-661, called at
// LoopClosing.cc:270) for (current keyframe, candidate) pairs: ivf_tracker_search_by_bow_keyframes, whose d_match12 ivf_tracker_solve_sim3 reads.
// Nothing crosses PCIe and nothing is replayed on the host.  The search parallelises exactly: a FeatureVector holds every feature in
// exactly one node, and the loop's only serial dependence -- `if(vpMapPointMatches[realIdxF]) continue;` (:215) -- links keyframe
// features of the SAME node only.  Nodes are independent (whichever wave takes whichever node, in whatever order, the result is the
// same); inside a node one wave walks the keyframe features in list order with the frame's features in its lanes.  The rotation
// histogram needs the bin counts and the members of each bin, not the push order.
//
// Kernels (gfx950, wave = 64; no workgroup waits for another, every loop is bounded by nfeatures or by the node count):
//   k_bow_nodes    every record slot (2 * pair + side) through bow_descend_slot (ivf_bow.h): the node of every keypoint, -1 on a stopped word
//   k_bow_featvec  one workgroup per slot: sort_keys_and_runs (ivf_bow.h) on the keys node id << 32 | feature index -> the CSR feature
//                  vector in the handle's scratch
//   k_bow_search   one workgroup per pair: node merge (sorted_find of every keyframe node in the frame's list: only equal ids match,
//                  the lower_bound walk of :186-270), the common nodes handed to the four waves one at a time, the greedy walk,
//                  the rotation filter (rot_bin / rot_three_maxima, ivf_device.h), the quality epilogue (ivf_tracker.h)
//                  k_bow_search_keyframes is the same body (bow_search_body) with the differences of the (KF, KF) overload: vbMatched2 links
//                  KF2 features of one node only, so the argument above carries over unchanged
// Which pairs take part (pair_live) is ivf_search.h's, the one test of it for every search of the handle.
#include "ivf_search.h"

using namespace ivf;

namespace {

struct BowParams {
    int nf, nRecords, nidLevel, checkOri;
    size_t recBytes;
    float nnRatio;
};

// the record of slot s = 2 * pair + side of a pair that takes part, or null
DEVINL const uint8_t* slot_record(const BowParams& P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs, const int* __restrict__ select, int s)
{
    const int p = s >> 1;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p)) return nullptr;
    return records + (size_t)((s & 1) ? pr.y : pr.x) * P.recBytes;
}

__global__ __launch_bounds__(256) void k_bow_nodes(BowParams P, VocabularyView V, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                  const int* __restrict__ select, int* __restrict__ nodeKey)
{
    const int s = blockIdx.y;
    const uint8_t* rec = slot_record(P, records, pairs, select, s);
    if (!rec) return;
    bow_descend_slot(V.childStart, V.child, V.nodeDesc, rec_desc(rec, P.nf), rec_count(rec, P.nf), blockIdx.x, P.nidLevel,
                     [&](int f, int leaf, int nid) { nodeKey[(size_t)s * P.nf + f] = word_live(V, leaf) ? nid : -1; });
}

__global__ __launch_bounds__(256) void k_bow_featvec(BowParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                    const int* __restrict__ select, TrackerBowScratch B)
{
    extern __shared__ unsigned long long s_key[];             // [npad]: node id << 32 | feature index
    __shared__ int part[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const uint8_t* rec = slot_record(P, records, pairs, select, s);
    if (!rec) return;
    featvec_of_slot(B, s, P.nf, rec_count(rec, P.nf), s_key, part, tid);
}

// The one body of both SearchByBoW overloads.  KF2KF = false: SearchByBoW(KeyFrame*, Frame&) (:165-294), side 2 is the current frame, the
// result is indexed by ITS keypoint.  KF2KF = true: SearchByBoW(KeyFrame*, KeyFrame*) (:528-661): a KF2 candidate must itself hold a live
// point (:580-586), the occupancy is vbMatched2 (by KF2 keypoint, the same s_assign), the acceptance is bestDist1 < TH_LOW strictly (:604),
// the result is vpMatches12, indexed by KF1 keypoint, a dead pair writes nothing but its count, and there is no quality epilogue.
template <bool KF2KF>
DEVINL void bow_search_body(const BowParams& P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                            const int* __restrict__ select, const uint8_t* __restrict__ pointFlags, const TrackerBowScratch& B,
                            float* __restrict__ pointQuality, float* __restrict__ keyQuality,
                            int* __restrict__ assignOut, int* __restrict__ nmatchesOut)
{
    extern __shared__ int s_mem[];
    int* s_assign = s_mem;                                    // [nf] vpMapPointMatches as keyframe keypoint | bin << 16, or -1
    int* s_common = s_mem + P.nf;                             // [nf] nodes on both sides: position in the keyframe's list | the frame's << 12
    __shared__ int s_hist[32];                                // rotHist[b].size()
    __shared__ int s_nCommon, s_next, s_nm;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int* out = assignOut + (size_t)p * P.nf;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, select, p)) {
        if (!KF2KF) for (int i = tid; i < P.nf; i += 256) out[i] = -1;
        if (tid == 0) nmatchesOut[p] = (select && select[p] == 0) ? -2 : -1;
        return;
    }
    const uint8_t* recK = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recF = records + (size_t)pr.y * P.recBytes;
    const int nF = rec_count(recF, P.nf);
    const size_t sK = 2 * (size_t)p, sF = sK + 1;
    const int* nodeK = B.fvNode + sK * P.nf; const int* nodeF = B.fvNode + sF * P.nf;
    const int* startK = B.fvStart + sK * (P.nf + 1); const int* startF = B.fvStart + sF * (P.nf + 1);
    const int* idxK = B.fvIdx + sK * P.nf; const int* idxF = B.fvIdx + sF * P.nf;
    const int nnK = B.fvN[sK], nnF = B.fvN[sF];
    for (int i = tid; i < nF; i += 256) s_assign[i] = -1;
    if (tid < 32) s_hist[tid] = 0;
    if (tid == 0) { s_nCommon = 0; s_next = 0; s_nm = 0; }
    __syncthreads();
    // ---- node merge (:186-270): a keyframe node takes part when the frame's ascending list holds the same id
    for (int a = tid; a < nnK; a += 256) {
        const int b = sorted_find(nodeF, nnF, nodeK[a]);
        if (b >= 0) s_common[atomicAdd(&s_nCommon, 1)] = a | (b << 12);
    }
    __syncthreads();
    const int nCommon = s_nCommon;
    const ivf_keypoint* kK = rec_kps(recK);
    const ivf_keypoint* kF = rec_kps(recF);
    const uint8_t* dK = rec_desc(recK, P.nf);
    const uint8_t* dF = rec_desc(recF, P.nf);
    const float* zK = rec_depth(recK, P.nf);
    const uint8_t* fl = pointFlags ? pointFlags + (size_t)pr.x * P.nf : nullptr;
    const float* zF = rec_depth(recF, P.nf);                  // KF2KF: the candidate's own point, by the rule of side 1
    const uint8_t* fl2 = pointFlags ? pointFlags + (size_t)pr.y * P.nf : nullptr;
    auto holds2 = [&](int iF) { return fl2 ? (fl2[iF] & 1) != 0 : zF[iF] > 0; };
    int nmWave = 0;
    for (;;) {
        int c = 0;
        if (lane == 0) c = atomicAdd(&s_next, 1);
        c = __builtin_amdgcn_readfirstlane(c);
        if (c >= nCommon) break;
        const int e = s_common[c], a = e & 0xfff, b = e >> 12;
        const int ks = startK[a], ke = startK[a + 1], fs = startF[b], nFn = startF[b + 1] - fs;      // both runs hold at least one feature
        // the frame's first 64 features of the node stay in registers for every keyframe feature of the node; all loads of a lane are
        // unconditional, at an index clamped into the run, and requested before the first reduction reads them
        const int iF0 = idxF[fs + min(lane, nFn - 1)];
        const uint4* pf0 = (const uint4*)(dF + (size_t)iF0 * 32);
        const uint4 fa0 = pf0[0], fb0 = pf0[1];
        const float ang0 = kF[iF0].angle;
        bool pt0 = true;
        if (KF2KF) pt0 = holds2(iF0);
        for (int k0 = ks; k0 < ke; k0 += 64) {
            // 64 keyframe features at once: index, map point, descriptor and angle of feature k0 + lane, broadcast from its lane in turn
            const int i1L = idxK[min(k0 + lane, ke - 1)];
            const bool pointL = fl ? (fl[i1L] & 1) != 0 : zK[i1L] > 0;
            const uint4* pk = (const uint4*)(dK + (size_t)i1L * 32);
            const uint4 kaL = pk[0], kbL = pk[1];
            const float angL = kK[i1L].angle;
            unsigned long long todo = __ballot(k0 + lane < ke && pointL);                          // :199-203
            while (todo) {
                const int k = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const uint4 qa = readlane_u4(kaL, k), qb = readlane_u4(kbL, k);
                const int i1 = __builtin_amdgcn_readlane(i1L, k);
                const float angK = readlane_f32(angL, k);
                // per lane over its strides: the smallest (distance, list position) and the smallest distance among its others
                unsigned bestKey = 0xffffffffu; int second = 256, bestI = 0; float bestAng = 0.0f;
                for (int q = 0; q < nFn; q += 64) {
                    int iF = iF0; uint4 fa = fa0, fb = fb0; float ang = ang0; bool pt = pt0;
                    if (q) {
                        iF = idxF[fs + min(q + lane, nFn - 1)];
                        const uint4* pf = (const uint4*)(dF + (size_t)iF * 32);
                        fa = pf[0]; fb = pf[1]; ang = kF[iF].angle;
                        if (KF2KF) pt = holds2(iF);
                    }
                    const bool free_ = q + lane < nFn && s_assign[iF] < 0 && pt;                   // :215; :580-586
                    const unsigned d = (unsigned)hamming256(qa, qb, fa, fb);
                    const unsigned key = free_ ? (d << 12) | (unsigned)(q + lane) : 0xffffffffu;
                    if (key < bestKey) { second = min(second, (int)min(bestKey >> 12, 256u)); bestKey = key; bestI = iF; bestAng = ang; }
                    else second = min(second, (int)min(key >> 12, 256u));
                }
                // :222-231: bestDist1 = the first minimum in list order (strict <), bestDist2 = the smallest distance of all the others
                const unsigned best = wave_min_u32(bestKey);
                if (best == 0xffffffffu) continue;                                                  // every candidate taken
                const int who = __ffsll((long long)__ballot(bestKey == best)) - 1;
                const int bestDist1 = (int)(best >> 12);
                const int bestDist2 = (int)wave_min_u32(lane == who ? (unsigned)second : min(bestKey >> 12, 256u));
                if ((KF2KF ? bestDist1 < 50 : bestDist1 <= 50) && (float)bestDist1 < P.nnRatio * (float)bestDist2) {   // TH_LOW, mfNNratio (:234-236; :604-606)
                    const int bestIdxF = __builtin_amdgcn_readlane(bestI, who);
                    int bin = 0;
                    if (P.checkOri) bin = rot_bin(angK - readlane_f32(bestAng, who));
                    if (lane == 0) {
                        s_assign[bestIdxF] = i1 | (bin << 16);                                       // seen by the next keyframe feature of this node
                        if (P.checkOri) atomicAdd(&s_hist[bin], 1);
                    }
                    nmWave++;
                    wave_sync_lds();
                }
            }
        }
    }
    if (lane == 0 && nmWave) atomicAdd(&s_nm, nmWave);
    __syncthreads();
    if (P.checkOri) {
        const RotKeep keep = rot_three_maxima(s_hist);                                              // :273-291
        int removed = 0;
        for (int i = tid; i < nF; i += 256) {
            const int a = s_assign[i];
            if (a >= 0 && !keep.keeps(a >> 16)) { s_assign[i] = -1; removed++; }
        }
        if (removed) atomicSub(&s_nm, removed);
        __syncthreads();
    }
    if (KF2KF) {
        // vpMatches12 by KF1 keypoint: a KF1 feature is walked once, so it names at most one KF2 keypoint; the node list is done with
        int* s_m12 = s_common;
        for (int i = tid; i < P.nf; i += 256) s_m12[i] = -1;
        __syncthreads();
        for (int i = tid; i < nF; i += 256) { const int a = s_assign[i]; if (a >= 0) s_m12[a & 0xffff] = i; }
        __syncthreads();
        for (int i = tid; i < P.nf; i += 256) out[i] = s_m12[i];
        if (tid == 0) nmatchesOut[p] = s_nm;
        return;
    }
    for (int i = tid; i < P.nf; i += 256) { const int a = i < nF ? s_assign[i] : -1; out[i] = a < 0 ? -1 : (a & 0xffff); }
    // UpdateQualityScores(mCurrentFrame) (Tracking.cc:1174-1176)
    if (pointQuality && keyQuality) update_quality_scores(s_assign, nF, 0xffff, tid, 256, pointQuality + (size_t)p * P.nf, keyQuality + (size_t)p * P.nf);
    if (tid == 0) nmatchesOut[p] = s_nm;
}

__global__ __launch_bounds__(256) void k_bow_search(BowParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                   const int* __restrict__ select, const uint8_t* __restrict__ pointFlags, TrackerBowScratch B,
                                                   float* __restrict__ pointQuality, float* __restrict__ keyQuality,
                                                   int* __restrict__ assignOut, int* __restrict__ nmatchesOut)
{
    bow_search_body<false>(P, records, pairs, select, pointFlags, B, pointQuality, keyQuality, assignOut, nmatchesOut);
}

__global__ __launch_bounds__(256) void k_bow_search_keyframes(BowParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                             const int* __restrict__ select, const uint8_t* __restrict__ pointFlags,
                                                             TrackerBowScratch B, int* __restrict__ match12, int* __restrict__ nmatchesOut)
{
    bow_search_body<true>(P, records, pairs, select, pointFlags, B, nullptr, nullptr, match12, nmatchesOut);
}

}  // namespace

extern "C" {

// both entry points: the checks, the feature vectors of both records of every pair, the search of one of the two overloads
static int search_by_bow(bool kf2kf, ivf_tracker* t, const ivf_vocabulary* voc, int levelsup, const uint8_t* d_records, size_t record_bytes, int n_records,
                         const int32_t* d_pairs, int n_pairs, const int32_t* d_select, const uint8_t* d_point_flags, float nn_ratio,
                         int check_orientation, float* d_point_quality, float* d_key_quality, int32_t* d_assign, int32_t* d_nmatches,
                         void* hip_stream)
{
    if (!t || !voc || !d_records || !d_pairs || !d_assign || !d_nmatches) return fail(IVF_E_INVALID, "null argument");
    if (((size_t)d_records & 15) != 0) return fail(IVF_E_INVALID, "the record block must be 16-byte aligned");
    if (levelsup < 0) return fail(IVF_E_INVALID, "levelsup %d is negative", levelsup);
    if (!(nn_ratio > 0)) return fail(IVF_E_INVALID, "nn_ratio must be positive");
    if ((d_point_quality == nullptr) != (d_key_quality == nullptr)) return fail(IVF_E_INVALID, "d_point_quality and d_key_quality come together");
    VocabularyView V;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin_with_vocabulary(t, voc, &V, true, record_bytes, n_records, n_pairs, st);
    if (rc != IVF_OK) return rc;
    if (n_pairs == 0) return IVF_OK;
    const int nf = t->P.nf;
    BowParams P;
    P.nf = nf; P.nRecords = n_records; P.nidLevel = V.depth - levelsup; P.checkOri = check_orientation ? 1 : 0;
    P.recBytes = t->P.recBytes; P.nnRatio = nn_ratio;
    const TrackerBowScratch B = t->bow;
    const int2* pairs = (const int2*)d_pairs;
    size_t keyBytes;
    key_sort_pad(nf, &keyBytes);
    hipLaunchKernelGGL(k_bow_nodes, dim3((nf + 15) / 16, 2 * n_pairs), dim3(256), 0, st, P, V, d_records, pairs, d_select, B.nodeKey);
    hipLaunchKernelGGL(k_bow_featvec, dim3(2 * n_pairs), dim3(256), keyBytes, st, P, d_records, pairs, d_select, B);
    if (kf2kf)
        hipLaunchKernelGGL(k_bow_search_keyframes, dim3(n_pairs), dim3(256), (size_t)nf * 2 * sizeof(int), st, P, d_records, pairs, d_select,
                           d_point_flags, B, d_assign, d_nmatches);
    else
        hipLaunchKernelGGL(k_bow_search, dim3(n_pairs), dim3(256), (size_t)nf * 2 * sizeof(int), st, P, d_records, pairs, d_select, d_point_flags, B,
                           d_point_quality, d_key_quality, d_assign, d_nmatches);
    return tracker_end(t, st);
}

int ivf_tracker_search_by_bow(ivf_tracker* t, const ivf_vocabulary* voc, int levelsup, const uint8_t* d_records, size_t record_bytes, int n_records,
                              const int32_t* d_pairs, int n_pairs, const int32_t* d_select, const uint8_t* d_point_flags, float nn_ratio,
                              int check_orientation, float* d_point_quality, float* d_key_quality, int32_t* d_assign, int32_t* d_nmatches,
                              void* hip_stream)
{
    return search_by_bow(false, t, voc, levelsup, d_records, record_bytes, n_records, d_pairs, n_pairs, d_select, d_point_flags, nn_ratio,
                         check_orientation, d_point_quality, d_key_quality, d_assign, d_nmatches, hip_stream);
}

int ivf_tracker_search_by_bow_keyframes(ivf_tracker* t, const ivf_vocabulary* voc, int levelsup, const uint8_t* d_records, size_t record_bytes,
                                        int n_records, const int32_t* d_pairs, int n_pairs, const int32_t* d_select, const uint8_t* d_point_flags,
                                        float nn_ratio, int check_orientation, int32_t* d_match12, int32_t* d_nmatches, void* hip_stream)
{
    return search_by_bow(true, t, voc, levelsup, d_records, record_bytes, n_records, d_pairs, n_pairs, d_select, d_point_flags, nn_ratio,
                         check_orientation, nullptr, nullptr, d_match12, d_nmatches, hip_stream);
}

}  // extern "C"
