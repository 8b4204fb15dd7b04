// ivf_track_db.hip -- the first two lines of Tracking::Relocalization (ORB/src/Tracking.cc:2274-2285), batched and device-resident:
//   * ivf_tracker_bow_vectors: Frame::ComputeBoW's mBowVec (ORB/src/Frame.cc:683-694), i.e. TemplatedVocabulary::transform
//     (TemplatedVocabulary.h:1126-1204) with TF_IDF weights and L1_NORM, for every frame slot of a list of gather records;
//   * ivf_tracker_reloc_candidates: KeyFrameDatabase::DetectRelocalizationCandidates (ORB/src/KeyFrameDatabase.cc:199-309) with
//     L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) for many lost frames against one database given as flat arrays;
//     it writes the (keyframe record, lost frame record) pair table every later step of the chain starts from.
// Nothing crosses PCIe and nothing is replayed on the host.  What the reference computes in an order is computed in that order: the k
// additions of a word that k keypoints reach (keypoint order), the L1 norm and the score's sum (ascending word order), all in f64 with
// -ffp-contract=off; what it only collects (shared words per keyframe, the maximum, the retained set) is collected in parallel.  The
// reference's list order -- first encounter walking the frame's words ascending and each inverted list in insertion order -- is the
// order of (smallest shared word, keyframe index): an inverted list holds keyframes in the order of KeyFrameDatabase::add, and a
// keyframe enters lKFsSharingWords at the first of the frame's words it holds.
//
// Kernels (gfx950, wave = 64; no workgroup waits for another; every loop is bounded by nfeatures, the tree's depth, n_keyframes or 10):
//   k_dbv_leaves   every frame slot through bow_descend_slot (ivf_bow.h) -> the leaf, or -1 for a stopped word, parked in the d_bow_word row
//   k_dbv_vector   one workgroup per frame: sort_keys_and_runs (ivf_bow.h) on the keys word id << 32 | keypoint, one thread per run of
//                  equal words adds the weights in keypoint order, one wave adds the norm in word order, everybody divides
// the three below are ivf_db.h's, shared with ivf_track_loop.hip (DetectLoopCandidates) and instantiated here for the lost-frame query:
//   k_db_common    one workgroup per (frame, tile of 32 keyframes), the frame's words in LDS, one wave per keyframe: shared_word_rounds
//                  takes the keyframe's words 64 per round and finds them in the frame's list (sorted_find, ivf_bow.h); ballot /
//                  popcount = mnRelocWords, the first hit = the smallest shared word; atomicMax -> maxCommonWords of the frame
//   k_db_score     the same shape and the same rounds with the frame's values in LDS too: the terms of a scored keyframe are added
//                  in lane order, i.e. in ascending word order
//   k_db_select    one workgroup per frame: covisibility accumulation per scored keyframe, bestAccScore, retention, the place of every
//                  distinct pBestKF (atomicMin of the retained entries' order keys), their ranks, the candidate / pair / select rows
#include "ivf_db.h"

using namespace ivf;

namespace {

// ---- mBowVec ----------------------------------------------------------------------------------------------------------------------
struct BowVecParams { int nf, nRecords; size_t recBytes; };

__global__ __launch_bounds__(256) void k_dbv_leaves(BowVecParams P, VocabularyView V, const uint8_t* __restrict__ records, const int* __restrict__ frames,
                                                   int* __restrict__ leafOut)
{
    const int s = blockIdx.y;
    const int r = frames[s];
    if (!rec_ok(P.nRecords, r)) return;
    const uint8_t* rec = records + (size_t)r * P.recBytes;
    bow_descend_slot(V.childStart, V.child, V.nodeDesc, rec_desc(rec, P.nf), rec_count(rec, P.nf), blockIdx.x, 0,
                     [&](int f, int leaf, int) { leafOut[(size_t)s * P.nf + f] = word_live(V, leaf) ? leaf : -1; });
}

__global__ __launch_bounds__(256) void k_dbv_vector(BowVecParams P, VocabularyView V, const uint8_t* __restrict__ records, const int* __restrict__ frames,
                                                   unsigned npadMax, int* bowWord, double* bowValue, int* __restrict__ bowN)
{
    extern __shared__ unsigned long long s_key[];             // [npadMax]: word id << 32 | keypoint; then the values
    int* s_leaf = (int*)(s_key + npadMax);                    // [nf] the leaf of every keypoint
    __shared__ int part[256];
    __shared__ double s_norm;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int r = frames[s];
    if (!rec_ok(P.nRecords, r)) { if (tid == 0) bowN[s] = -1; return; }
    const int n = rec_count(records + (size_t)r * P.recBytes, P.nf);
    int* word = bowWord + (size_t)s * P.nf;
    double* value = bowValue + (size_t)s * P.nf;
    // std::map order of the words with the keypoints of a word in the order the loop of TemplatedVocabulary.h:1147-1160 meets them
    const KeyRuns R = sort_keys_and_runs(s_key, key_sort_pad(n), n, tid, [&](unsigned i) {
        const int leaf = word[i];                             // k_dbv_leaves parked it here
        s_leaf[i] = leaf;
        return leaf >= 0 ? sort_key(V.nodeWord[leaf], i) : kNoKey;
    }, part);
    int k = R.k;
    const int total = R.total();                              // words of the vector
    // BowVector::addWeight (BowVector.cpp:34-46): operator[] makes the entry 0.0, then one `+= weight` per keypoint, in keypoint order
    for (int j = R.j0; j < R.j0 + R.per; j++) {
        if (j >= R.m) break;
        if (!R.starts(j)) continue;
        const unsigned w = R.id(j);
        double v = 0.0;
        for (int e = j; e < R.m && R.id(e) == w; e++) v += V.nodeWeight[s_leaf[(unsigned)s_key[e]]];
        word[k] = (int)w; value[k] = v; k++;
    }
    __syncthreads();
    double* s_val = (double*)s_key;
    for (int i = tid; i < total; i += 256) s_val[i] = value[i];
    __syncthreads();
    // BowVector::normalize(L1) (BowVector.cpp:62-84): the sum of fabs in ascending word order by one wave, 64 values per round in its
    // lanes and added lane after lane
    if (tid < 64) {
        double norm = 0.0;
        for (int c = 0; c < total; c += 64) {
            const double v = c + tid < total ? fabs(s_val[c + tid]) : 0.0;
            const int lim = min(64, total - c);
            for (int q = 0; q < lim; q++) norm += readlane_f64(v, q);
        }
        if (tid == 0) s_norm = norm;
    }
    __syncthreads();
    const double norm = s_norm;
    for (int i = tid; i < P.nf; i += 256) {
        if (i < total) { if (norm > 0.0) value[i] = s_val[i] / norm; }
        else { word[i] = -1; value[i] = 0.0; }
    }
    if (tid == 0) bowN[s] = total;
}

// ---- DetectRelocalizationCandidates: k_db_common / k_db_score / k_db_select<false> and db_grow of ivf_db.h ---------------------------------

}  // namespace

extern "C" {

int ivf_tracker_bow_vectors(ivf_tracker* t, const ivf_vocabulary* voc, const uint8_t* d_records, size_t record_bytes, int n_records,
                            const int32_t* d_frames, int n_frames, int32_t* d_bow_word, double* d_bow_value, int32_t* d_bow_n, void* hip_stream)
{
    if (!t || !voc || !d_records || n_frames < 0 || (n_frames > 0 && (!d_frames || !d_bow_word || !d_bow_value || !d_bow_n)))
        return fail(IVF_E_INVALID, "null argument or n_frames < 0");
    if (((size_t)d_records & 15) != 0) return fail(IVF_E_INVALID, "the record block must be 16-byte aligned");
    VocabularyView V;
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = tracker_begin_with_vocabulary(t, voc, &V, true, record_bytes, n_records, 0, st);
    if (rc != IVF_OK) return rc;
    if (n_frames == 0) return IVF_OK;
    const int nf = t->P.nf;
    BowVecParams P;
    P.nf = nf; P.nRecords = n_records; P.recBytes = t->P.recBytes;
    size_t lds;
    const unsigned npad = key_sort_pad(nf, &lds);
    lds += (size_t)nf * sizeof(int);                          // the leaves behind the keys: 16 KB more at most
    // the outputs are the only per-frame storage: a list of any length is walked in chunks the grid's second dimension can hold
    for (int c0 = 0; c0 < n_frames; c0 += 32768) {
        const int nc = n_frames - c0 < 32768 ? n_frames - c0 : 32768;
        int32_t* word = d_bow_word + (size_t)c0 * nf;
        hipLaunchKernelGGL(k_dbv_leaves, dim3((nf + 15) / 16, nc), dim3(256), 0, st, P, V, d_records, d_frames + c0, word);
        hipLaunchKernelGGL(k_dbv_vector, dim3(nc), dim3(256), lds, st, P, V, d_records, d_frames + c0, npad, word, d_bow_value + (size_t)c0 * nf, d_bow_n + c0);
    }
    return tracker_end(t, st);
}

int ivf_tracker_reloc_candidates(ivf_tracker* t, const ivf_vocabulary* voc, const int32_t* d_kf_bow_word, const double* d_kf_bow_value,
                                 const int32_t* d_kf_bow_n, const uint8_t* d_kf_live, const int32_t* d_kf_neigh, const float* d_kf_reloc_score,
                                 const int32_t* d_kf_record, int n_keyframes, const int32_t* d_bow_word, const double* d_bow_value,
                                 const int32_t* d_bow_n, const int32_t* d_frame_record, int n_frames, int max_candidates, int32_t* d_cand,
                                 int32_t* d_ncand, int32_t* d_pairs, int32_t* d_select, float* d_scores, int32_t* d_common, void* hip_stream)
{
    if (!t || !voc) return fail(IVF_E_INVALID, "null argument");
    if (n_keyframes < 0 || n_frames < 0) return fail(IVF_E_INVALID, "n_keyframes %d / n_frames %d is negative", n_keyframes, n_frames);
    if (max_candidates < 1) return fail(IVF_E_INVALID, "max_candidates must be >= 1");
    if (n_keyframes > 0 && (!d_kf_bow_word || !d_kf_bow_value || !d_kf_bow_n || !d_kf_neigh || !d_kf_record))
        return fail(IVF_E_INVALID, "null database array");
    if (n_frames > 0 && (!d_bow_word || !d_bow_value || !d_bow_n || !d_frame_record || !d_cand || !d_ncand || !d_pairs || !d_select))
        return fail(IVF_E_INVALID, "null frame or output array");
    VocabularyView V;
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = tracker_begin_with_vocabulary(t, voc, &V, false, 0, 0, 0, st);
    if (rc != IVF_OK) return rc;
    if (n_frames == 0) return IVF_OK;
    DbParams P;
    P.nf = t->P.nf; P.nK = n_keyframes; P.nF = n_frames; P.maxCand = max_candidates; P.nTiles = (n_keyframes + kKfTile - 1) / kKfTile;
    if ((long long)P.nTiles * n_frames > 0x7fffffffLL) return fail(IVF_E_CAPACITY, "%d frames x %d keyframes exceed one launch", n_frames, n_keyframes);
    rc = db_grow(t, (size_t)n_frames * (size_t)n_keyframes, n_frames);
    if (rc != IVF_OK) return rc;
    const DbScratch S = t->db;
    const DbIn I{d_kf_bow_word, d_kf_bow_value, d_kf_bow_n, d_kf_live, d_kf_neigh, d_kf_reloc_score, d_kf_record, d_bow_word, d_bow_value, d_bow_n, d_frame_record,
                 nullptr, nullptr, nullptr, nullptr};
    HIPCHK(hipMemsetAsync(S.maxCommon, 0, (size_t)n_frames * sizeof(int), st));
    if (n_keyframes > 0) {
        const size_t nf = (size_t)P.nf;
        hipLaunchKernelGGL(k_db_common<false>, dim3(P.nTiles * n_frames), dim3(256), nf * sizeof(int), st, P, I, S);
        hipLaunchKernelGGL(k_db_score<false>, dim3(P.nTiles * n_frames), dim3(256), nf * (sizeof(double) + sizeof(int)), st, P, I, S, d_scores, d_common);
    }
    hipLaunchKernelGGL(k_db_select<false>, dim3(n_frames), dim3(256), 0, st, P, I, S, d_cand, d_ncand, (int2*)d_pairs, d_select);
    return tracker_end(t, st);
}

}  // extern "C"
