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
//   k_db_common    one workgroup per (frame, tile of 32 keyframes), the frame's words in LDS, one wave per keyframe: shared_word_rounds
//                  takes the keyframe's words 64 per round and finds them in the frame's list (sorted_find, ivf_bow.h); ballot /
//                  popcount = mnRelocWords, the first hit = the smallest shared word; atomicMax -> maxCommonWords of the frame
//   k_db_score     the same shape and the same rounds with the frame's values in LDS too: the terms of a scored keyframe are added
//                  in lane order, i.e. in ascending word order
//   k_db_select    one workgroup per frame: covisibility accumulation per scored keyframe, bestAccScore, retention, the place of every
//                  distinct pBestKF (atomicMin of the retained entries' order keys), their ranks, the candidate / pair / select rows
#include "ivf_tracker.h"

using namespace ivf;

namespace {

constexpr int kKfTile = 32;                        // keyframes per workgroup of k_db_common / k_db_score: 8 per wave
constexpr int kNeigh = 10;                         // GetBestCovisibilityKeyFrames(10) (KeyFrameDatabase.cc:265)
constexpr unsigned kNoScoreBits = 0x7fc00000u;     // d_scores of a keyframe that was not scored (include/ivfront.h)
constexpr unsigned long long kNoPlace = ~0ull;

DEVINL int clamp_count(int n, int nf) { return n < 0 ? 0 : (n > nf ? nf : n); }
// int minCommonWords = maxCommonWords*0.8f (KeyFrameDatabase.cc:235): the product in float, where a double 0.8 would round some counts
// the other way; a keyframe is scored when it shares MORE words than that (:246), and only scored keyframes are accumulated (:262)
DEVINL int min_common(int maxCommon) { return (int)((float)maxCommon * 0.8f); }
DEVINL bool scored(int common, int minCommon) { return common > minCommon; }

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

// ---- DetectRelocalizationCandidates -------------------------------------------------------------------------------------------------
struct DbParams { int nf, nK, nF, maxCand, nTiles; };
struct DbIn {
    const int* kfWord; const double* kfValue; const int* kfN; const uint8_t* kfLive; const int* kfNeigh; const float* kfReloc; const int* kfRecord;
    const int* fWord; const double* fValue; const int* fN; const int* fRecord;
};

// the words keyframe k brings to a query of a frame with nW words: none when it was erased (it is in no inverted list) or the frame is empty
DEVINL int kf_words(const DbParams& P, const DbIn& I, int k, int nW)
{
    if (nW == 0 || (I.kfLive && I.kfLive[k] == 0)) return 0;
    return clamp_count(I.kfN[k], P.nf);
}
// the keyframe's ascending words kw[0 .. nk), 64 per round in the lanes of one wave, looked up in the frame's ascending list
// s_fw[0 .. nW) (LDS): round(hit, w, pos, x) gets the ballot of the lanes whose word the frame holds (lane order = word order), the
// lane's word, its position in the frame's list (-1: not there, or a lane past the end, which reads word nk - 1) and x = fetch(j), what
// the caller keeps beside word j, requested before the search
template <class Fetch, class Round>
DEVINL void shared_word_rounds(const int* kw, int nk, const int* s_fw, int nW, int lane, Fetch fetch, Round round)
{
    for (int c = 0; c < nk; c += 64) {
        const bool in = c + lane < nk;
        const int j = in ? c + lane : nk - 1;
        const int w = kw[j];
        const auto x = fetch(j);
        const int pos = in ? sorted_find(s_fw, nW, w) : -1;
        round(__ballot(pos >= 0), w, pos, x);
    }
}

__global__ __launch_bounds__(256) void k_db_common(DbParams P, DbIn I, DbScratch S)
{
    extern __shared__ int s_fw[];                             // [nf] the frame's words, ascending
    const int f = blockIdx.x / P.nTiles, tile = blockIdx.x - f * P.nTiles, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nW = clamp_count(I.fN[f], P.nf);
    const int* fw = I.fWord + (size_t)f * P.nf;
    for (int i = tid; i < nW; i += 256) s_fw[i] = fw[i];
    __syncthreads();
    int waveMax = 0;
    for (int q = wave; q < kKfTile; q += 4) {
        const int k = tile * kKfTile + q;
        if (k >= P.nK) break;
        const int nk = kf_words(P, I, k, nW);
        const int* kw = I.kfWord + (size_t)k * P.nf;
        int cnt = 0, minw = 0;
        shared_word_rounds(kw, nk, s_fw, nW, lane, [](int) { return 0; }, [&](unsigned long long hit, int w, int, int) {
            if (hit) {
                if (cnt == 0) minw = __builtin_amdgcn_readlane(w, __ffsll((long long)hit) - 1);   // the keyframe's words ascend too
                cnt += __popcll(hit);
            }
        });
        if (lane == 0) { const size_t c = (size_t)f * P.nK + k; S.common[c] = cnt; S.minWord[c] = minw; }
        waveMax = max(waveMax, cnt);
    }
    if (lane == 0 && waveMax > 0) atomicMax(&S.maxCommon[f], waveMax);                            // :228-233
}

__global__ __launch_bounds__(256) void k_db_score(DbParams P, DbIn I, DbScratch S, float* __restrict__ scoresOut, int* __restrict__ commonOut)
{
    extern __shared__ double s_fv[];                          // [nf] the frame's values, then [nf] its words
    int* s_fw = (int*)(s_fv + P.nf);
    const int f = blockIdx.x / P.nTiles, tile = blockIdx.x - f * P.nTiles, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nW = clamp_count(I.fN[f], P.nf);
    const int* fw = I.fWord + (size_t)f * P.nf;
    const double* fv = I.fValue + (size_t)f * P.nf;
    for (int i = tid; i < nW; i += 256) { s_fw[i] = fw[i]; s_fv[i] = fv[i]; }
    __syncthreads();
    const int minCommon = min_common(S.maxCommon[f]);
    for (int q = wave; q < kKfTile; q += 4) {
        const int k = tile * kKfTile + q;
        if (k >= P.nK) break;
        const size_t c = (size_t)f * P.nK + k;
        const int common = S.common[c];
        unsigned bits = kNoScoreBits;
        if (scored(common, minCommon)) {
            const int nk = kf_words(P, I, k, nW);
            const int* kw = I.kfWord + (size_t)k * P.nf;
            const double* kv = I.kfValue + (size_t)k * P.nf;
            double score = 0.0;
            shared_word_rounds(kw, nk, s_fw, nW, lane, [&](int j) { return kv[j]; }, [&](unsigned long long hit, int, int pos, double wi) {
                double term = 0.0;
                if (pos >= 0) { const double vi = s_fv[pos]; term = fabs(vi - wi) - fabs(vi) - fabs(wi); }   // ScoringObject.cpp:41
                while (hit) {                                                                      // one `score +=` per common word, words ascending
                    const int b = __ffsll((long long)hit) - 1;
                    hit &= hit - 1;
                    score += readlane_f64(term, b);
                }
            });
            score = -score / 2.0;                                                                  // ScoringObject.cpp:65
            bits = __builtin_bit_cast(unsigned, (float)score);                                     // float si = ... (:249)
        }
        if (lane == 0) {
            S.score[c] = __builtin_bit_cast(float, bits);
            S.place[c] = kNoPlace;
            if (scoresOut) ((unsigned*)scoresOut)[c] = bits;
            if (commonOut) commonOut[c] = common;
        }
    }
}

DEVINL unsigned long long load_place(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void k_db_select(DbParams P, DbIn I, DbScratch S, int* __restrict__ cand, int* __restrict__ ncand, int2* __restrict__ pairs,
                                                  int* __restrict__ select)
{
    __shared__ unsigned long long s_keys[256];
    __shared__ int s_best, s_n;
    const int f = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)f * P.nK;
    const int* common = S.common + base;
    const float* score = S.score + base;
    const int minCommon = min_common(S.maxCommon[f]);
    if (tid == 0) { s_best = 0; s_n = 0; }
    __syncthreads();
    // ---- accumulate by covisibility (:262-287): one thread per scored keyframe
    int myBest = 0;                                           // the bits of the largest accScore above 0 (positive floats order like their bits)
    for (int k = tid; k < P.nK; k += 256) {
        if (!scored(common[k], minCommon)) continue;
        float bestScore = score[k], accScore = bestScore;
        int bestKF = k;
        for (int j = 0; j < kNeigh; j++) {
            const int nb = I.kfNeigh[(size_t)k * kNeigh + j];
            if ((unsigned)nb >= (unsigned)P.nK) continue;                                          // -1 padding, or garbage
            if (I.kfLive && I.kfLive[nb] == 0) continue;
            const int cn = common[nb];
            if (cn == 0) continue;                                                                 // mnRelocQuery != F->mnId (:273)
            // mRelocScore of the neighbour: this query's when it was scored (:250), else what it held before the call
            const float s = scored(cn, minCommon) ? score[nb] : (I.kfReloc ? I.kfReloc[nb] : 0.0f);
            accScore += s;
            if (s > bestScore) { bestKF = nb; bestScore = s; }
        }
        S.acc[base + k] = accScore; S.best[base + k] = bestKF;
        if (accScore > 0.0f) myBest = max(myBest, __builtin_bit_cast(int, accScore));
    }
    if (myBest > 0) atomicMax(&s_best, myBest);
    __syncthreads();
    const float minScoreToRetain = 0.75f * __builtin_bit_cast(float, s_best);                      // :290
    // ---- the place of every distinct pBestKF: the smallest order key among the retained entries that name it (:294-305)
    for (int k = tid; k < P.nK; k += 256) {
        if (!scored(common[k], minCommon)) continue;
        if (S.acc[base + k] > minScoreToRetain)
            atomicMin(&S.place[base + S.best[base + k]], ((unsigned long long)(unsigned)S.minWord[base + k] << 32) | (unsigned)k);
    }
    __syncthreads();
    for (int k = tid; k < P.nK; k += 256) {
        const unsigned long long key = load_place(&S.place[base + k]);
        if (key != kNoPlace) { const int pos = atomicAdd(&s_n, 1); S.list[base + pos] = k; S.listKey[base + pos] = key; }
    }
    __syncthreads();
    const int C = s_n;                                        // vpRelocCandidates.size()
    // ---- the keys are unique (an entry names one pBestKF): a candidate's rank among them is its position in the reference's vector
    int* candRow = cand + (size_t)f * P.maxCand;
    const size_t slot0 = (size_t)f * P.maxCand;
    const int frameRecord = I.fRecord[f];
    for (int i0 = 0; i0 < C; i0 += 256) {
        const bool mine = i0 + tid < C;
        const unsigned long long key = mine ? S.listKey[base + i0 + tid] : 0;
        int rank = 0;
        for (int j0 = 0; j0 < C; j0 += 256) {
            __syncthreads();
            s_keys[tid] = j0 + tid < C ? S.listKey[base + j0 + tid] : kNoPlace;
            __syncthreads();
            const int lim = min(256, C - j0);
            for (int j = 0; j < lim; j++) rank += s_keys[j] < key ? 1 : 0;
        }
        if (mine && rank < P.maxCand) {
            const int kf = S.list[base + i0 + tid];
            const int rec = I.kfRecord[kf];
            candRow[rank] = kf;
            pairs[slot0 + rank] = rec >= 0 ? make_int2(rec, frameRecord) : make_int2(-1, -1);
            select[slot0 + rank] = rec >= 0 ? 1 : 0;
        }
    }
    for (int j = C + tid; j < P.maxCand; j += 256) { candRow[j] = -1; pairs[slot0 + j] = make_int2(-1, -1); select[slot0 + j] = 0; }
    if (tid == 0) ncand[f] = C;
}

// the scratch of ivf_tracker_reloc_candidates for n (frame, keyframe) cells and `frames` frames: two sets, each with its cap
int db_grow(ivf_tracker* t, size_t n, int frames)
{
    DbScratch& S = t->db;
    if (n > S.cap) {                                                   // the eight cell arrays
        if (!t->replace({{S.common, n * sizeof(int)}, {S.minWord, n * sizeof(int)}, {S.score, n * sizeof(float)}, {S.acc, n * sizeof(float)},
                         {S.best, n * sizeof(int)}, {S.place, n * sizeof(unsigned long long)}, {S.list, n * sizeof(int)},
                         {S.listKey, n * sizeof(unsigned long long)}}))
            return fail(IVF_E_NO_DEVICE, "device allocation failed for %zu frame x keyframe cells", n);
        S.cap = n;
    }
    if (frames > S.frameCap) {                                         // maxCommon, per frame
        if (!t->replace({{S.maxCommon, (size_t)frames * sizeof(int)}})) return fail(IVF_E_NO_DEVICE, "device allocation failed for %zu frame x keyframe cells", n);
        S.frameCap = frames;
    }
    return IVF_OK;
}

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
    const DbIn I{d_kf_bow_word, d_kf_bow_value, d_kf_bow_n, d_kf_live, d_kf_neigh, d_kf_reloc_score, d_kf_record, d_bow_word, d_bow_value, d_bow_n, d_frame_record};
    HIPCHK(hipMemsetAsync(S.maxCommon, 0, (size_t)n_frames * sizeof(int), st));
    if (n_keyframes > 0) {
        const size_t nf = (size_t)P.nf;
        hipLaunchKernelGGL(k_db_common, dim3(P.nTiles * n_frames), dim3(256), nf * sizeof(int), st, P, I, S);
        hipLaunchKernelGGL(k_db_score, dim3(P.nTiles * n_frames), dim3(256), nf * (sizeof(double) + sizeof(int)), st, P, I, S, d_scores, d_common);
    }
    hipLaunchKernelGGL(k_db_select, dim3(n_frames), dim3(256), 0, st, P, I, S, d_cand, d_ncand, (int2*)d_pairs, d_select);
    return tracker_end(t, st);
}

}  // extern "C"
