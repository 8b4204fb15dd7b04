// ivf_db.h -- the one device text of the two queries of the keyframe database, shared by ivf_track_db.hip
// (KeyFrameDatabase::DetectRelocalizationCandidates, ORB/src/KeyFrameDatabase.cc:199-309) and ivf_track_loop.hip
// (KeyFrameDatabase::DetectLoopCandidates, :76-197, behind the minScore of LoopClosing::DetectLoop): the database and query arguments,
// which keyframes a query meets (kf_words), the 64-per-round word lookup (shared_word_rounds), the L1 score on it (l1_score_rounds),
// the thresholds (min_common, scored), the three kernels as templates on the query kind, the rank-by-key tail that writes the candidate
// rows, and the growth of the handle's DbScratch.  What the loop query does differently is said at each `kLoop`: the query's vector is a
// database row, keyframes at or past its visible limit, itself and its connected keyframes are in no inverted list, an entry needs
// si >= minScore, a neighbour counts only if it was scored in this query, and bestAccScore starts at minScore.
#pragma once
#include "ivf_tracker.h"

namespace ivf {

constexpr int kKfTile = 32;                        // keyframes per workgroup of k_db_common / k_db_score: 8 per wave
constexpr int kNeigh = 10;                         // GetBestCovisibilityKeyFrames(10) (KeyFrameDatabase.cc:151, :265)
constexpr unsigned kNoScoreBits = 0x7fc00000u;     // d_scores of a keyframe that was not scored (include/ivfront.h)
constexpr unsigned long long kNoPlace = ~0ull;
constexpr int kConnected = -1;                     // DbScratch::common of a (query, connected keyframe) cell before k_db_common<true> (k_loop_min_score)

DEVINL int clamp_count(int n, int nf) { return n < 0 ? 0 : (n > nf ? nf : n); }
// int minCommonWords = maxCommonWords*0.8f (KeyFrameDatabase.cc:120, :235): the product in float.  A double 0.8 gives the same integer,
// (4 * n) / 5, for every count a vector can hold (the two products part beyond 2^23 words; nfeatures <= 4096), so no scene can tell the
// two: tests/test_reloc_db_cpu.py and tests/test_loop_detect_cpu.py check the whole range instead.  A keyframe is scored when it shares
// MORE words than that (:129, :246), and only scored keyframes are accumulated (:159, :262)
DEVINL int min_common(int maxCommon) { return (int)((float)maxCommon * 0.8f); }
DEVINL bool scored(int common, int minCommon) { return common > minCommon; }

struct DbParams { int nf, nK, nF, maxCand, nTiles; };
struct DbIn {
    const int* kfWord; const double* kfValue; const int* kfN; const uint8_t* kfLive; const int* kfNeigh; const float* kfReloc; const int* kfRecord;
    const int* fWord; const double* fValue; const int* fN; const int* fRecord;                    // the lost frames (relocalization)
    const int* qKf; const int* qVisible; const int* qSelect; const float* minScore;              // the current keyframes (loop detection)
};
// frame / query f of a call: its vector (words ascending), which keyframes it can meet (k < visible, k != self), and whether it runs
// at all.  A loop query that does not run (select 0, or a keyframe index outside the database) reads and writes nothing but its d_ncand.
struct DbFrame { const int* word; const double* value; int nW, self, visible; bool run; };
constexpr int kNcandSkipped = -2, kNcandBadQuery = -1;
template <bool kLoop> DEVINL DbFrame db_frame(const DbParams& P, const DbIn& I, int f)
{
    if (!kLoop) return DbFrame{I.fWord + (size_t)f * P.nf, I.fValue + (size_t)f * P.nf, clamp_count(I.fN[f], P.nf), -1, P.nK, true};
    const int q = I.qKf[f];
    if ((I.qSelect && I.qSelect[f] == 0) || (unsigned)q >= (unsigned)P.nK) return DbFrame{nullptr, nullptr, 0, -1, 0, false};
    return DbFrame{I.kfWord + (size_t)q * P.nf, I.kfValue + (size_t)q * P.nf, clamp_count(I.kfN[q], P.nf), q, I.qVisible[f], true};
}
template <bool kLoop> DEVINL int db_skipped_ncand(const DbIn& I, int f) { return kLoop && I.qSelect && I.qSelect[f] == 0 ? kNcandSkipped : kNcandBadQuery; }

// the words keyframe k brings to a query: none when it was erased (it is in no inverted list), when the query's vector is empty, or (loop)
// when it was added to the database after the query or is the query itself
DEVINL int kf_words(const DbParams& P, const DbIn& I, int k, const DbFrame& F)
{
    if (F.nW == 0 || k >= F.visible || k == F.self || (I.kfLive && I.kfLive[k] == 0)) return 0;
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
// L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) of the frame in LDS (s_fw, s_fv) and the vector kw / kv [0 .. nk) by
// one wave, narrowed to float as every caller of mpVoc->score holds it: the terms of the common words added in lane order, i.e. in
// ascending word order, in f64.  No common word: -0.0 / 2.0 = -0.0f.
DEVINL float l1_score_rounds(const int* kw, const double* kv, int nk, const int* s_fw, const double* s_fv, int nW, int lane)
{
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
    return (float)score;                                                                   // float si = ... (KeyFrameDatabase.cc:133, :249)
}

// one workgroup per (frame, tile of 32 keyframes), the frame's words in LDS, one wave per keyframe: mnRelocWords / mnLoopWords, the
// smallest shared word, atomicMax -> maxCommonWords of the frame
template <bool kLoop> __global__ __launch_bounds__(256) void k_db_common(DbParams P, DbIn I, DbScratch S)
{
    extern __shared__ int s_fw[];                             // [nf] the frame's words, ascending
    const int f = blockIdx.x / P.nTiles, tile = blockIdx.x - f * P.nTiles, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DbFrame F = db_frame<kLoop>(P, I, f);
    if (!F.run) return;
    const int nW = F.nW;
    for (int i = tid; i < nW; i += 256) s_fw[i] = F.word[i];
    __syncthreads();
    int waveMax = 0;
    for (int q = wave; q < kKfTile; q += 4) {
        const int k = tile * kKfTile + q;
        if (k >= P.nK) break;
        const size_t c = (size_t)f * P.nK + k;
        // a connected keyframe never enters lKFsSharingWords (KeyFrameDatabase.cc:96) and never raises maxCommonWords
        const int nk = kLoop && S.common[c] == kConnected ? 0 : kf_words(P, I, k, F);
        const int* kw = I.kfWord + (size_t)k * P.nf;
        int cnt = 0, minw = 0;
        shared_word_rounds(kw, nk, s_fw, nW, lane, [](int) { return 0; }, [&](unsigned long long hit, int w, int, int) {
            if (hit) {
                if (cnt == 0) minw = __builtin_amdgcn_readlane(w, __ffsll((long long)hit) - 1);   // the keyframe's words ascend too
                cnt += __popcll(hit);
            }
        });
        if (lane == 0) { S.common[c] = cnt; S.minWord[c] = minw; }
        waveMax = max(waveMax, cnt);
    }
    if (lane == 0 && waveMax > 0) atomicMax(&S.maxCommon[f], waveMax);                            // :114-118, :228-233
}

// the same shape and the same rounds with the frame's values in LDS too
template <bool kLoop> __global__ __launch_bounds__(256) void k_db_score(DbParams P, DbIn I, DbScratch S, float* __restrict__ scoresOut, int* __restrict__ commonOut)
{
    extern __shared__ double s_fv[];                          // [nf] the frame's values, then [nf] its words
    int* s_fw = (int*)(s_fv + P.nf);
    const int f = blockIdx.x / P.nTiles, tile = blockIdx.x - f * P.nTiles, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DbFrame F = db_frame<kLoop>(P, I, f);
    if (!F.run) return;
    const int nW = F.nW;
    for (int i = tid; i < nW; i += 256) { s_fw[i] = F.word[i]; s_fv[i] = F.value[i]; }
    __syncthreads();
    const int minCommon = min_common(S.maxCommon[f]);
    for (int q = wave; q < kKfTile; q += 4) {
        const int k = tile * kKfTile + q;
        if (k >= P.nK) break;
        const size_t c = (size_t)f * P.nK + k;
        const int common = S.common[c];
        unsigned bits = kNoScoreBits;
        if (scored(common, minCommon))
            bits = __builtin_bit_cast(unsigned, l1_score_rounds(I.kfWord + (size_t)k * P.nf, I.kfValue + (size_t)k * P.nf, kf_words(P, I, k, F), s_fw, s_fv, nW, lane));
        if (lane == 0) {
            S.score[c] = __builtin_bit_cast(float, bits);
            S.place[c] = kNoPlace;
            if (scoresOut) ((unsigned*)scoresOut)[c] = bits;
            if (commonOut) commonOut[c] = common;
        }
    }
}

DEVINL unsigned long long load_place(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one workgroup per frame: covisibility accumulation per entry of lScoreAndMatch, bestAccScore, retention, the place of every distinct
// pBestKF (atomicMin of the retained entries' order keys), their ranks, the candidate rows and (pairs != nullptr) the pair / select rows
template <bool kLoop> __global__ __launch_bounds__(256) void k_db_select(DbParams P, DbIn I, DbScratch S, int* __restrict__ cand, int* __restrict__ ncand,
                                                                        int2* __restrict__ pairs, int* __restrict__ select)
{
    __shared__ unsigned long long s_keys[256];
    __shared__ int s_best, s_n;
    const int f = blockIdx.x, tid = threadIdx.x;
    if (kLoop && !db_frame<kLoop>(P, I, f).run) { if (tid == 0) ncand[f] = db_skipped_ncand<kLoop>(I, f); return; }
    const size_t base = (size_t)f * P.nK;
    const int* common = S.common + base;
    const float* score = S.score + base;
    const int minCommon = min_common(S.maxCommon[f]);
    // lScoreAndMatch holds a scored keyframe iff si >= minScore (:136); bestAccScore starts at minScore (:145) where relocalization
    // starts at 0 (:259).  The running maximum is kept as the bits of a float above 0 (they order like the floats); a start of +-0 is
    // bits 0, which every `>` below treats alike.
    const float minScore = kLoop ? I.minScore[f] : 0.0f;
    auto entry = [&](int k) { return scored(common[k], minCommon) && (!kLoop || score[k] >= minScore); };
    if (tid == 0) { s_best = minScore > 0.0f ? __builtin_bit_cast(int, minScore) : 0; s_n = 0; }
    __syncthreads();
    // ---- accumulate by covisibility (:148-173, :262-287): one thread per entry
    int myBest = 0;
    for (int k = tid; k < P.nK; k += 256) {
        if (!entry(k)) continue;
        float bestScore = score[k], accScore = bestScore;
        int bestKF = k;
        for (int j = 0; j < kNeigh; j++) {
            const int nb = I.kfNeigh[(size_t)k * kNeigh + j];
            if ((unsigned)nb >= (unsigned)P.nK) continue;                                          // -1 padding, or garbage
            if (I.kfLive && I.kfLive[nb] == 0) continue;
            const int cn = common[nb];
            float s;
            if (kLoop) {
                // mnLoopQuery == this query && mnLoopWords > minCommonWords (:159): only a keyframe scored in this query, whether or not
                // its own score reached minScore; mLoopScore of any other query is never read
                if (!scored(cn, minCommon)) continue;
                s = score[nb];
            } else {
                if (cn == 0) continue;                                                             // mnRelocQuery != F->mnId (:273)
                // mRelocScore of the neighbour: this query's when it was scored (:250), else what it held before the call
                s = scored(cn, minCommon) ? score[nb] : (I.kfReloc ? I.kfReloc[nb] : 0.0f);
            }
            accScore += s;
            if (s > bestScore) { bestKF = nb; bestScore = s; }
        }
        S.acc[base + k] = accScore; S.best[base + k] = bestKF;
        if (accScore > 0.0f) myBest = max(myBest, __builtin_bit_cast(int, accScore));
    }
    if (myBest > 0) atomicMax(&s_best, myBest);
    __syncthreads();
    const float minScoreToRetain = 0.75f * __builtin_bit_cast(float, s_best);                      // :176, :290
    // ---- the place of every distinct pBestKF: the smallest order key among the retained entries that name it (:182-193, :294-305)
    for (int k = tid; k < P.nK; k += 256) {
        if (!entry(k)) continue;
        if (S.acc[base + k] > minScoreToRetain)
            atomicMin(&S.place[base + S.best[base + k]], ((unsigned long long)(unsigned)S.minWord[base + k] << 32) | (unsigned)k);
    }
    __syncthreads();
    for (int k = tid; k < P.nK; k += 256) {
        const unsigned long long key = load_place(&S.place[base + k]);
        if (key != kNoPlace) { const int pos = atomicAdd(&s_n, 1); S.list[base + pos] = k; S.listKey[base + pos] = key; }
    }
    __syncthreads();
    const int C = s_n;                                        // vpRelocCandidates.size() / vpLoopCandidates.size()
    // ---- the keys are unique (an entry names one pBestKF): a candidate's rank among them is its position in the reference's vector
    int* candRow = cand + (size_t)f * P.maxCand;
    const size_t slot0 = (size_t)f * P.maxCand;
    const int frameRecord = pairs ? I.fRecord[f] : -1;
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
            candRow[rank] = kf;
            if (pairs) {
                const int rec = I.kfRecord[kf];
                pairs[slot0 + rank] = rec >= 0 ? make_int2(rec, frameRecord) : make_int2(-1, -1);
                select[slot0 + rank] = rec >= 0 ? 1 : 0;
            }
        }
    }
    for (int j = C + tid; j < P.maxCand; j += 256) {
        candRow[j] = -1;
        if (pairs) { pairs[slot0 + j] = make_int2(-1, -1); select[slot0 + j] = 0; }
    }
    if (tid == 0) ncand[f] = C;
}

// the handle's DbScratch for n (frame, keyframe) cells and `frames` frames: two sets, each with its cap
inline int db_grow(ivf_tracker* t, size_t n, int frames)
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

}  // namespace ivf
