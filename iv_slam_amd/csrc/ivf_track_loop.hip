// ivf_track_loop.hip -- LoopClosing::DetectLoop (ORB/src/LoopClosing.cc:108-234) for a batch of new keyframes, device-resident:
//   * ivf_tracker_loop_candidates: the reference score against the covisible keyframes (LoopClosing.cc:129-143) and
//     KeyFrameDatabase::DetectLoopCandidates (ORB/src/KeyFrameDatabase.cc:76-197) with L1Scoring::score, for many current keyframes
//     against one database given as flat arrays and the connected sets as a CSR;
//   * ivf_tracker_loop_consistency: the covisibility-consistency bookkeeping (LoopClosing.cc:148-230) over the queries of the call in
//     order, on mvConsistentGroups held in device memory by the caller; it writes mvpEnoughConsistentCandidates and the
//     (current keyframe record, candidate record) pair table ivf_tracker_search_by_bow_keyframes starts from.
// The database query is ivf_db.h's, shared with ivf_track_db.hip and instantiated here with kLoop = true; this file adds minScore and the
// groups.  Each query sees the database as it was when the reference ran it: keyframe k is in the inverted file of query q iff
// k < d_query_visible[q], it is live and it is not the query itself, so a batch of consecutive keyframes appended in order gives the
// reference's sequential result (mpKeyFrameDB->add(mpCurrentKF) after each DetectLoop) from one snapshot.
//
// Kernels (gfx950, wave = 64; no workgroup waits for another; every loop is bounded by nfeatures, n_keyframes, a connected row, 10,
// max_candidates, group_cap or member_cap):
//   k_loop_min_score    one workgroup per query, its vector in LDS, one wave per connected keyframe: marks the (query, connected) cell
//                       for k_db_common<true> and scores the live ones with l1_score_rounds; the minimum with `<` from 1.0f, as the first
//                       entry of the row that reaches it (the bits of -0.0f against 0.0f are the reference's)
//   k_db_common / k_db_score / k_db_select <true>    ivf_db.h
//   k_loop_consistency  ONE workgroup walks the queries in order (the reference's state is sequential); inside a query the candidates'
//                       groups are bitmaps over the keyframes (atomicOr: a set, whatever the row repeats), group against previous group
//                       is one wave testing the previous members' bits, and the new state is written from the bitmaps in ascending order
#include "ivf_db.h"

using namespace ivf;

namespace {

// a row of the connected CSR: empty when its offsets are negative, decreasing or past the array
DEVINL void conn_row(const int* __restrict__ connStart, int nConn, int k, int& s, int& e)
{
    s = connStart[k]; e = connStart[k + 1];
    if (s < 0 || e < s || e > nConn) s = e = 0;
}

__global__ __launch_bounds__(256) void k_loop_min_score(DbParams P, DbIn I, DbScratch S, const int* __restrict__ connStart, const int* __restrict__ conn,
                                                       int nConn, float* __restrict__ minScoreOut)
{
    extern __shared__ double s_fv[];                          // [nf] the query's values, then [nf] its words
    int* s_fw = (int*)(s_fv + P.nf);
    __shared__ float s_min[4];
    __shared__ int s_at[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DbFrame F = db_frame<true>(P, I, f);
    if (!F.run) return;
    const int nW = F.nW;
    for (int i = tid; i < nW; i += 256) { s_fw[i] = F.word[i]; s_fv[i] = F.value[i]; }
    __syncthreads();
    int s, e;
    conn_row(connStart, nConn, F.self, s, e);
    float best = 1.0f;                                        // float minScore = 1 (LoopClosing.cc:131)
    int at = 0x7fffffff;
    for (int j = s + wave; j < e; j += 4) {                   // the wave's entries, ascending
        const int c = conn[j];
        if ((unsigned)c >= (unsigned)P.nK) continue;
        if (lane == 0) S.common[(size_t)f * P.nK + c] = kConnected;                                // spConnectedKeyFrames.count(pKFi) (KeyFrameDatabase.cc:96)
        if (I.kfLive && I.kfLive[c] == 0) continue;                                                // isBad (:135); no visible limit: not a database lookup
        const float sc = l1_score_rounds(I.kfWord + (size_t)c * P.nf, I.kfValue + (size_t)c * P.nf, clamp_count(I.kfN[c], P.nf), s_fw, s_fv, nW, lane);
        if (sc < best) { best = sc; at = j; }                                                      // :141
    }
    if (lane == 0) { s_min[wave] = best; s_at[wave] = at; }
    __syncthreads();
    if (tid == 0) {
        // the sequential loop ends on the first entry of the row that holds the smallest value
        for (int w = 1; w < 4; w++)
            if (s_min[w] < best || (s_min[w] == best && s_at[w] < at)) { best = s_min[w]; at = s_at[w]; }
        minScoreOut[f] = best;
    }
}

// ---- the consistency groups ---------------------------------------------------------------------------------------------------------
struct GroupParams { int nK, nQ, maxCand, th, groupCap, memberCap, nConn, W; };
struct GroupIn { const int* kfRecord; const int* connStart; const int* conn; const int* qKf; const int* cand; const int* ncand; };
struct GroupState { int* member; int* size; int* count; int* nGroups; };
struct GroupOut { int* enough; int* nenough; int2* pairs; int* select; int* status; };
// the call's carving of LoopScratch: bits [maxCand][W], gsize / flags / entries [maxCand], off [maxCand + 1], cons [maxCand][groupCap],
// first / newSrc / newCount [groupCap]
struct GroupWork { unsigned* bits; int *gsize, *flags, *entries, *off, *cons, *first, *newSrc, *newCount; };
size_t group_work_words(const GroupParams& P) { return (size_t)P.maxCand * ((size_t)P.W + 4 + (size_t)P.groupCap) + 1 + 3 * (size_t)P.groupCap; }
GroupWork group_work(unsigned* buf, const GroupParams& P)
{
    GroupWork K;
    const size_t mc = (size_t)P.maxCand, gc = (size_t)P.groupCap;
    K.bits = buf; buf += mc * (size_t)P.W;
    K.gsize = (int*)buf; buf += mc;
    K.flags = (int*)buf; buf += mc;
    K.entries = (int*)buf; buf += mc;
    K.off = (int*)buf; buf += mc + 1;
    K.cons = (int*)buf; buf += mc * gc;
    K.first = (int*)buf; buf += gc;
    K.newSrc = (int*)buf; buf += gc;
    K.newCount = (int*)buf;
    return K;
}
constexpr int kAny = 1, kEnough = 2;                          // GroupWork::flags: bConsistentForSomeGroup, bEnoughConsistent

DEVINL int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
DEVINL int wave_scan_inclusive(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o); if (lane >= o) v += u; }
    return v;
}
// row e of the state cleared: what a row at or past n_groups holds
DEVINL void group_clear(const GroupParams& P, const GroupState& G, int e, int lane)
{
    for (int j = lane; j < P.memberCap; j += 64) G.member[(size_t)e * P.memberCap + j] = -1;
    if (lane == 0) { G.size[e] = 0; G.count[e] = 0; }
}

__global__ __launch_bounds__(256) void k_loop_consistency(GroupParams P, GroupIn I, GroupState G, GroupOut O, GroupWork K)
{
    __shared__ int s_over, s_sticky, s_nNew, s_nEnough;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_sticky = 0;
    for (int q = 0; q < P.nQ; q++) {
        __syncthreads();                                      // the state and the flags of the previous query are written
        const int nc = I.ncand[q];
        const int nOld = min(max(G.nGroups[0], 0), P.groupCap);
        const bool sticky = s_sticky != 0;
        const int* candRow = I.cand + (size_t)q * P.maxCand;
        const bool run = !sticky && nc > 0 && nc <= P.maxCand;
        __syncthreads();                                      // everybody has read s_sticky and n_groups
        if (tid == 0) { s_over = sticky || nc > P.maxCand ? 1 : 0; s_nNew = 0; s_nEnough = 0; }
        if (run) {
            // ---- spCandidateGroup = GetConnectedKeyFrames() + the candidate (:169-170), as a bitmap over the keyframes
            for (size_t i = tid; i < (size_t)nc * P.W; i += 256) K.bits[i] = 0;
            __syncthreads();
            for (int i = wave; i < nc; i += 4) {
                const int c = candRow[i];
                if ((unsigned)c >= (unsigned)P.nK) continue;
                unsigned* bits = K.bits + (size_t)i * P.W;
                if (lane == 0) atomicOr(&bits[c >> 5], 1u << (c & 31));
                int s, e;
                conn_row(I.connStart, P.nConn, c, s, e);
                for (int j = s + lane; j < e; j += 64) {
                    const int m = I.conn[j];
                    if ((unsigned)m < (unsigned)P.nK) atomicOr(&bits[m >> 5], 1u << (m & 31));
                }
            }
            __syncthreads();
            for (int i = wave; i < nc; i += 4) {
                int n = 0;
                for (int w = lane; w < P.W; w += 64) n += __popc(K.bits[(size_t)i * P.W + w]);
                n = wave_sum(n);
                if (lane == 0) { K.gsize[i] = n; if (n > P.memberCap) s_over = 1; }
            }
            // ---- bConsistent of (candidate i, previous group g): they share a keyframe (:176-187)
            for (int p = wave; p < nc * nOld; p += 4) {
                const int i = p / nOld, g = p - i * nOld;
                const int sz = min(max(G.size[g], 0), P.memberCap);
                bool hit = false;
                for (int j = lane; j < sz; j += 64) {
                    const int m = G.member[(size_t)g * P.memberCap + j];
                    if ((unsigned)m < (unsigned)P.nK && ((K.bits[(size_t)i * P.W + (m >> 5)] >> (m & 31)) & 1u)) hit = true;
                }
                const bool any = __ballot(hit) != 0;
                if (lane == 0) K.cons[(size_t)i * P.groupCap + g] = any ? 1 : 0;
            }
            __syncthreads();
            // ---- vbConsistentGroup (:193-198): a previous group is continued by the FIRST candidate consistent with it
            for (int g = tid; g < nOld; g += 256) {
                int first = -1;
                for (int i = 0; i < nc; i++) if (K.cons[(size_t)i * P.groupCap + g]) { first = i; break; }
                K.first[g] = first;
            }
            __syncthreads();
            for (int i = tid; i < nc; i += 256) {
                int flags = 0, cnt = 0;
                for (int g = 0; g < nOld; g++) {
                    if (K.cons[(size_t)i * P.groupCap + g]) flags |= kAny | (G.count[g] + 1 >= P.th ? kEnough : 0);   // :199, whether or not g was flagged
                    cnt += K.first[g] == i ? 1 : 0;
                }
                K.flags[i] = flags;
                K.entries[i] = (flags & kAny) ? cnt : 1;      // :208-212: consistent with no previous group -> one entry, counter 0
            }
            __syncthreads();
            if (tid == 0) {
                long long o = 0;
                int ne = 0;
                for (int i = 0; i < nc; i++) { K.off[i] = (int)min(o, (long long)P.groupCap); o += K.entries[i]; ne += (K.flags[i] & kEnough) ? 1 : 0; }
                if (o > P.groupCap) s_over = 1;
                s_nNew = (int)min(o, (long long)P.groupCap); s_nEnough = ne;
            }
        }
        __syncthreads();
        const bool over = s_over != 0;
        const int nEnough = run && !over ? s_nEnough : 0;
        if (run && !over) {
            // ---- vCurrentConsistentGroups in the order of the pushes: candidate by candidate, the continued groups ascending
            for (int g = tid; g < nOld; g += 256) {
                const int i = K.first[g];
                if (i < 0) continue;
                int r = 0;
                for (int g2 = 0; g2 < g; g2++) r += K.first[g2] == i ? 1 : 0;
                const int e = K.off[i] + r;
                K.newSrc[e] = i; K.newCount[e] = G.count[g] + 1;                                   // nCurrentConsistency (:191-192)
            }
            for (int i = tid; i < nc; i += 256)
                if (!(K.flags[i] & kAny)) { K.newSrc[K.off[i]] = i; K.newCount[K.off[i]] = 0; }
            __syncthreads();
            // ---- mvConsistentGroups = vCurrentConsistentGroups (:216): a wave per entry, the members ascending out of the bitmap
            const int nNew = s_nNew;
            for (int e = wave; e < nNew; e += 4) {
                const int i = K.newSrc[e];
                int* row = G.member + (size_t)e * P.memberCap;
                int base = 0;
                for (int w0 = 0; w0 < P.W; w0 += 64) {
                    const int w = w0 + lane;
                    unsigned word = w < P.W ? K.bits[(size_t)i * P.W + w] : 0u;
                    const int pc = __popc(word), incl = wave_scan_inclusive(pc, lane);
                    int pos = base + incl - pc;
                    while (word) { const int b = __ffs((int)word) - 1; word &= word - 1; row[pos++] = w * 32 + b; }   // pos < gsize <= memberCap
                    base += __shfl(incl, 63);
                }
                for (int j = base + lane; j < P.memberCap; j += 64) row[j] = -1;
                if (lane == 0) { G.size[e] = K.gsize[i]; G.count[e] = K.newCount[e]; }
            }
            for (int e = nNew + wave; e < nOld; e += 4) group_clear(P, G, e, lane);
            if (tid == 0) G.nGroups[0] = nNew;
        } else if (nc == 0 && !over) {
            for (int e = wave; e < nOld; e += 4) group_clear(P, G, e, lane);                       // mvConsistentGroups.clear() (:152)
            if (tid == 0) G.nGroups[0] = 0;
        }
        // ---- mvpEnoughConsistentCandidates in candidate order and the (KF1, KF2) = (current keyframe, candidate) pair table
        const size_t slot0 = (size_t)q * P.maxCand;
        if (nEnough > 0) {
            const int qk = I.qKf[q];
            const int rq = (unsigned)qk < (unsigned)P.nK ? I.kfRecord[qk] : -1;
            for (int i = tid; i < nc; i += 256) {
                if (!(K.flags[i] & kEnough)) continue;
                int pos = 0;
                for (int i2 = 0; i2 < i; i2++) pos += (K.flags[i2] & kEnough) ? 1 : 0;
                const int c = candRow[i];
                const int rc = (unsigned)c < (unsigned)P.nK ? I.kfRecord[c] : -1;
                const bool ok = rq >= 0 && rc >= 0;
                O.enough[slot0 + pos] = c;
                O.pairs[slot0 + pos] = ok ? make_int2(rq, rc) : make_int2(-1, -1);
                O.select[slot0 + pos] = ok ? 1 : 0;
            }
        }
        for (int j = nEnough + tid; j < P.maxCand; j += 256) { O.enough[slot0 + j] = -1; O.pairs[slot0 + j] = make_int2(-1, -1); O.select[slot0 + j] = 0; }
        if (tid == 0) { O.nenough[q] = nEnough; O.status[q] = over ? 1 : 0; if (over) s_sticky = 1; }
    }
}

int loop_scratch_grow(ivf_tracker* t, size_t words)
{
    LoopScratch& L = t->loop;
    if (words <= L.cap) return IVF_OK;
    if (!t->replace({{L.buf, words * sizeof(unsigned)}})) return fail(IVF_E_NO_DEVICE, "device allocation failed for %zu words of group scratch", words);
    L.cap = words;
    return IVF_OK;
}

}  // namespace

extern "C" {

int ivf_tracker_loop_candidates(ivf_tracker* t, const int32_t* d_kf_bow_word, const double* d_kf_bow_value, const int32_t* d_kf_bow_n,
                                const uint8_t* d_kf_live, const int32_t* d_kf_neigh, int n_keyframes, const int32_t* d_conn_start,
                                const int32_t* d_conn, int n_conn, const int32_t* d_query_kf, const int32_t* d_query_visible,
                                const int32_t* d_query_select, int n_queries, int max_candidates, float* d_min_score, int32_t* d_cand,
                                int32_t* d_ncand, float* d_scores, int32_t* d_common, void* hip_stream)
{
    if (!t) return fail(IVF_E_INVALID, "null argument");
    if (n_keyframes < 0 || n_queries < 0 || n_conn < 0)
        return fail(IVF_E_INVALID, "n_keyframes %d / n_queries %d / n_conn %d is negative", n_keyframes, n_queries, n_conn);
    if (max_candidates < 1) return fail(IVF_E_INVALID, "max_candidates must be >= 1");
    if (n_keyframes > 0 && (!d_kf_bow_word || !d_kf_bow_value || !d_kf_bow_n || !d_kf_neigh || !d_conn_start)) return fail(IVF_E_INVALID, "null database array");
    if (n_conn > 0 && !d_conn) return fail(IVF_E_INVALID, "null connected array of %d entries", n_conn);
    if (n_queries > 0 && (!d_query_kf || !d_query_visible || !d_min_score || !d_cand || !d_ncand)) return fail(IVF_E_INVALID, "null query or output array");
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = tracker_begin(t, false, 0, 0, 0, st);
    if (rc != IVF_OK) return rc;
    if (n_queries == 0) return IVF_OK;
    DbParams P;
    P.nf = t->P.nf; P.nK = n_keyframes; P.nF = n_queries; P.maxCand = max_candidates; P.nTiles = (n_keyframes + kKfTile - 1) / kKfTile;
    if ((long long)P.nTiles * n_queries > 0x7fffffffLL) return fail(IVF_E_CAPACITY, "%d queries x %d keyframes exceed one launch", n_queries, n_keyframes);
    const size_t cells = (size_t)n_queries * (size_t)n_keyframes;
    rc = db_grow(t, cells, n_queries);
    if (rc != IVF_OK) return rc;
    const DbScratch S = t->db;
    const DbIn I{d_kf_bow_word, d_kf_bow_value, d_kf_bow_n, d_kf_live, d_kf_neigh, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                 d_query_kf, d_query_visible, d_query_select, d_min_score};
    HIPCHK(hipMemsetAsync(S.maxCommon, 0, (size_t)n_queries * sizeof(int), st));
    if (n_keyframes > 0) {
        const size_t nf = (size_t)P.nf;
        HIPCHK(hipMemsetAsync(S.common, 0, cells * sizeof(int), st));                              // no cell is kConnected before k_loop_min_score says so
        hipLaunchKernelGGL(k_loop_min_score, dim3(n_queries), dim3(256), nf * (sizeof(double) + sizeof(int)), st, P, I, S, d_conn_start, d_conn, n_conn, d_min_score);
        hipLaunchKernelGGL(k_db_common<true>, dim3(P.nTiles * n_queries), dim3(256), nf * sizeof(int), st, P, I, S);
        hipLaunchKernelGGL(k_db_score<true>, dim3(P.nTiles * n_queries), dim3(256), nf * (sizeof(double) + sizeof(int)), st, P, I, S, d_scores, d_common);
    }
    hipLaunchKernelGGL(k_db_select<true>, dim3(n_queries), dim3(256), 0, st, P, I, S, d_cand, d_ncand, (int2*)nullptr, (int*)nullptr);
    return tracker_end(t, st);
}

int ivf_tracker_loop_consistency(ivf_tracker* t, const int32_t* d_kf_record, int n_keyframes, const int32_t* d_conn_start, const int32_t* d_conn,
                                 int n_conn, const int32_t* d_query_kf, int n_queries, const int32_t* d_cand, const int32_t* d_ncand,
                                 int max_candidates, int th, int32_t* d_group_member, int32_t* d_group_size, int32_t* d_group_count,
                                 int32_t* d_n_groups, int group_cap, int member_cap, int32_t* d_enough, int32_t* d_nenough, int32_t* d_pairs,
                                 int32_t* d_select, int32_t* d_status, void* hip_stream)
{
    if (!t) return fail(IVF_E_INVALID, "null argument");
    if (n_keyframes < 0 || n_queries < 0 || n_conn < 0)
        return fail(IVF_E_INVALID, "n_keyframes %d / n_queries %d / n_conn %d is negative", n_keyframes, n_queries, n_conn);
    if (max_candidates < 1 || group_cap < 1 || member_cap < 1)
        return fail(IVF_E_INVALID, "max_candidates %d / group_cap %d / member_cap %d must be >= 1", max_candidates, group_cap, member_cap);
    if (n_keyframes > 0 && (!d_kf_record || !d_conn_start)) return fail(IVF_E_INVALID, "null database array");
    if (n_conn > 0 && !d_conn) return fail(IVF_E_INVALID, "null connected array of %d entries", n_conn);
    if (!d_group_member || !d_group_size || !d_group_count || !d_n_groups) return fail(IVF_E_INVALID, "null state array");
    if (n_queries > 0 && (!d_query_kf || !d_cand || !d_ncand || !d_enough || !d_nenough || !d_pairs || !d_select || !d_status))
        return fail(IVF_E_INVALID, "null query or output array");
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = tracker_begin(t, false, 0, 0, 0, st);
    if (rc != IVF_OK) return rc;
    if (n_queries == 0) return IVF_OK;
    GroupParams P;
    P.nK = n_keyframes; P.nQ = n_queries; P.maxCand = max_candidates; P.th = th; P.groupCap = group_cap; P.memberCap = member_cap; P.nConn = n_conn;
    P.W = (n_keyframes + 31) / 32;
    if ((long long)max_candidates * group_cap > 0x7fffffffLL) return fail(IVF_E_CAPACITY, "%d candidates x %d groups exceed the scratch's index", max_candidates, group_cap);
    rc = loop_scratch_grow(t, group_work_words(P));
    if (rc != IVF_OK) return rc;
    const GroupIn I{d_kf_record, d_conn_start, d_conn, d_query_kf, d_cand, d_ncand};
    const GroupState G{d_group_member, d_group_size, d_group_count, d_n_groups};
    const GroupOut O{d_enough, d_nenough, (int2*)d_pairs, d_select, d_status};
    hipLaunchKernelGGL(k_loop_consistency, dim3(1), dim3(256), 0, st, P, I, G, O, group_work(t->loop.buf, P));
    return tracker_end(t, st);
}

}  // extern "C"
