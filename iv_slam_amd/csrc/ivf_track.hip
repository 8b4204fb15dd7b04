// ivf_track.hip -- the batched tracker handle (struct ivf_tracker, ivf_tracker.h: create, destroy, the begin / end every entry point
// shares) and its first search, ivf_tracker_run: the consumer of the descriptor all-gather.
//
// For every (last, cur) pair of gather records -- what ivf_frontend_pack_gather_block writes and the RCCL all-gather
// delivers -- one launch sequence runs the matcher part of Tracking::TrackWithMotionModel (ORB/src/Tracking.cc:1303-1330):
//   * UpdateLastFrame's "visual odometry" points (Tracking.cc:1256-1300): the last frame's stereo points, optionally only the
//     close ones + the 100 closest, un-projected with Frame::UnprojectStereo (ORB/src/Frame.cc:958-972);
//   * ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono = false) (ORB/src/ORBmatcher.cc:1372-1518): projection
//     into the current frame (:1399-1427), Frame::GetFeaturesInArea windows on the 64x48 grid (ORB/src/Frame.cc:615-668) with the
//     forward / backward / +-1 octave range (:1429-1434), the ORDER-DEPENDENT greedy assignment in last-keypoint order with the
//     stereo-consistency check (:1444-1472), the 30-bin rotation histogram and ComputeThreeMaxima (:1475-1511, :1654-1695);
//   * the retry with the wider window when fewer than 20 matches were found (Tracking.cc:1320-1330).
// Nothing crosses PCIe: records, poses, the per-pair grids, candidate lists and results stay in HBM.
//
// Kernels (all hand-written for gfx950; wave = 64):
//   k_track_prepare  one workgroup per frame pair: AssignFeaturesToGrid of the current record (stable counting sort in LDS),
//                    pose algebra in double (cv::gemm semantics), depth ranking, projection -> query table
//   k_track_window   one wave per (frame pair, last keypoint): window + octave / box filters + Hamming distances,
//                    ballot-compacted, ORDERED candidate list of <= 64 packed entries (index | distance << 16)
//   k_track_greedy   one wave per frame pair walks the queries in order: assignment state, uRight and angles of the current
//                    frame live in LDS, the lists of the next 16 queries are in registers before they are needed, the first
//                    minimum is a DPP row_shr / row_bcast reduction of (distance << 6 | list position); histogram in one VGPR
//                    (lane = bin).  Queries whose window overflowed the list are re-walked in place against the live state
//                    (first_min_in_window, ivf_search.h).
// The grid itself -- grid_build / grid_walk, here with unsigned short indices (nfeatures <= 4096) -- is ivf_grid.h's, shared with the
// device-resident ivf_frame (ivf_match.hip); the pieces the three projection searches repeat (liveness, the ordered list, the gates, the
// first minimum) are ivf_search.h's.  This file also owns the candidate scratch all three use, one call at a time
// (tracker_grow_queries), their shared argument checks (search_args_ok) and those of the two RANSAC solvers (ransac_args_ok).
#include "ivf_search.h"
#include <climits>
#include <cstring>

using namespace ivf;

namespace {

// k_track_greedy's candidate admission against the live state in LDS (ORBmatcher.cc:1447-1457): current keypoint i2 is out when a point
// with observations holds it, or when its right coordinate fails ur_admits
constexpr int kNoBlock = 0x10000;                 // flag on an assignment made by a point without observations: it does not block (:1447-1449)
DEVINL bool track_admits(const int* s_assign, const float* s_ur, int i2, float qur, float radius)
{
    const int a = s_assign[i2];
    const bool held = a >= 0 && !(a & kNoBlock);
    const bool ur = ur_admits(s_ur[i2], qur, radius);
    return !held && ur;
}

// ------------------------------------------------------------------------------------------------
// k_track_prepare: one workgroup per frame pair
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_prepare(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                      const float* __restrict__ poses, const uint8_t* __restrict__ pointFlags,
                                                      int* __restrict__ gStart, unsigned short* __restrict__ gIdx,
                                                      Query* __restrict__ queries, int* __restrict__ retryFlag)
{
    __shared__ int cnt[kGC * kGR];
    __shared__ int part[256];
    __shared__ int blk[256];
    __shared__ float s_z[kMaxTrackFeatures];
    __shared__ int s_nStereo, s_nClose;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, nullptr, p)) { if (tid == 0) retryFlag[p] = 0; return; }
    const uint8_t* recL = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recC = records + (size_t)pr.y * P.recBytes;
    const int nL = rec_count(recL, P.nf), nC = rec_count(recC, P.nf);
    if (tid == 0) { retryFlag[p] = 0; s_nStereo = 0; s_nClose = 0; }

    // ---- Frame::AssignFeaturesToGrid of the current frame (Frame.cc:415-430)
    const ivf_keypoint* kc = rec_kps(recC);
    grid_build(geom_of(P), kc, nC, gStart + (size_t)p * (kGC * kGR + 1), gIdx + (size_t)p * P.nf, cnt, part, blk, tid);

    // ---- poses of THIS pair: {LastFrame.mTcw, CurrentFrame.mTcw = mVelocity * mLastFrame.mTcw (Tracking.cc:1311)}, row-major 3x4;
    //      identity when none are given (zero-motion prior)
    float Rl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tl[3] = {0, 0, 0}, Rc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tc[3] = {0, 0, 0};
    if (poses) { load_pose(poses + (size_t)p * 24, Rl, tl); load_pose(poses + (size_t)p * 24 + 12, Rc, tc); }
    float twc[3], tlc[3];
    neg_rt_mul(Rc, tc, twc);                                                          // ORBmatcher.cc:1385
    mul_add(Rl, twc, tl, tlc);                                                        // tlc = Rlw * twc + tlw (:1390)
    const bool bForward = tlc[2] > P.b, bBackward = -tlc[2] > P.b;                    // :1392-1393 (bMono = false)

    // ---- which last-frame keypoints carry a point
    const float* zL = rec_depth(recL, P.nf);
    const ivf_keypoint* kl = rec_kps(recL);
    const uint8_t* fl = pointFlags ? pointFlags + (size_t)pr.x * P.nf : nullptr;
    const bool rule = !fl && P.thDepth > 0.0f;
    int rStop = INT_MAX;
    if (rule) {
        // UpdateLastFrame (Tracking.cc:1256-1300): points sorted by (depth, index); all close ones, and at least the 100 closest:
        // the walk stops after the first entry with z > mThDepth once more than 100 have been taken
        int ns = 0, nc = 0;
        for (int i = tid; i < nL; i += 256) { const float z = zL[i]; s_z[i] = z; if (z > 0) { ns++; if (!(z > P.thDepth)) nc++; } }
        atomicAdd(&s_nStereo, ns); atomicAdd(&s_nClose, nc);
        __syncthreads();
        rStop = max(s_nClose, 100);
    }
    Query* Q = queries + (size_t)p * P.nf;
    for (int i = tid; i < nL; i += 256) {
        const float z = zL[i];
        bool has = z > 0;
        int blocks = P.defaultBlocks;
        if (fl) { has = has && (fl[i] & 1); blocks = (fl[i] >> 1) & 1; }
        if (has && rule) {
            int rank = 0;
            for (int j = 0; j < nL; j++) { const float zj = s_z[j]; rank += (zj > 0 && (zj < z || (zj == z && j < i))) ? 1 : 0; }
            has = rank <= rStop;
            blocks = 0;                                                               // new "visual odometry" points have no observations
        }
        Query q; q.u = 0; q.v = 0; q.ur = 0; q.bits = 0;
        if (has) {
            const ivf_keypoint kp = kl[i];
            float xw[3], xc[3];
            unproject_stereo(P, Rl, tl, kp, z, xw);                                   // the pose terms in it do not depend on i
            mul_add(Rc, xw, tc, xc);                                                  // ORBmatcher.cc:1405
            const float invzc = (float)(1.0 / (double)xc[2]);                         // :1409
            if (!(invzc < 0)) {
                const float u = P.fx * xc[0] * invzc + P.cx, v = P.fy * xc[1] * invzc + P.cy;
                if (in_image(P, u, v)) {
                    const int o = kp.octave;
                    int lo, hi;
                    if (bForward) { lo = o; hi = -1; } else if (bBackward) { lo = 0; hi = o; } else { lo = o - 1; hi = o + 1; }   // :1429-1434
                    q.u = u; q.v = v; q.ur = u - P.bf * invzc;                         // :1453
                    q.bits = pack_bits(o, lo, hi, 1, blocks);
                }
            }
        }
        Q[i] = q;
    }
}

// ------------------------------------------------------------------------------------------------
// k_track_window: one wave per (frame pair, last keypoint)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_window(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                     const int* __restrict__ gStart, const unsigned short* __restrict__ gIdx,
                                                     const Query* __restrict__ queries, float th, const int* __restrict__ retryFlag,
                                                     int onlyFlagged, int* __restrict__ count, unsigned* __restrict__ lists)
{
    const int p = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (onlyFlagged && !retryFlag[p]) return;
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, nullptr, p)) return;
    const uint8_t* recL = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recC = records + (size_t)pr.y * P.recBytes;
    const int nL = rec_count(recL, P.nf);
    if (i >= nL) return;
    const Query q = queries[(size_t)p * P.nf + i];
    int total = 0;
    if ((q.bits >> 24) & 1) {
        const int o = q.bits & 0xff, lo = (int)((q.bits >> 8) & 0xff) - 1, hi = (int)((q.bits >> 16) & 0xff) - 1;
        const float r = th * P.scale[o];                                              // :1427
        const uint4* qd = (const uint4*)(rec_desc(recL, P.nf) + (size_t)i * 32);       // pMP->GetDescriptor(): the point's one observation
        const uint4 qa = qd[0], qb = qd[1];
        unsigned* L = lists + ((size_t)p * P.nf + i) * kListCap;
        grid_walk(geom_of(P), rec_kps(recC), rec_desc(recC, P.nf), gStart + (size_t)p * (kGC * kGR + 1), gIdx + (size_t)p * P.nf,
                  q.u, q.v, r, lo, hi, qa, qb, lane, [&](bool ok, int i2, int d) { list_append(ok, lane, total, L, (unsigned)i2 | ((unsigned)d << 16)); });
    }
    if (lane == 0) count[(size_t)p * P.nf + i] = total;
}

// ------------------------------------------------------------------------------------------------
// k_track_greedy: one wave per frame pair
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_track_greedy(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                    const int* __restrict__ gStart, const unsigned short* __restrict__ gIdx,
                                                    const Query* __restrict__ queries, float th, int* __restrict__ retryFlag,
                                                    int onlyFlagged, int retryBelow, const int* __restrict__ count,
                                                    const unsigned* __restrict__ lists, float* __restrict__ pointQuality,
                                                    float* __restrict__ keyQuality, int* __restrict__ assignOut,
                                                    int* __restrict__ nmatchesOut)
{
    extern __shared__ int s_mem[];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (onlyFlagged && !retryFlag[p]) return;
    int* s_assign = s_mem;                                    // [nf] CurrentFrame.mvpMapPoints as last-keypoint indices
    float* s_ur = (float*)(s_mem + P.nf);                     // [nf] CurrentFrame.mvuRight
    float* s_ang = (float*)(s_mem + 2 * P.nf);                // [nf] CurrentFrame.mvKeysUn[].angle
    unsigned* s_match = (unsigned*)(s_mem + 3 * P.nf);        // [nf] matches in the order they were made: idx2 | bin << 16
    const int2 pr = pairs[p];
    if (!pair_live(P.nRecords, pr, nullptr, p)) {
        for (int i = lane; i < P.nf; i += 64) assignOut[(size_t)p * P.nf + i] = -1;
        if (lane == 0) { nmatchesOut[p] = -1; retryFlag[p] = 0; }
        return;
    }
    const uint8_t* recL = records + (size_t)pr.x * P.recBytes;
    const uint8_t* recC = records + (size_t)pr.y * P.recBytes;
    const int nL = rec_count(recL, P.nf), nC = rec_count(recC, P.nf);
    const ivf_keypoint* kc = rec_kps(recC);
    const ivf_keypoint* kl = rec_kps(recL);
    const float* urC = rec_uright(recC, P.nf);
    for (int i = lane; i < nC; i += 64) { s_assign[i] = -1; s_ur[i] = urC[i]; s_ang[i] = kc[i].angle; }
    __shared__ float s_scale[kMaxLevels];
    __shared__ int s_hist[32];                                // rotHist[b].size()
    int* s_claim = s_mem + 4 * P.nf;                          // [nf] scratch of the group commit
    if (lane < kMaxLevels) s_scale[lane] = P.scale[lane];
    if (lane < 32) s_hist[lane] = 0;
    wave_sync_lds();
    const Query* Q = queries + (size_t)p * P.nf;
    const int* C = count + (size_t)p * P.nf;
    const unsigned* Lp = lists + (size_t)p * P.nf * kListCap;

    // r04: a group of 16 queries is evaluated SPECULATIVELY against the live state -- four queries per pass, one per DPP row of 16 lanes
    // (a window holds a handful of candidates: radius 7 px x the octave's scale) -- and the longest PREFIX of the group in which no two
    // matched queries chose the same keypoint is committed at once: for those queries the state they would have seen in turn differs
    // from the evaluated one only by assignments to keypoints none of them chose, so the speculative first minimum is the serial one.
    // The first query that lost a keypoint to an earlier one of the group (the same corner found at two pyramid levels: common) starts
    // the next round, evaluated against the state that now holds the winner; a query whose list is longer than a row is walked alone
    // against the live state (64 entries per step, or its window again when the list overflowed).  The next group's lists are
    // requested before the current group is evaluated.
    // r06: the loads of a group are UNCONDITIONAL (index clamped into the frame's own arrays) and their results are touched for the first time when the group is
    // evaluated, two groups later; validity is re-derived from the indices there.  The r04 form -- `valid ? load : 0` per field, then `cur = nxt; nxt = nx2` --
    // compiled to branches around the loads with PHI copies behind them and register moves of the newest group at the loop's end: an s_waitcnt vmcnt(0) at the
    // head of EVERY group, i.e. no prefetch at all (phase timers: 56 % of the walk was that wait).  The three groups now rotate by unrolling, not by copies.
    struct Grp { unsigned ent[4]; int cnt[4]; float2 urb[4]; int myCnt; Query myQ; float myAng; };
    const int nLc = max(nL - 1, 0);
    auto load_group = [&](int g0, Grp& g) {
        const int gi = min(g0 + (lane & (kPrefetch - 1)), nLc);
        g.myCnt = C[gi]; g.myQ = Q[gi]; g.myAng = kl[gi].angle;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int qi = min(g0 + 4 * m + (lane >> 4), nLc);
            g.ent[m] = Lp[(size_t)qi * kListCap + (lane & 15)];
            g.cnt[m] = C[qi];
            g.urb[m] = *(const float2*)&Q[qi].ur;
        }
    };
    int nmAcc = 0, nMatchAcc = 0;
    auto process = [&](const int g0, const Grp& cur) {
        int nm = nmAcc, nMatch = nMatchAcc;
        int fb = -1;                              // lane k: the keypoint query k matched (-1: none)
        const int kEnd = min(kPrefetch, nL - g0);
        const int myCnt = (g0 + (lane & (kPrefetch - 1))) < nL ? cur.myCnt : 0;
        const Query myQ = cur.myQ;
        const unsigned bigMask = (unsigned)__ballot(lane < kEnd && myCnt > 16);
        int kstart = 0;
        while (kstart < kEnd) {
            if ((bigMask >> kstart) & 1u) {
                // ---- a long list: this query alone, against the live state
                const int k = kstart, i = g0 + k;
                const int cnt = __builtin_amdgcn_readlane(myCnt, k);
                const float qur = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myQ.ur), k));
                const unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)myQ.bits, k);
                const float radius = th * P.scale[bits & 0xff];
                int bestDist = 256, bestIdx2 = -1;
                auto admits = [&](int i2) { return track_admits(s_assign, s_ur, i2, qur, radius); };
                if (cnt <= kListCap) {
                    const unsigned e = Lp[(size_t)i * kListCap + lane];
                    const int i2 = e & 0xffff, d = e >> 16;
                    first_min_in_list(lane < cnt, d, i2, lane, admits, bestDist, bestIdx2);  // first minimum in list order (:1463-1467)
                } else {
                    // the window overflowed its list: walk it again, against the live assignment state
                    const float qu = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myQ.u), k));
                    const float qv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myQ.v), k));
                    const int lo = (int)((bits >> 8) & 0xff) - 1, hi = (int)((bits >> 16) & 0xff) - 1;
                    const uint4* qd = (const uint4*)(rec_desc(recL, P.nf) + (size_t)i * 32);
                    first_min_in_window(geom_of(P), kc, rec_desc(recC, P.nf), gStart + (size_t)p * (kGC * kGR + 1), gIdx + (size_t)p * P.nf, qu, qv, radius,
                                        lo, hi, qd[0], qd[1], lane, admits, bestDist, bestIdx2);
                }
                if (bestIdx2 >= 0 && bestDist <= 100) {                                     // TH_HIGH (:1469)
                    if (lane == 0) s_assign[bestIdx2] = ((bits >> 25) & 1u) ? i : (i | kNoBlock);
                    if (lane == k) fb = bestIdx2;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                kstart++;
                continue;
            }
            // ---- speculative pass: row r of pass m = query 4 m + r
            unsigned key[4]; int i2m[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const unsigned e = cur.ent[m];
                const int i2 = e & 0xffff, d = e >> 16, pos = lane & 15;
                const int cntm = (g0 + 4 * m + (lane >> 4)) < nL ? cur.cnt[m] : 0;
                const float urm = cur.urb[m].x; const unsigned bitsm = __builtin_bit_cast(unsigned, cur.urb[m].y);
                bool ok = pos < cntm && cntm <= 16;
                if (ok) ok = track_admits(s_assign, s_ur, i2, urm, th * s_scale[bitsm & 0xff]);
                i2m[m] = i2;
                key[m] = ok ? ((unsigned)d << 6) | (unsigned)pos : 0xffffffffu;
            }
#pragma unroll
            for (int m = 0; m < 4; m++) key[m] = wave_row_min_u32(key[m]);   // minimum of each row of 16 lanes, in its lane 15
            // lane k < 16 collects query k's result (row k & 3 of pass k >> 2)
            const int src = 16 * (lane & 3) + 15, mSel = (lane >> 2) & 3;
            unsigned kq[4];
#pragma unroll
            for (int m = 0; m < 4; m++) kq[m] = (unsigned)__builtin_amdgcn_ds_bpermute(4 * src, (int)key[m]);
            const unsigned best = mSel == 0 ? kq[0] : (mSel == 1 ? kq[1] : (mSel == 2 ? kq[2] : kq[3]));
            const int src2 = 16 * (lane & 3) + (int)(best & 15u);
            int iq[4];
#pragma unroll
            for (int m = 0; m < 4; m++) iq[m] = __builtin_amdgcn_ds_bpermute(4 * src2, i2m[m]);
            const int bi = mSel == 0 ? iq[0] : (mSel == 1 ? iq[1] : (mSel == 2 ? iq[2] : iq[3]));
            const bool mine = lane >= kstart && lane < kEnd;
            const bool mt = mine && myCnt != 0 && myCnt <= 16 && best != 0xffffffffu && (int)(best >> 6) <= 100;      // TH_HIGH (:1469)
            // the lowest query of every set that chose the same keypoint wins it; the others are losers
            if (mt) s_claim[bi] = 64;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (mt) atomicMin(&s_claim[bi], lane);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const bool loser = mt && s_claim[bi] != lane;
            const unsigned stopMask = ((unsigned)__ballot(loser) | bigMask) & (0xffffffffu << kstart);
            const int kstop = stopMask ? min(__ffs((int)stopMask) - 1, kEnd) : kEnd;
            if (mt && lane < kstop) {
                s_assign[bi] = ((myQ.bits >> 25) & 1u) ? (g0 + lane) : ((g0 + lane) | kNoBlock);
                fb = bi;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            kstart = kstop;
        }
        // ---- the group's matches: rotation bins (:1476-1484) and the match list, lane k = query k
        {
            const bool mt = fb >= 0;
            int bin = 0;
            if (P.checkOri && mt) bin = rot_bin(cur.myAng - s_ang[fb]);
            const unsigned long long mm = __ballot(mt);
            if (mt) s_match[nMatch + __popcll(mm & ((1ull << lane) - 1ull))] = (unsigned)fb | ((unsigned)bin << 16);
            if (P.checkOri && mt) atomicAdd(&s_hist[bin], 1);
            const int n = __popcll(mm);
            nMatch += n; nm += n;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        nmAcc = nm; nMatchAcc = nMatch;
    };
    {
        Grp gA, gB, gC;                       // two groups ahead: a group's work (~1 us) is shorter than a trip to L2 / HBM under load
        load_group(0, gA);
        load_group(kPrefetch, gB);
        for (int g0 = 0; g0 < nL; g0 += 3 * kPrefetch) {
            load_group(g0 + 2 * kPrefetch, gC); process(g0, gA);
            if (g0 + kPrefetch < nL) { load_group(g0 + 3 * kPrefetch, gA); process(g0 + kPrefetch, gB); }
            if (g0 + 2 * kPrefetch < nL) { load_group(g0 + 4 * kPrefetch, gB); process(g0 + 2 * kPrefetch, gC); }
        }
    }
    int nm = nmAcc, nMatch = nMatchAcc;
    // ---- rotation consistency: ComputeThreeMaxima (:1654-1695) over the 30 bins, matches of every other bin are taken back
    if (P.checkOri) {
        const RotKeep keep = rot_three_maxima(s_hist);
        __builtin_amdgcn_wave_barrier();
        int removed = 0;
        for (int m0 = 0; m0 < nMatch; m0 += 64) {
            const int m = m0 + lane;
            bool rm = false;
            if (m < nMatch) {
                const unsigned e = s_match[m];
                const int bin = (int)(e >> 16);
                rm = !keep.keeps(bin);
                if (rm) s_assign[e & 0xffff] = -1;                                      // :1504
            }
            removed += __popcll(__ballot(rm));
        }
        nm -= removed;
        wave_sync_lds();
    }
    int* out = assignOut + (size_t)p * P.nf;
    for (int i = lane; i < P.nf; i += 64) { const int a = i < nC ? s_assign[i] : -1; out[i] = a < 0 ? -1 : (a & 0xffff); }
    // ORBmatcher::UpdateQualityScores(CurrentFrame) at the end of EVERY SearchByProjection call (:1513-1515; the retry is a second call
    // and updates again from what the first left)
    if (pointQuality && keyQuality) update_quality_scores(s_assign, nC, 0xffff, lane, 64, pointQuality + (size_t)p * P.nf, keyQuality + (size_t)p * P.nf);
    if (lane == 0) {
        nmatchesOut[p] = nm;
        retryFlag[p] = (!onlyFlagged && nm < retryBelow) ? 1 : 0;                      // Tracking.cc:1320
    }
}

}  // namespace

// ---- the handle ------------------------------------------------------------------------------------------------------------
namespace ivf {
int tracker_begin(ivf_tracker* t, bool reads_records, size_t record_bytes, int n_records, int n_items, hipStream_t st)
{
    if (!t) return fail(IVF_E_INVALID, "null argument");
    if (reads_records && record_bytes != t->P.recBytes)
        return fail(IVF_E_INVALID, "record_bytes %zu: records of %d features are %zu bytes", record_bytes, t->P.nf, t->P.recBytes);
    if (reads_records && n_records < 1) return fail(IVF_E_INVALID, "n_records must be >= 1");
    if (n_items < 0 || n_items > t->cfg.max_pairs) return fail(IVF_E_INVALID, "%d frames / pairs outside [0,%d]", n_items, t->cfg.max_pairs);
    HIPCHK(hipSetDevice(t->cfg.device_id));
    if (t->ran) HIPCHK(hipStreamWaitEvent(st, t->evDone, 0));                          // the handle runs one call at a time
    return IVF_OK;
}
int tracker_begin_with_vocabulary(ivf_tracker* t, const ivf_vocabulary* voc, VocabularyView* V, bool reads_records, size_t record_bytes, int n_records,
                                  int n_items, hipStream_t st)
{
    int rc = vocabulary_view(voc, V);
    if (rc == IVF_OK) rc = tracker_begin(t, reads_records, record_bytes, n_records, n_items, st);
    if (rc != IVF_OK) return rc;
    if (V->device != t->cfg.device_id)
        return fail(IVF_E_INVALID, "the vocabulary lives on device %d, the tracker on device %d", V->device, t->cfg.device_id);
    return IVF_OK;
}
int tracker_end(ivf_tracker* t, hipStream_t st)
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(t->evDone, st));
    t->ran = true;
    return IVF_OK;
}
int search_args_ok(const ivf_tracker* t, const void* records, const void* items, bool has_points, const void* points, const void* assign,
                   const void* nmatches, int n_items, const float* point_quality, const float* key_quality)
{
    if (!t || !records || !items || (has_points && !points) || !assign || !nmatches) return fail(IVF_E_INVALID, "null argument");
    if (((size_t)records & 15) != 0 || ((size_t)points & 15) != 0)
        return fail(IVF_E_INVALID, has_points ? "the record block and the point array must be 16-byte aligned" : "the record block must be 16-byte aligned");
    if (n_items != 0 && (point_quality == nullptr) != (key_quality == nullptr))
        return fail(IVF_E_INVALID, "d_point_quality and d_key_quality come together");
    return IVF_OK;
}
int ransac_args_ok(const void* records, int max_iterations, double probability, int min_inliers)
{
    if (((size_t)records & 15) != 0) return fail(IVF_E_INVALID, "the record block must be 16-byte aligned");
    if (max_iterations < 1 || max_iterations > kRansacMaxIterations) return fail(IVF_E_INVALID, "max_iterations %d outside [1,%d]", max_iterations, kRansacMaxIterations);
    if (!(probability > 0.0 && probability < 1.0)) return fail(IVF_E_INVALID, "probability %g outside (0,1)", probability);
    if (min_inliers < 0) return fail(IVF_E_INVALID, "min_inliers must be >= 0");
    return IVF_OK;
}
int tracker_grow_queries(ivf_tracker* t, int cap)
{
    if (cap <= t->queryCap) return IVF_OK;
    const size_t n = (size_t)t->cfg.max_pairs * (size_t)cap;
    if (!t->replace({{t->dQ, n * sizeof(Query)}, {t->dLRad, n * sizeof(float)}, {t->dCount, n * sizeof(int)}, {t->dLists, n * kListCap * sizeof(unsigned)}}))
        return fail(IVF_E_NO_DEVICE, "device allocation failed for %d frames x %d queries", t->cfg.max_pairs, cap);
    t->queryCap = cap;
    return IVF_OK;
}
int tracker_grow_grids(ivf_tracker* t, int per_pair)
{
    if (per_pair <= t->gridCap) return IVF_OK;
    const size_t n = (size_t)t->cfg.max_pairs * (size_t)per_pair;
    if (!t->replace({{t->dStart, n * (kGC * kGR + 1) * sizeof(int)}, {t->dIdx, n * (size_t)t->cfg.nfeatures * sizeof(unsigned short)}}))
        return fail(IVF_E_NO_DEVICE, "device allocation failed for %d pairs x %d grids", t->cfg.max_pairs, per_pair);
    t->gridCap = per_pair;
    return IVF_OK;
}
}  // namespace ivf

extern "C" {

size_t ivf_track_record_bytes(int nfeatures)
{
    return nfeatures < 0 ? 0 : 16 + (size_t)nfeatures * (sizeof(ivf_keypoint) + 32 + 2 * sizeof(float));
}

void ivf_tracker_destroy(ivf_tracker* t)
{
    if (!t) return;
    (void)hipSetDevice(t->cfg.device_id);
    scratch_free_all(ivf_tracker::Device{t}, t->owned);
    if (t->evDone) (void)hipEventDestroy(t->evDone);
    delete t;
}

int ivf_tracker_create(const ivf_track_config* cfg, ivf_tracker** out)
{
    if (!cfg || !out) return fail(IVF_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->nfeatures < 1 || cfg->nfeatures > kMaxTrackFeatures)
        return fail(IVF_E_CAPACITY, "the batched tracker keeps 20 bytes of state per keypoint in LDS: nfeatures %d outside [1,%d]", cfg->nfeatures, kMaxTrackFeatures);
    if (cfg->nlevels < 1 || cfg->nlevels > kMaxLevels) return fail(IVF_E_INVALID, "nlevels %d outside [1,%d]", cfg->nlevels, kMaxLevels);
    if (cfg->max_pairs < 1) return fail(IVF_E_INVALID, "max_pairs must be >= 1");
    if (!(cfg->bounds.max_x > cfg->bounds.min_x) || !(cfg->bounds.max_y > cfg->bounds.min_y)) return fail(IVF_E_INVALID, "empty image bounds");
    if (!(cfg->fx > 0) || !(cfg->fy > 0) || !(cfg->bf > 0) || !(cfg->b > 0)) return fail(IVF_E_INVALID, "fx, fy, bf and b must be positive");
    if (!(cfg->th > 0) || (cfg->retry_below > 0 && !(cfg->th_retry > 0))) return fail(IVF_E_INVALID, "th (and th_retry with retry_below > 0) must be positive");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(IVF_E_NO_DEVICE, "no HIP device available; libivfront has no CPU path");
    if (cfg->device_id < 0 || cfg->device_id >= n) return fail(IVF_E_INVALID, "device_id %d outside [0,%d)", cfg->device_id, n);
    HIPCHK(hipSetDevice(cfg->device_id));
    ivf_tracker* t = new ivf_tracker();
    t->cfg = *cfg;
    TrackParams& P = t->P;
    memset(&P, 0, sizeof P);
    P.nf = cfg->nfeatures; P.nlevels = cfg->nlevels;
    for (int l = 0; l < kMaxLevels; l++) P.scale[l] = l < cfg->nlevels ? cfg->scale_factors[l] : 1.0f;
    P.fx = cfg->fx; P.fy = cfg->fy; P.cx = cfg->cx; P.cy = cfg->cy; P.invfx = 1.0f / cfg->fx; P.invfy = 1.0f / cfg->fy;   // Frame.cc:203-204
    P.bf = cfg->bf; P.b = cfg->b;
    const GridGeom G = grid_geom(cfg->bounds);
    P.minX = G.minX; P.minY = G.minY; P.maxX = cfg->bounds.max_x; P.maxY = cfg->bounds.max_y; P.invW = G.invW; P.invH = G.invH;
    P.thDepth = cfg->th_depth; P.checkOri = cfg->check_orientation ? 1 : 0; P.defaultBlocks = cfg->points_block ? 1 : 0;
    P.recBytes = ivf_track_record_bytes(cfg->nfeatures);
    P.logScale = cfg->nlevels > 1 ? logf(cfg->scale_factors[1]) : 1.0f;             // mfLogScaleFactor = log(mfScaleFactor) (Frame.cc:106): logf
    const size_t np = (size_t)cfg->max_pairs, nf = (size_t)cfg->nfeatures;
    t->ldsBytes = nf * 20;
    if (tracker_grow_grids(t, 1) != IVF_OK || tracker_grow_queries(t, cfg->nfeatures) != IVF_OK ||
        !t->replace({{t->dRetry, np * sizeof(int)}, {t->bow.nodeKey, 2 * np * nf * sizeof(int)}, {t->bow.fvNode, 2 * np * nf * sizeof(int)},
                     {t->bow.fvStart, 2 * np * (nf + 1) * sizeof(int)}, {t->bow.fvIdx, 2 * np * nf * sizeof(int)}, {t->bow.fvN, 2 * np * sizeof(int)}})) {
        ivf_tracker_destroy(t);
        return fail(IVF_E_NO_DEVICE, "device allocation failed for a tracker of %d pairs x %d features", cfg->max_pairs, cfg->nfeatures);
    }
    if (hipEventCreateWithFlags(&t->evDone, hipEventDisableTiming) != hipSuccess) {
        ivf_tracker_destroy(t);
        return fail(IVF_E_NO_DEVICE, "event creation failed");
    }
    if (t->ldsBytes > 48 * 1024 &&
        hipFuncSetAttribute((const void*)k_track_greedy, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->ldsBytes) != hipSuccess) {
        ivf_tracker_destroy(t);
        return fail(IVF_E_NO_DEVICE, "cannot reserve %zu bytes of LDS for k_track_greedy", t->ldsBytes);
    }
    *out = t;
    return IVF_OK;
}

int ivf_tracker_run(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                    const float* d_poses, const uint8_t* d_point_flags, float* d_point_quality, float* d_key_quality,
                    int32_t* d_assign, int32_t* d_nmatches, void* hip_stream)
{
    const int ra = search_args_ok(t, d_records, d_pairs, false, nullptr, d_assign, d_nmatches, n_pairs, d_point_quality, d_key_quality);
    if (ra != IVF_OK || n_pairs == 0) return ra;
    hipStream_t st = (hipStream_t)hip_stream;
    // the per-pair grids, query tables and candidate lists are scratch of the HANDLE: a run enqueued on another stream than the
    // previous one queues behind it (use one tracker per stream to let runs overlap)
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_pairs, st);
    if (rc != IVF_OK) return rc;
    TrackParams P = t->P;
    P.nRecords = n_records;
    const int2* pairs = (const int2*)d_pairs;
    hipLaunchKernelGGL(k_track_prepare, dim3(n_pairs), dim3(256), 0, st, P, d_records, pairs, d_poses, d_point_flags, t->dStart, t->dIdx, t->dQ, t->dRetry);
    const dim3 wg((P.nf + 3) / 4, n_pairs);
    for (int pass = 0; pass < (t->cfg.retry_below > 0 ? 2 : 1); pass++) {
        const float th = pass ? t->cfg.th_retry : t->cfg.th;
        hipLaunchKernelGGL(k_track_window, wg, dim3(256), 0, st, P, d_records, pairs, t->dStart, t->dIdx, t->dQ, th, t->dRetry, pass, t->dCount, t->dLists);
        hipLaunchKernelGGL(k_track_greedy, dim3(n_pairs), dim3(64), t->ldsBytes, st, P, d_records, pairs, t->dStart, t->dIdx, t->dQ, th, t->dRetry, pass,
                           t->cfg.retry_below, t->dCount, t->dLists, d_point_quality, d_key_quality, d_assign, d_nmatches);
    }
    return tracker_end(t, st);
}

}  // extern "C"
