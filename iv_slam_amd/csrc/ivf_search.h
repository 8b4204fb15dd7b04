// ivf_search.h -- the device text the projection searches of the batched tracker share: ivf_track.hip (TrackWithMotionModel),
// ivf_track_local.hip (SearchLocalPoints) and ivf_track_reloc.hip (Relocalization); ivf_track_bow.hip takes the liveness test,
// ivf_track_sim3.hip (SearchBySim3, which is not greedy) the liveness test, the range-and-level gate and the first minimum of a window.  Every
// other search is prepare -> window -> greedy walk; what makes them differ -- what a dead pair writes, the depth and viewing-angle tests, the
// radius, the level range, best / second best, the admission against the live state -- stays with each kernel.
#pragma once
#include "ivf_tracker.h"

namespace ivf {

// a pair takes part when the mask (null: none) selects it and both record indices lie inside the block of this call
DEVINL bool pair_live(int nRecords, const int2 pr, const int* __restrict__ select, int p)
{
    return (!select || select[p] != 0) && rec_ok(nRecords, pr.x) && rec_ok(nRecords, pr.y);
}

// ---- the ORDERED candidate list of one query, built by one wave from grid_walk's steps: the position of this lane's candidate in
// window order (meaningful where ok); `total` advances by the step's candidates
DEVINL int list_ordinal(bool ok, int lane, int& total)
{
    const unsigned long long m = __ballot(ok);
    const int pos = total + __popcll(m & ((1ull << lane) - 1ull));
    total += __popcll(m);
    return pos;
}
// ... and the append: the first kListCap are listed, `total` counts them all (> kListCap: the greedy walk goes through the window again)
DEVINL void list_append(bool ok, int lane, int& total, unsigned* __restrict__ L, unsigned entry)
{
    const int pos = list_ordinal(ok, lane, total);
    if (ok && pos < kListCap) L[pos] = entry;
}

// the stereo-consistency gate (ORBmatcher.cc:91-96, :1451-1457): a keypoint with a right coordinate u2 is out when that lies further
// than the window radius from the projected one
DEVINL bool ur_admits(float u2, float qur, float r) { return !(u2 > 0 && fabsf(qur - u2) > r); }

// ---- the gates of a projected map point (Frame::isInFrustum, Frame.cc:579-590; ORBmatcher.cc:1556-1572)
DEVINL bool in_image(const TrackParams& P, float u, float v) { return !(u < P.minX || u > P.maxX) && !(v < P.minY || v > P.maxY); }
// false: dist outside [0.8 min_distance, 1.2 max_distance] (MapPoint.cc:378-388); else lv = MapPoint::PredictScale.  The one statement of
// the range and the level, whatever distance a search measures: |P - Ow| below, the camera-frame norm in SearchBySim3 (ivf_track_sim3.hip)
DEVINL bool range_level(const TrackParams& P, const ivf_local_point& mp, float dist, int& lv)
{
    const float minD = 0.8f * mp.min_distance, maxD = 1.2f * mp.max_distance;
    if (dist < minD || dist > maxD) return false;
    lv = predict_scale(P, mp.max_distance, dist);
    return true;
}
// dist = cv::norm(P - Ow), then range_level
DEVINL bool point_range_level(const TrackParams& P, const ivf_local_point& mp, const float* Ow, float& dist, int& lv)
{
    const float PO[3] = {mp.pos[0] - Ow[0], mp.pos[1] - Ow[1], mp.pos[2] - Ow[2]};
    const double n2 = (double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2];
    dist = (float)sqrt(n2);
    return range_level(P, mp, dist, lv);
}

// ---- the FIRST minimum of up to 64 candidates in list order, one per lane (live: the lane holds one; admits(idx): the search's own
// occupancy / stereo test of current keypoint idx against the LIVE state, asked for live lanes only): the reference's
// `dist < bestDist` is strict, so among equal distances the earliest wins = the minimum of (distance << 6 | lane).  The running
// (bestDist, bestIdx) -- start them at 256, -1 -- is replaced only by a strictly smaller distance: called once per step of a window
// walk it keeps the earlier step's candidate, so within a step the key orders by (distance, window position), across steps the
// strict `<` does, and the result is the first minimum in window order whether the candidates came as one list or as many steps.
template <class Admit>
DEVINL void first_min_in_list(bool live, int dist, int idx, int lane, Admit admits, int& bestDist, int& bestIdx)
{
    unsigned key = 0xffffffffu;
    if (live) key = admits(idx) ? ((unsigned)dist << 6) | (unsigned)lane : 0xffffffffu;   // the key is ready when the state's answer arrives
    const unsigned best = wave_min_u32(key);
    if (best != 0xffffffffu && (int)(best >> 6) < bestDist) {
        bestDist = (int)(best >> 6);
        bestIdx = __builtin_amdgcn_readlane(idx, (int)(best & 63));
    }
}
// ... of a window that overflowed its list: walked again, 64 candidates at a time, on the search's own level range [minL, maxL]
template <class IDX, class Admit>
DEVINL void first_min_in_window(const GridGeom G, const ivf_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                const int* __restrict__ start, const IDX* __restrict__ idx, float u, float v, float r, int minL, int maxL,
                                const uint4 qa, const uint4 qb, int lane, Admit admits, int& bestDist, int& bestIdx)
{
    grid_walk(G, kps, desc, start, idx, u, v, r, minL, maxL, qa, qb, lane,
              [&](bool ok, int i2, int d) { first_min_in_list(ok, d, i2, lane, admits, bestDist, bestIdx); });
}

// ---- the LAST minimum of a list of up to 4096 candidates, the other rule: SearchForTriangulation's `dist>bestDist` (ORBmatcher.cc:744)
// lets a later equal distance replace the earlier one, so the candidate kept is the minimum of (distance << 12 | 4095 - position) over
// the candidates that pass every gate; a lane folds its strides with min(), the wave with wave_min_u32
DEVINL unsigned last_min_key(bool ok, int dist, int pos) { return ok ? ((unsigned)dist << 12) | (unsigned)(4095 - pos) : 0xffffffffu; }
DEVINL int last_min_position(unsigned best) { return 4095 - (int)(best & 4095u); }

// ---- the greedy walk over the lists of queries 0 .. n - 1 (C [n] counts, Lp [n][kListCap] entries), in order, by one wave:
// body(i, cnt, ent, aux) runs for every query with cnt != 0; ent = this lane's entry of the list, aux() = loadAux(i), one 4-byte word
// per query that travels with the lists (a call, so that a body which needs it on one path only pays for it there).  The next group of
// kPrefetch lists is in flight while this one is walked.
// r06: the loads of a group are UNCONDITIONAL (index clamped into the arrays) and their results are touched for the first time when the
// group is processed; validity is re-derived from the indices there.  The form `valid ? load : 0` per field, then `cur = nxt` compiled
// to branches around the loads with PHI copies behind them and register moves at the loop's end: an s_waitcnt vmcnt(0) at the head of
// EVERY group, i.e. no prefetch at all.  The two register sets alternate by unrolling, not by copies.
template <class LoadAux, class Body>
DEVINL void walk_lists_prefetched(int n, const int* __restrict__ C, const unsigned* __restrict__ Lp, int lane, LoadAux loadAux, Body body)
{
    using Aux = decltype(loadAux(0));
    struct Grp { unsigned ent[kPrefetch]; int myCnt; Aux myAux; };
    const int nc = max(n - 1, 0);
    auto load_group = [&](int g0, Grp& g) {
        const int gi = min(g0 + (lane & (kPrefetch - 1)), nc);
        g.myCnt = C[gi]; g.myAux = loadAux(gi);
#pragma unroll
        for (int k = 0; k < kPrefetch; k++) g.ent[k] = Lp[(size_t)min(g0 + k, nc) * kListCap + lane];
    };
    auto process = [&](const int g0, const Grp& grp) {
        const int myCnt = (g0 + (lane & (kPrefetch - 1))) < n ? grp.myCnt : 0;
#pragma unroll
        for (int k = 0; k < kPrefetch; k++) {
            const int cnt = __builtin_amdgcn_readlane(myCnt, k);
            if (g0 + k >= n || cnt == 0) continue;                                      // an empty window; an invalid query lists nothing
            body(g0 + k, cnt, grp.ent[k], [&] { return readlane_b32(grp.myAux, k); });
        }
    };
    if (n > 0) {
        Grp gA, gB;
        load_group(0, gA);
        for (int g0 = 0; g0 < n; g0 += 2 * kPrefetch) {
            load_group(g0 + kPrefetch, gB); process(g0, gA);
            if (g0 + kPrefetch < n) { load_group(g0 + 2 * kPrefetch, gA); process(g0 + kPrefetch, gB); }
        }
    }
}

}  // namespace ivf
