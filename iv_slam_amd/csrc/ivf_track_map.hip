// ivf_track_map.hip -- ivf_tracker_update_local_map: Tracking::UpdateLocalMap (ORB/src/Tracking.cc:2134-2270), batched and
// device-resident, between the first PoseOptimization and SearchLocalPoints.  The map is an ivf_map_view of flat tables
// (include/ivfront.h); nothing crosses PCIe and no pointer graph is walked on the host.  Every index read from a table goes through
// in_range / csr_row before it is used: the house rule of rec_ok.
//
// Kernels (gfx950, wave = 64; one workgroup per frame, no workgroup waits for another; every loop is bounded by nfeatures, a table's
// length, n_keyframes, 10 or the hash set's size):
//   k_map_keyframes  UpdateLocalKeyFrames (:2168-2270).  The vote row (one int per keyframe, in LDS up to kVoteLds keyframes, else in the
//                    handle's scratch) collects the observations of the held points with integer atomics; compact_ordered (ivf_solve.h)
//                    lists the voted, live keyframes in kf_order and marks them in the row; pKFmax is an atomicMax of (count, ~position).
//                    The expansion is serial by definition -- every append changes the test of the next -- so one wave walks it:
//                    lanes over the candidates of one step (ten neighbours, 64 children at a time), a ballot for the first eligible.
//   k_map_points     UpdateLocalPoints (:2143-2166) as a stable unique: pass 1 puts every candidate (list position a, keypoint j) into
//                    the frame's hash set, atomicMin of the position a * nfeatures + j per point; pass 2 walks the candidates in
//                    order again, keeps the one whose position the set holds (compact_ordered) and copies the kept records as five
//                    16-byte pieces.  A small LDS set of the points the frame holds gives flags bit 0; the same loop writes d_occupied.
#include "ivf_solve.h"

using namespace ivf;

namespace {

static_assert(sizeof(ivf_local_point) == 80, "ivf_local_point is copied as five 16-byte pieces");

constexpr int kVoteLds = 8192;                     // keyframes whose vote row fits LDS (32 KB); more: the row lives in the handle's scratch
constexpr int kNeigh = 10;                         // GetBestCovisibilityKeyFrames(10) (Tracking.cc:2225)
constexpr int kLocalLimit = 80;                    // :2221
constexpr int kExpandCap = 96;                     // the list the expansion can see: <= 80 before a step, <= 3 appended by it
constexpr int kVoteMark = 0x40000000;              // vote row: the keyframe is in the list (mnTrackReferenceForFrame == mnId)
constexpr unsigned kEmpty = 0xffffffffu;           // hash set: an unclaimed slot / no position yet (what the memset leaves)

struct MapParams { int nf, maxLK, maxPts, voteInLds, hashLog2; };

DEVINL bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }
// row i of a CSR over a table of `len` entries: false (an empty row) unless 0 <= begin <= end <= len
DEVINL bool csr_row(const int* __restrict__ off, int i, int len, int& b, int& e)
{
    b = off[i]; e = off[i + 1];
    return b >= 0 && b <= e && e <= len;
}
DEVINL bool kf_live(const ivf_map_view& M, int k) { return !M.kf_live || M.kf_live[k] != 0; }
// the vote row is LDS or HBM behind one generic pointer, written with atomics: every access goes to where the atomics act
DEVINL int row_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEVINL void row_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEVINL unsigned set_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void k_map_keyframes(MapParams P, ivf_map_view M, int* __restrict__ framePoints, int* voteScratch,
                                                      int* __restrict__ localKf, int* __restrict__ nLocalKf, int* __restrict__ refKf)
{
    extern __shared__ int s_vote[];                           // [n_keyframes] when P.voteInLds
    __shared__ int s_wcnt[4];
    __shared__ int s_any, s_size;
    __shared__ unsigned long long s_best;
    __shared__ int s_list[kExpandCap];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nK = M.n_keyframes, nP = M.n_points;
    int* vote = P.voteInLds ? s_vote : voteScratch + (size_t)f * nK;
    int* fp = framePoints + (size_t)f * P.nf;
    int* row = localKf + (size_t)f * P.maxLK;
    for (int k = tid; k < nK; k += 256) row_store(&vote[k], 0);
    if (tid == 0) { s_any = 0; s_best = 0ull; }
    __syncthreads();
    // ---- each map point votes for the keyframes in which it has been observed (:2170-2185)
    bool any = false;
    for (int i = tid; i < P.nf; i += 256) {
        const int m = fp[i];
        if (!in_range(m, nP)) continue;
        if (M.points[m].flags & 1) { fp[i] = -1; continue; }                                       // :2182
        int b, e;
        if (!csr_row(M.obs_offsets, m, M.n_obs, b, e)) continue;
        for (int o = b; o < e; o++) {
            const int k = M.obs_kf[o];
            if (in_range(k, nK)) { atomicAdd(&vote[k], 1); any = true; }
        }
    }
    if (any) atomicOr(&s_any, 1);
    __syncthreads();
    if (!s_any) {                                                                                  // keyframeCounter.empty(): return (:2187)
        if (tid == 0) { const int n = nLocalKf[f]; nLocalKf[f] = n < 0 ? 0 : (n > P.maxLK ? P.maxLK : n); }
        return;
    }
    // ---- the voted, live keyframes in order, and the first of them with the largest count (:2197-2212)
    const int* order = M.kf_order;
    const int K = compact_ordered<256>(nK, s_wcnt, tid,
        [&](int j) {
            const int k = order ? order[j] : j;
            return in_range(k, nK) && (row_load(&vote[k]) & (kVoteMark - 1)) > 0 && kf_live(M, k);
        },
        [&](int j, int slot) {
            const int k = order ? order[j] : j;
            const int count = atomicOr(&vote[k], kVoteMark) & (kVoteMark - 1);
            if (slot < kExpandCap) s_list[slot] = k;
            if (slot < P.maxLK) row[slot] = k;
            atomicMax(&s_best, ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)j));
        });
    if (tid == 0) {
        s_size = K;
        if (s_best != 0ull) { const int j = (int)(0xffffffffu - (unsigned)s_best); refKf[f] = order ? order[j] : j; }   // :2266-2269
    }
    // ---- the expansion (:2216-2264): wave 0, over the K voted entries; K > 80 leaves at the first test
    if (tid < 64 && K <= kLocalLimit) {
        volatile int* list = s_list;
        int size = K;
        // included: voted (the mark, set before the barrier above) or appended by an earlier step (list[K .. size))
        auto included = [&](int x) {
            if (row_load(&vote[x]) & kVoteMark) return true;
            for (int q = K; q < size; q++) if (list[q] == x) return true;
            return false;
        };
        auto append = [&](int x) {
            if (lane == 0) { list[size] = x; if (size < P.maxLK) row[size] = x; }
            size++;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                 // lane 0's entry before the other lanes' next included()
        };
        for (int it = 0; it < K; it++) {
            if (size > kLocalLimit) break;                                                         // :2221
            const int k = list[it];
            {   // the first neighbour of the ten that is live and not yet included (:2225-2239)
                const int nb = lane < kNeigh ? M.kf_neigh[(size_t)k * kNeigh + lane] : -1;
                const bool ok = in_range(nb, nK) && kf_live(M, nb) && !included(nb);
                const unsigned long long hit = __ballot(ok);
                if (hit) append(__builtin_amdgcn_readlane(nb, __ffsll((long long)hit) - 1));
            }
            {   // the first such child in the given order (:2241-2254)
                int b, e;
                if (csr_row(M.kf_child_offsets, k, M.n_children, b, e))
                    for (int c = b; c < e; c += 64) {
                        const int ch = c + lane < e ? M.kf_children[c + lane] : -1;
                        const bool ok = in_range(ch, nK) && kf_live(M, ch) && !included(ch);
                        const unsigned long long hit = __ballot(ok);
                        if (hit) { append(__builtin_amdgcn_readlane(ch, __ffsll((long long)hit) - 1)); break; }
                    }
            }
            // the parent, bad or not, ends the expansion for every later keyframe (:2256-2263)
            const int par = M.kf_parent[k];
            if (in_range(par, nK) && !included(par)) { append(par); break; }
        }
        if (lane == 0) s_size = size;
    }
    __syncthreads();
    const int total = s_size;
    for (int j = total + tid; j < P.maxLK; j += 256) row[j] = -1;
    if (tid == 0) nLocalKf[f] = total;
}

DEVINL unsigned hash_of(int m, int log2n) { return ((unsigned)m * 0x9e3779b1u) >> (32 - log2n); }

__global__ __launch_bounds__(256) void k_map_points(MapParams P, ivf_map_view M, const int* __restrict__ framePoints, const int* __restrict__ localKf,
                                                   const int* __restrict__ nLocalKf, unsigned* hashScratch, int heldLog2, uint4* __restrict__ out,
                                                   int* __restrict__ outIds, int* __restrict__ offsets, int* __restrict__ nLocalPoints,
                                                   uint8_t* __restrict__ occupied)
{
    extern __shared__ int s_held[];                           // [1 << heldLog2] the points the frame holds, -1 = empty
    __shared__ int s_wcnt[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int nK = M.n_keyframes, nP = M.n_points;
    const unsigned slots = 1u << P.hashLog2, heldSlots = 1u << heldLog2;
    unsigned* ids = hashScratch + (size_t)f * 2 * slots;
    unsigned* pos = ids + slots;
    const int* fp = framePoints + (size_t)f * P.nf;
    const int* row = localKf + (size_t)f * P.maxLK;
    const int nLK0 = nLocalKf[f], nLK = nLK0 < 0 ? 0 : (nLK0 > P.maxLK ? P.maxLK : nLK0);
    for (unsigned i = tid; i < heldSlots; i += 256) s_held[i] = -1;
    if (tid == 0) { offsets[f] = f * P.maxPts; if (f == (int)gridDim.x - 1) offsets[f + 1] = (f + 1) * P.maxPts; }
    __syncthreads();
    // ---- what the frame holds: the set behind flags bit 0 of its local points, and d_occupied (ORBmatcher.cc:87-89)
    for (int i = tid; i < P.nf; i += 256) {
        const int m = fp[i];
        uint8_t occ = 0;
        if (in_range(m, nP)) {
            occ = (M.points[m].flags & 2) ? 1 : 0;
            for (unsigned h = hash_of(m, heldLog2), n = 0; n < heldSlots; n++, h = (h + 1) & (heldSlots - 1)) {   // at most nf <= heldSlots / 2 entries
                const int old = atomicCAS(&s_held[h], -1, m);
                if (old == -1 || old == m) break;
            }
        }
        occupied[(size_t)f * P.nf + i] = occ;
    }
    // the candidate (a, j): keyframe a of the row, its keypoint j -> the point, or -1 for none / bad / out of range
    auto row_of = [&](int a, int& b, int& len) {
        const int k = row[a];
        int e;
        len = 0;
        if (in_range(k, nK) && csr_row(M.kf_point_offsets, k, M.n_kf_points, b, e)) len = e - b > P.nf ? P.nf : e - b;
    };
    auto point_at = [&](int b, int j) {
        const int m = M.kf_points[b + j];
        return in_range(m, nP) && !(M.points[m].flags & 1) ? m : -1;
    };
    // ---- pass 1: the first position of every point (:2159: mnTrackReferenceForFrame == mnId -> continue)
    for (int a = 0; a < nLK; a++) {
        int b, len;
        row_of(a, b, len);
        for (int j = tid; j < len; j += 256) {
            const int m = point_at(b, j);
            if (m < 0) continue;
            for (unsigned h = hash_of(m, P.hashLog2), n = 0; n < slots; n++, h = (h + 1) & (slots - 1)) {
                const unsigned old = atomicCAS(&ids[h], kEmpty, (unsigned)m);
                if (old == kEmpty || old == (unsigned)m) { atomicMin(&pos[h], (unsigned)(a * P.nf + j)); break; }
            }
        }
    }
    __threadfence();
    __syncthreads();
    // ---- pass 2: the candidates in order, kept where they are the first of their point
    uint4* outRow = out + (size_t)f * P.maxPts * 5;
    int* idRow = outIds + (size_t)f * P.maxPts;
    int total = 0;
    for (int a = 0; a < nLK; a++) {
        int b, len;
        row_of(a, b, len);
        const int base = total;
        total += compact_ordered<256>(len, s_wcnt, tid,
            [&](int j) {
                const int m = point_at(b, j);
                if (m < 0) return false;
                for (unsigned h = hash_of(m, P.hashLog2), n = 0; n < slots; n++, h = (h + 1) & (slots - 1)) {
                    const unsigned id = set_load(&ids[h]);
                    if (id == (unsigned)m) return set_load(&pos[h]) == (unsigned)(a * P.nf + j);
                    if (id == kEmpty) break;
                }
                return false;
            },
            [&](int j, int slot) {
                slot += base;
                if (slot >= P.maxPts) return;
                const int m = M.kf_points[b + j];
                bool held = false;
                for (unsigned h = hash_of(m, heldLog2), n = 0; n < heldSlots; n++, h = (h + 1) & (heldSlots - 1)) {
                    const int id = s_held[h];
                    if (id == m) { held = true; break; }
                    if (id == -1) break;
                }
                const uint4* src = (const uint4*)(M.points + m);
                uint4 r0 = src[0], r1 = src[1], r2 = src[2], r3 = src[3], r4 = src[4];
                if (held) r4.x |= 1u;                                                              // flags: mnLastFrameSeen == mnId (:2114)
                uint4* dst = outRow + (size_t)slot * 5;
                dst[0] = r0; dst[1] = r1; dst[2] = r2; dst[3] = r3; dst[4] = r4;
                idRow[slot] = m;
            });
    }
    for (int s = total + tid; s < P.maxPts; s += 256) {
        uint4* dst = outRow + (size_t)s * 5;
        const uint4 z = make_uint4(0, 0, 0, 0);
        dst[0] = z; dst[1] = z; dst[2] = z; dst[3] = z; dst[4] = make_uint4(1u, 0, 0, 0);
        idRow[s] = -1;
    }
    if (tid == 0) nLocalPoints[f] = total;
}

int ceil_log2(size_t n) { int l = 0; while (((size_t)1 << l) < n) l++; return l; }

// the scratch of ivf_tracker_update_local_map: voteInts ints of vote rows (0: the rows are in LDS), hashWords words of hash sets
int map_grow(ivf_tracker* t, size_t voteInts, size_t hashWords)
{
    MapScratch& S = t->map;
    if (voteInts > S.voteCap) {
        if (!t->replace({{S.vote, voteInts * sizeof(int)}})) return fail(IVF_E_NO_DEVICE, "device allocation failed for %zu vote cells", voteInts);
        S.voteCap = voteInts;
    }
    if (hashWords > S.hashCap) {
        if (!t->replace({{S.hash, hashWords * sizeof(unsigned)}})) return fail(IVF_E_NO_DEVICE, "device allocation failed for %zu hash words", hashWords);
        S.hashCap = hashWords;
    }
    return IVF_OK;
}

// log2 of a frame's hash set: it holds the distinct points of the candidates, never more than there are candidates, nor than there are
// points, at a load of at most one half
int hash_log2(int max_local_keyframes, int nf, int n_points)
{
    size_t distinct = (size_t)max_local_keyframes * (size_t)nf;
    if ((size_t)n_points < distinct) distinct = (size_t)n_points;
    const int l = ceil_log2(2 * distinct);
    return l < 6 ? 6 : l;
}

}  // namespace

extern "C" int ivf_tracker_local_map_lds_keyframes(void) { return kVoteLds; }

extern "C" size_t ivf_tracker_local_map_set_bytes(int nfeatures, int n_points, int n_frames, int max_local_keyframes)
{
    if (nfeatures < 1 || n_points < 0 || n_frames < 0 || max_local_keyframes < 1) return 0;
    const int l = hash_log2(max_local_keyframes, nfeatures, n_points);
    return l > 30 ? 0 : (size_t)n_frames * 2 * ((size_t)1 << l) * sizeof(unsigned);
}

extern "C" int ivf_tracker_update_local_map(ivf_tracker* t, const ivf_map_view* map, int32_t* d_frame_points, int n_frames, int max_local_keyframes,
                                            int max_points_per_frame, int32_t* d_local_kf, int32_t* d_n_local_kf, int32_t* d_ref_kf,
                                            ivf_local_point* d_points, int32_t* d_point_ids, int32_t* d_point_offsets, int32_t* d_n_local_points,
                                            uint8_t* d_occupied, void* hip_stream)
{
    if (!t || !map || !d_frame_points || !d_local_kf || !d_n_local_kf || !d_ref_kf || !d_points || !d_point_ids || !d_point_offsets ||
        !d_n_local_points || !d_occupied)
        return fail(IVF_E_INVALID, "null argument");
    const ivf_map_view M = *map;
    if (M.n_points < 0 || M.n_keyframes < 0 || M.n_obs < 0 || M.n_kf_points < 0 || M.n_children < 0)
        return fail(IVF_E_INVALID, "a negative table length in the map view");
    if (!M.obs_offsets || !M.kf_point_offsets || !M.kf_child_offsets || (M.n_points > 0 && !M.points) || (M.n_obs > 0 && !M.obs_kf) ||
        (M.n_kf_points > 0 && !M.kf_points) || (M.n_children > 0 && !M.kf_children) || (M.n_keyframes > 0 && (!M.kf_neigh || !M.kf_parent)))
        return fail(IVF_E_INVALID, "null table in the map view");
    if (((size_t)M.points & 15) != 0 || ((size_t)d_points & 15) != 0) return fail(IVF_E_INVALID, "the point arrays must be 16-byte aligned");
    if (max_local_keyframes < 1) return fail(IVF_E_INVALID, "max_local_keyframes must be >= 1");
    if (max_points_per_frame < 1) return fail(IVF_E_INVALID, "max_points_per_frame must be >= 1");
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, false, 0, 0, n_frames, st);
    if (rc != IVF_OK) return rc;
    if (n_frames == 0) return IVF_OK;
    const int nf = t->P.nf;
    if ((long long)n_frames * max_points_per_frame > 0x7fffffffLL)
        return fail(IVF_E_CAPACITY, "%d frames x %d points exceed the int32 offsets", n_frames, max_points_per_frame);
    if ((long long)max_local_keyframes * nf > 0x7fffffffLL)
        return fail(IVF_E_CAPACITY, "%d local keyframes x %d features exceed the int32 positions", max_local_keyframes, nf);
    MapParams P;
    P.nf = nf; P.maxLK = max_local_keyframes; P.maxPts = max_points_per_frame;
    P.voteInLds = M.n_keyframes <= kVoteLds ? 1 : 0;
    P.hashLog2 = hash_log2(max_local_keyframes, nf, M.n_points);
    if (P.hashLog2 > 30) return fail(IVF_E_CAPACITY, "%d local keyframes x %d features exceed one hash set", max_local_keyframes, nf);
    const size_t slots = (size_t)1 << P.hashLog2;
    int heldLog2 = ceil_log2(2 * (size_t)nf);
    if (heldLog2 < 6) heldLog2 = 6;
    const int rg = map_grow(t, P.voteInLds ? 0 : (size_t)n_frames * (size_t)M.n_keyframes, (size_t)n_frames * 2 * slots);
    if (rg != IVF_OK) return rg;
    const MapScratch S = t->map;
    HIPCHK(hipMemsetAsync(S.hash, 0xff, (size_t)n_frames * 2 * slots * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_map_keyframes, dim3(n_frames), dim3(256), P.voteInLds ? (size_t)M.n_keyframes * sizeof(int) : 0, st, P, M, d_frame_points,
                       S.vote, d_local_kf, d_n_local_kf, d_ref_kf);
    hipLaunchKernelGGL(k_map_points, dim3(n_frames), dim3(256), ((size_t)1 << heldLog2) * sizeof(int), st, P, M, d_frame_points, d_local_kf, d_n_local_kf,
                       S.hash, heldLog2, (uint4*)d_points, d_point_ids, d_point_offsets, d_n_local_points, d_occupied);
    return tracker_end(t, st);
}
