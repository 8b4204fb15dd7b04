// ivf_select.hip -- keypoint selection of the gfx950 front end: ComputeKeyPointsOld's quotas and both retainBest passes.
//
// Path (ORB/ = introspective_ORB_SLAM/), between k_fast_nms and k_describe of ivf_kernels.hip:
//   k_cell_qsum     cv::sum over the cost-map window of every cell (introspection)        (ORBextractor.cc :977)
//   k_quota         threshold fallback, cell quotas, redistribution, list offsets           (:946-987, :1028-1133)
//   k_cell_select / k_cell_select_list / k_cell_select_huge   one body, cell_select_one: a cell's survivors in cv::FAST's order,
//                   response x quality, retainBest                                           (:1058-1080, :1146-1148)
//   k_level_select  level-wide retainBest, keypoint slots                                   (:1162-1166)
// retainBest is std::nth_element: libstdc++'s introselect replayed compare for compare, once sequentially and once wave-cooperatively.
#include "ivf_device.h"
#include <algorithm>

namespace ivf {

// ------------------------------------------------------------------------------------------------
// libstdc++ std::nth_element (bits/stl_algo.h __introselect) on 64-bit keys whose high word is the
// response as f32 bits (responses are >= 0, so unsigned compare == float compare).  Must replay the
// exact compare/swap sequence: FAST responses tie constantly and the surviving ORDER feeds every
// downstream index (SURVEY §7 hard part 1).  Comparator = cv::KeypointResponseGreater.
// ------------------------------------------------------------------------------------------------
typedef unsigned long long u64;
#define RGT(a, b) ((unsigned)((a) >> 32) > (unsigned)((b) >> 32))

template <typename PTR>
DEVINL void sel_adjust_heap(PTR f, int hole, int len, u64 value)
{
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (RGT(f[child], f[child - 1])) child--;
        f[hole] = f[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        f[hole] = f[child - 1];
        hole = child - 1;
    }
    int parent = (hole - 1) / 2;
    while (hole > top && RGT(f[parent], value)) {
        f[hole] = f[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    f[hole] = value;
}
// The three passages of __introselect that run sequentially in both replays below.
// depth limit reached: __heap_select(first, nth + 1, last) ; iter_swap(first, nth)
template <typename PTR>
DEVINL void sel_heap_select(PTR v, int first, int nth, int last)
{
    PTR f = v + first;
    const int len = nth + 1 - first;
    if (len >= 2) {
        int parent = (len - 2) / 2;
        for (;;) { u64 val = f[parent]; sel_adjust_heap(f, parent, len, val); if (parent == 0) break; parent--; }
    }
    for (int i = nth + 1; i < last; ++i)
        if (RGT(v[i], f[0])) { u64 val = v[i]; v[i] = f[0]; sel_adjust_heap(f, 0, len, val); }
    u64 tmp = v[first]; v[first] = v[nth]; v[nth] = tmp;
}
// __move_median_to_first(first, first + 1, mid, last - 1)
template <typename PTR>
DEVINL void sel_median_to_first(PTR v, int first, int last)
{
    const int mid = first + (last - first) / 2;
    const int a = first + 1, b = mid, c = last - 1;
    const u64 va = v[a], vb = v[b], vc = v[c];
    int m;
    if (RGT(va, vb)) { if (RGT(vb, vc)) m = b; else if (RGT(va, vc)) m = c; else m = a; }
    else if (RGT(va, vc)) m = a;
    else if (RGT(vb, vc)) m = c;
    else m = b;
    const u64 tmp = v[first]; v[first] = v[m]; v[m] = tmp;
}
// __insertion_sort(first, last), <= 3 elements
template <typename PTR>
DEVINL void sel_insertion_sort(PTR v, int first, int last)
{
    for (int i = first + 1; i < last; ++i) {
        const u64 val = v[i];
        if (RGT(val, v[first])) { for (int k = i; k > first; --k) v[k] = v[k - 1]; v[first] = val; }
        else { int l = i; while (RGT(val, v[l - 1])) { v[l] = v[l - 1]; --l; } v[l] = val; }
    }
}
DEVINL int sel_depth_limit(int n)                   // 2 * floor(log2(n))
{
    int depth = 0;
    for (int t = n; t > 1; t >>= 1) depth++;
    return 2 * depth;
}

// One thread, lists anywhere: k_level_select's fallback for a level list longer than its LDS copy.
template <typename PTR>
DEVINL void sel_nth_element(PTR v, int n, int nth)
{
    if (n <= 0 || nth >= n) return;
    int first = 0, last = n;
    int depth = sel_depth_limit(n);
    while (last - first > 3) {
        if (depth == 0) { sel_heap_select(v, first, nth, last); return; }
        --depth;
        sel_median_to_first(v, first, last);
        // __unguarded_partition(first+1, last, pivot = first)
        int lo = first + 1, hi = last;
        const u64 pivot = v[first];
        for (;;) {
            while (RGT(v[lo], pivot)) ++lo;
            --hi;
            while (RGT(pivot, v[hi])) --hi;
            if (!(lo < hi)) break;
            u64 tmp = v[lo]; v[lo] = v[hi]; v[hi] = tmp;
            ++lo;
        }
        if (lo <= nth) first = lo; else last = lo;
    }
    sel_insertion_sort(v, first, last);
}

// ------------------------------------------------------------------------------------------------
// Wave-cooperative replay of the same introselect.  The sequential bottleneck of std::nth_element is
// __unguarded_partition's two pointer scans; its outcome, however, is a pure function of the array at
// the start of the round:
//   a_0 < a_1 < ...  positions >= first+1 whose value is NOT greater than the pivot  (where `lo` stops)
//   b_0 > b_1 > ...  positions <= last-1  whose value is NOT less    than the pivot  (where `hi` stops)
//   the loop swaps (a_k, b_k) for k < K, K = first k with a_k >= b_k, and returns
//   cut = min(a_K, b_{K-1})   (a swapped-in value <= pivot sits at b_{K-1}; b_{-1} = +inf)
// so one round is two ordered compactions (wave ballots), a count and K independent swaps: O(range/64)
// steps instead of O(range).  The three sequential passages stay on lane 0.  All 64 lanes call this with
// uniform arguments.  SYNC orders one lane's stores before another lane's loads of v, A, B:
//   SyncLds     the lists live in LDS
//   SyncGlobal  the lists live in global memory (the huge tier's scratch slot): a workgroup-scope fence
//               (s_waitcnt vmcnt(0)); the CU's L1 is write-through, so the wave then reads what it wrote
// ------------------------------------------------------------------------------------------------
struct SyncLds { DEVINL void operator()() const { wave_sync_lds(); } };
struct SyncGlobal {
    DEVINL void operator()() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
};
template <typename SYNC, typename PTR, typename IDX>
DEVINL void sel_nth_element_wave(PTR v, int n, int nth, IDX A, IDX B, int lane)
{
    const SYNC sync;
    if (n <= 0 || nth >= n) return;
    int first = 0, last = n;
    int depth = sel_depth_limit(n);
    while (last - first > 3) {
        if (depth == 0) {                       // rare: finish sequentially exactly as libstdc++ does
            if (lane == 0) sel_heap_select(v, first, nth, last);
            sync();
            return;
        }
        --depth;
        if (lane == 0) sel_median_to_first(v, first, last);
        sync();
        const unsigned pivot = (unsigned)(v[first] >> 32);
        const int lo0 = first + 1, len = last - lo0;
        // ordered compaction of the left stops (ascending) and right stops (descending position)
        int nA = 0, nB = 0;
        for (int base = 0; base < len; base += 64) {
            const int i = lo0 + base + lane;                     // ascending walk
            const bool inA = base + lane < len && !((unsigned)(v[i] >> 32) > pivot);
            const unsigned long long mA = __ballot(inA);
            if (inA) A[nA + __popcll(mA & ((1ull << lane) - 1ull))] = i;
            nA += __popcll(mA);
            const int j = last - 1 - base - lane;                // descending walk
            const bool inB = base + lane < len && !(pivot > (unsigned)(v[j] >> 32));
            const unsigned long long mB = __ballot(inB);
            if (inB) B[nB + __popcll(mB & ((1ull << lane) - 1ull))] = j;
            nB += __popcll(mB);
        }
        sync();
        // K = number of leading pairs with a_k < b_k (monotone predicate)
        const int nP = min(nA, nB);
        int K = 0;
        for (int base = 0; base < nP; base += 64) {
            const int k = base + lane;
            const bool ok = k < nP && (int)A[k] < (int)B[k];
            const unsigned long long mk = __ballot(ok);
            K += __popcll(mk);
            if (mk != ~0ull) break;
        }
        const int aK = K < nA ? (int)A[K] : 0x7fffffff;
        const int bKm1 = K > 0 ? (int)B[K - 1] : 0x7fffffff;
        const int cut = min(aK, bKm1);
        for (int k = lane; k < K; k += 64) {                     // the swaps touch disjoint positions
            const int ia = A[k], ib = B[k];
            const u64 ta = v[ia], tb = v[ib];
            v[ia] = tb; v[ib] = ta;
        }
        sync();
        if (cut <= nth) first = cut; else last = cut;
    }
    if (lane == 0) sel_insertion_sort(v, first, last);
    sync();
}


// ------------------------------------------------------------------------------------------------
// Keypoint selection = ComputeKeyPointsOld :880-1213 minus the per-pixel work, in three kernels:
//   k_quota        per (image, level): `<=3 -> minThFAST` fallback per cell (:1047) from k_fast_nms's counters,
//                  cost-map cell weights and quotas (:946-987, :1028-1031), the single-pass quota redistribution
//                  (:1103-1133); what retainBest will keep per cell is data-independent, so the offsets of the
//                  concatenated level list are fixed here too.
//   k_cell_select  per (image, cell), one wave: restore cv::FAST's row-major order (bitonic sort of the packed
//                  positions in LDS), response x quality (:1058-1080), retainBest (:1146-1148) = exact replay of
//                  libstdc++ introselect by one lane on the LDS list, kept entries -> level list (i,j order).
//   k_level_select per (image, level): level-wide retainBest (:1162-1166), keypoint slots, level count.
// Candidate counts per cell are heavy-tailed (tens typically, >1000 on repetitive texture); one wave per cell lets
// the hardware balance that, and keeps every sequential replay in LDS (~64-cycle steps instead of L2 round trips).
// ------------------------------------------------------------------------------------------------
// level of a global cell index: the last VALID level whose cellBase is <= gc, from one wide scalar load (r06: the loop over cfg->lv[l].valid / .cellBase was two
// dependent scalar round trips per level at the head of every cell's wave)
DEVINL int level_of_cell(const Config* __restrict__ cfg, int gc)
{
    int level = 0;
#pragma unroll
    for (int l = 1; l < kMaxLevels; l++) level = gc >= cfg->cellBases[l] ? l : level;
    return level;
}


// cv::sum over every cell WINDOW of the cost pyramid (:977), one wave per cell; the sums are parked in cellInfo[].x
// until k_quota consumes them (introspection only).
__global__ __launch_bounds__(256) void k_cell_qsum(const Config* __restrict__ cfg, const uint8_t* __restrict__ qpyr,
                                                  const uint8_t* __restrict__ useCost, CellInfo* __restrict__ cellInfo)
{
    const int img = blockIdx.y, lane = threadIdx.x & 63;
    const int cell = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // a scalar: the level geometry below then comes through scalar loads
    if (cell >= cfg->nCellsTotal || !(cfg->introspection && (use_cost_of(useCost, img) & 1))) return;
    const int level = level_of_cell(cfg, cell);
    const LevelGeom& G = cfg->lv[level];
    const int c = cell - G.cellBase, cols = G.cols, rows = G.rows;
    if (!G.valid || c >= G.nCells) return;
    const uint8_t* Q = qpyr + (size_t)img * cfg->pyrBytes + G.off;
    const int i = c / cols, j = c % cols;
    const int x0 = kEdge + j * G.cellW, y0 = kEdge + i * G.cellH;
    const int wx0 = x0 - 3, wx1 = (j == cols - 1) ? G.maxBX + 3 : x0 + G.cellW + 3;
    const int wy0 = y0 - 3, wy1 = wy0 + ((i == rows - 1) ? G.winHLast : G.cellH + 6);
    // aligned dwords covering [wx0, wx1); bytes outside the window are masked; v_sad_u8 sums 4 bytes per op
    const int a0 = wx0 & ~3, nq = (wx1 - a0 + 3) / 4, nrow = wy1 - wy0;
    unsigned acc = 0;
    // r06: eight dwords per lane in flight.  One load per iteration with its use right behind it is one round trip per iteration: a level-0 cell's window is
    // ~4,500 dwords = 70 SEQUENTIAL round trips per wave, which was the kernel's whole time (87 us per 128 cost images, 325 at 1920 x 1200)
    constexpr int U = 8;
    const int total = nq * nrow;
    const int dr = 64 / nq, dq = 64 % nq;                                      // (row, dword) of item t + 64 from those of item t: one division per wave, not one per item
    int rr = lane / nq, qq = lane % nq;
    for (int t0 = lane; t0 < total; t0 += 64 * U) {
        unsigned v[U]; int bxs[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool in = t0 + 64 * u < total;
            const int r = in ? rr : nrow - 1, q = in ? qq : nq - 1;             // past the end: the last item again (not counted)
            bxs[u] = a0 + 4 * q;
            v[u] = *(const unsigned*)(Q + (size_t)(wy0 + r) * G.pitch + bxs[u]);
            qq += dq; rr += dr;
            if (qq >= nq) { qq -= nq; rr++; }
        }
#pragma unroll
        for (int u = 0; u < U; u++) asm volatile("" : "+v"(v[u]));            // (keeps the compiler from sinking a load into the branch of its use)
#pragma unroll
        for (int u = 0; u < U; u++) {
            unsigned w = v[u];
            const int bx = bxs[u];
            if (bx < wx0) w &= 0xffffffffu << (8 * (wx0 - bx));
            if (bx + 4 > wx1) w &= 0xffffffffu >> (8 * (bx + 4 - wx1));
            if (t0 + 64 * u < total) acc = __builtin_amdgcn_sad_u8(w, 0u, acc);
        }
    }
    const unsigned qs = (unsigned)wave_sum_i32((int)acc);
    if (lane == 0) cellInfo[(size_t)img * cfg->nCellsTotal + cell].nTotal = (int)qs;
}

constexpr int kCellCapTiny = 256, kCellCapSmall = 1024, kCellCapBig = 4096;
__global__ __launch_bounds__(256) void k_quota(const Config* __restrict__ cfg, const int* __restrict__ cellCnt,
                                              const uint8_t* __restrict__ qpyr, const uint8_t* __restrict__ useCost,
                                              CellInfo* __restrict__ cellInfo, int* __restrict__ lvlTotal,
                                              int* __restrict__ hugeCount, int* __restrict__ hugeList, int* __restrict__ tierList,
                                              int tierCap, int* __restrict__ status, int cap)
{
    // r06: the bookkeeping arrays are sized by the launch (cap = the largest level's cell count, rounded up) instead of kMaxCells = 2048 each: 51 KB per workgroup
    // meant three workgroups per CU for 2,048 (level, image) workgroups -- three rounds of a kernel whose time is one thread's sequential pass
    extern __shared__ __attribute__((aligned(16))) int s_quota[];
    int* const s_nIni = s_quota; int* const s_nMin = s_nIni + cap; int* const s_nTotal = s_nMin + cap; int* const s_nRetain = s_nTotal + cap;
    int* const s_prefix = s_nRetain + cap;                    // [cap + 1]
    unsigned* const s_qsum = (unsigned*)(s_prefix + cap + 4);
    float* const s_diff = (float*)(s_qsum + cap);             // nfeatures_cell - nKeys of the cells that keep all their keypoints
    unsigned char* const s_useMin = (unsigned char*)(s_diff + cap);
    __shared__ float s_wsum;
    const int img = blockIdx.y, level = blockIdx.x;
    const LevelGeom& G = cfg->lv[level];
    const int tid = threadIdx.x;
    if (!G.valid) { if (tid == 0) lvlTotal[img * kMaxLevels + level] = 0; return; }
    const int mode = (cfg->introspection && (use_cost_of(useCost, img) & 1)) ? 1 : 0;
    const int nCells = G.nCells, cols = G.cols, rows = G.rows;
    const int* cnt = cellCnt + ((size_t)img * cfg->nCellsTotal + G.cellBase) * 2;
    CellInfo* ci = cellInfo + (size_t)img * cfg->nCellsTotal + G.cellBase;
    if (mode && G.winHLast <= 0) {
        // the last cell row starts exactly at the bottom border: its hY is 0, the row is skipped (:953-954) and the stale hY
        // makes every other window of the level empty too -- the level yields nothing (accepted geometry, Context::build)
        for (int c = tid; c < nCells; c += 256) ci[c] = CellInfo{0, 0, 0, 0};
        if (tid == 0) lvlTotal[img * kMaxLevels + level] = 0;
        return;
    }
    for (int c = tid; c < nCells; c += 256) {
        s_nMin[c] = cnt[2 * c]; s_nIni[c] = cnt[2 * c + 1];
        s_qsum[c] = mode ? (unsigned)ci[c].nTotal : 0u;       // window sums from k_cell_qsum
    }
    __syncthreads();
    // r06: everything that is a function of ONE cell runs on all threads (the window weight with its f64 division, nfeatures_cell with its division and ceil,
    // the keep-all / retain decision); thread 0 keeps only what the reference's order defines: the float sum of the weights in (i, j) order, the int / float
    // accumulation of nToDistribute, the redistribution pass and the prefix.  (Was: all of it on thread 0 -- ~600 cycles per cell with 255 threads idle.)
    if (mode) {
        for (int c = tid; c < nCells; c += 256) {
            const int i = c / cols, j = c % cols;
            const float hX = (j == cols - 1) ? (float)(G.maxBX + 3 - (16 + j * G.cellW)) : (float)(G.cellW + 6);
            const float hY = (i == rows - 1) ? (float)G.winHLast : (float)(G.cellH + 6);
            const float cost = (float)s_qsum[c] / (float)(hX * hY);
            const float q = (float)(1.0 / (1.0 + (double)(cost / 255)));
            s_qsum[c] = __float_as_uint(2 * q - 1);
        }
        __syncthreads();
        if (tid == 0) { float wsum = 0.0f; for (int c = 0; c < nCells; c++) wsum += __uint_as_float(s_qsum[c]); s_wsum = wsum; }
        __syncthreads();
    }
    {
        const float wsum = mode ? s_wsum : 1.0f;
        for (int c = tid; c < nCells; c += 256) {
            const float nfc = mode ? fmaxf(1.0f, ceilf((float)G.nDesired * __uint_as_float(s_qsum[c]) / wsum))
                                   : (float)G.nfeaturesCell;
            const bool useMin = s_nIni[c] <= 3;
            const int nKeys = useMin ? s_nMin[c] : s_nIni[c];
            s_useMin[c] = useMin;
            s_nTotal[c] = nKeys;
            if ((float)nKeys > nfc) { s_nRetain[c] = (int)nfc; s_prefix[c] = 0; }
            else { s_nRetain[c] = nKeys; s_diff[c] = nfc - (float)nKeys; s_prefix[c] = 1; }      // s_prefix doubles as bNoMore here
            s_nIni[c] = __float_as_int(nfc);            // keep nfeatures_cell for the redistribution pass
        }
    }
    __syncthreads();
    if (tid == 0) {                                   // the order-dependent rest, exactly in (i,j) order
        int nToDistribute = 0, nNoMore = 0;
        for (int c = 0; c < nCells; c++)
            if (s_prefix[c]) { nToDistribute = (int)((float)nToDistribute + s_diff[c]); nNoMore++; }
        if (nToDistribute > 0 && nNoMore < nCells) {
            for (int c = 0; c < nCells; c++) {
                if (!s_prefix[c]) {
                    const int nNew = (int)(__int_as_float(s_nIni[c]) + ceilf((float)nToDistribute / (nCells - nNoMore)));
                    if (s_nTotal[c] > nNew) s_nRetain[c] = nNew;
                    else { s_nRetain[c] = s_nTotal[c]; nToDistribute += nNew - s_nTotal[c]; s_prefix[c] = 1; nNoMore++; }
                }
            }
        }
        int acc = 0;
        for (int c = 0; c < nCells; c++) {
            const int nT = s_nTotal[c], nR = s_nRetain[c];
            s_prefix[c] = acc;
            acc += (nR >= 0 && nT > nR) ? nR : nT;
        }
        lvlTotal[img * kMaxLevels + level] = acc;
    }
    __syncthreads();
    for (int c = tid; c < nCells; c += 256) {
        ci[c] = CellInfo{s_nTotal[c], s_nRetain[c], s_prefix[c], (int)s_useMin[c]};
        // cells above the one-wave tier go on the work list of their tier (hugeCount[1], [2]: r04 -- their kernels walk the list
        // instead of launching a workgroup per cell of every image that looks at its count and leaves)
        if (s_nTotal[c] > kCellCapTiny && s_nTotal[c] <= kCellCapBig) {
            const int tier = s_nTotal[c] > kCellCapSmall ? 1 : 0;
            const int k = atomicAdd(hugeCount + 1 + tier, 1);
            if (k < tierCap) tierList[(size_t)tier * tierCap + k] = img * cfg->nCellsTotal + G.cellBase + c;
            else atomicOr(status, 4);
        }
        if (s_nTotal[c] > kCellCapBig) {                 // too many survivors for the LDS selection: k_cell_select_huge's work list
            const int k = atomicAdd(hugeCount, 1);
            if (hugeList && k < kHugeListCap) hugeList[k] = img * cfg->nCellsTotal + G.cellBase + c;
            else atomicOr(status, 4);
        }
    }
}

// pass 0 handles cells with <= kCellCapSmall candidates (12 KB LDS, many waves per CU); pass 1 those up to kCellCapBig;
// anything bigger (large images with few features: 1920x1200 at N = 500 has 627x290-pixel cells) goes to k_cell_select_huge
// NTHR = 64: one wave per cell (the common, small cells: many cells per CU).  NTHR = 256 for the big-cell pass: gather and
// sort run on four waves (with the introspection quirk of overlapping cell domains most level-0/1 cells hold
// 1-4 thousand candidates and a single wave spent ~100 us per cell in the sort); the introselect stays on wave 0.
constexpr int kSelRows = 512;                            // tallest cell (rows) the counting sort of cell_select_one handles
struct SelCounts {
    int row[kSelRows + 2];                                    // per-row survivor counts, then their exclusive prefix
    int m;
};
// Where cell_select_one keeps a cell's lists.  keys: the packed survivors, padded to a power of two by the bitonic sort, and
// once `ord` is built the two partition stop lists of `Stop` indices; ord: the 64-bit keys (before that the counting sort's
// arrival ranks and grouped copy).  WaveSync is what a one-wave workgroup needs between two steps on the lists.
template <int CAP>
struct __attribute__((aligned(16))) SelShared {               // all of it in LDS, CAP (a power of two) survivors
    static constexpr bool kGlobal = false;
    static constexpr int kCap = CAP;
    typedef unsigned short Stop;
    typedef SyncLds WaveSync;
    unsigned keys[CAP];
    u64 ord[CAP];
    SelCounts c;
};
struct SelGlobal {                                            // the lists in a global scratch slot: keys u32[2 * cap], ord u64[cap]
    static constexpr bool kGlobal = true;
    typedef unsigned Stop;
    typedef SyncGlobal WaveSync;
    unsigned* keys;
    u64* ord;
    SelCounts& c;                                             // (LDS)
    int cap;
};
template <int NTHR, typename WAVESYNC>
DEVINL void sel_sync()
{
    if constexpr (NTHR == 64) WAVESYNC()(); else __syncthreads();
}
template <int NTHR, typename STORE>
DEVINL void cell_select_one(const Config* __restrict__ cfg, const unsigned* __restrict__ tileList,
                            const int* __restrict__ tileCnt, const CellInfo* __restrict__ cellInfo,
                            const uint8_t* __restrict__ qpyr, const uint8_t* __restrict__ useCost,
                            u64* __restrict__ lvlList, int* __restrict__ status, int nLo, int nHi, int img, int gc, int tid, STORE& S)
{
    typedef typename STORE::Stop Stop;
    int cap;
    if constexpr (STORE::kGlobal) cap = S.cap; else cap = STORE::kCap;
    unsigned* const keys = S.keys;
    u64* const ord = S.ord;
    int* const s_row = S.c.row;
    int& s_m = S.c.m;
    Stop* stopA = (Stop*)keys;                                // the sort keys are dead once `ord` is built:
    Stop* stopB = stopA + cap;                                // their space holds the partition stop lists
    const int lane = tid & 63;
    auto sync = [&]() { sel_sync<NTHR, typename STORE::WaveSync>(); };
    const int level = level_of_cell(cfg, gc);
    const LevelGeom& G = cfg->lv[level];
    const int c = gc - G.cellBase;
    if (!G.valid || c < 0 || c >= G.nCells) return;
    const CellInfo info = cellInfo[(size_t)img * cfg->nCellsTotal + gc];
    const int nT = info.nTotal, nR = info.nRetain;
    if (nT <= 0) return;
    if (nT <= nLo || nT > nHi) return;                               // this launch's tier: cells with nLo < survivors <= nHi
    const int mode = (cfg->introspection && (use_cost_of(useCost, img) & 1)) ? 1 : 0;
    const uint8_t* Q = mode ? qpyr + (size_t)img * cfg->pyrBytes + G.off : nullptr;
    const unsigned th = info.useMin ? 1u : (unsigned)cfg->iniTh;
    const int kept = (nR >= 0 && nT > nR) ? nR : nT;
    u64* dst = lvlList + (size_t)img * cfg->candTotal + G.candBase + info.prefix;
    if (nT > cap) {                                                  // LDS tiers: the next tier's cell
        if constexpr (STORE::kGlobal) { if (tid == 0) atomicOr(status, 4); }     // cannot happen: cap = max strict maxima per cell
        return;
    }
    // a) collect the cell's survivors from the FAST tiles it overlaps, filtered by its rectangle and threshold
    //    (order irrelevant here)
    const int ci = c / G.cols, cj = c % G.cols;
    const int cx0 = kEdge + cj * G.cellW, cx1 = (cj == G.cols - 1) ? G.maxBX : cx0 + G.cellW;
    const int cy0 = kEdge + ci * G.cellH, cy1 = cy0 + ((ci == G.rows - 1) ? G.domHLast : G.domH[mode]);
    int m = 0;
    if (tid == 0) s_m = 0;
    sync();
    if (cy1 > cy0 && cx1 > cx0) {
        // The gather is a chain of memory round trips (a tile's count, then its list, 64 entries per step): the counts of up to
        // 64 tiles are fetched by one wave-wide load and handed out by lane broadcast, and a tile's list is read four steps at
        // a time (four loads in flight per lane) -- one round trip per tile instead of ~5.  (Measured: 268 -> 263 us per 256 images only -- the kernel's time is the bitonic sort,
        // 41 %, and the introselect replay, 26 %, found by compiling each out.)
        const int tx0 = (cx0 - 16) / kFastTW, tx1 = (cx1 - 1 - 16) / kFastTW;
        const int ty0 = (cy0 - kEdge) / kFastTH, ty1 = (cy1 - 1 - kEdge) / kFastTH;
        const int ntx = tx1 - tx0 + 1, nt = ntx * (ty1 - ty0 + 1);
        const size_t tileBase = (size_t)img * cfg->nTiles + G.tileBase;
        // r04: the lists of up to 64 tiles are read as ONE flattened sequence (a cell of a plain extraction spans 20-30 tiles with a few
        // dozen survivors each: one round trip per tile was 30-40 us of dependent latency per cell).  Lane j holds tile j's count; the
        // exclusive prefix and the tiles' list offsets go to LDS (s_row is free until the sort), every thread finds the tile of its
        // flattened index by a 6-step binary search and U loads per thread are in flight together.
        constexpr int U = 4;
        int* const s_pref = s_row;                // [65]
        int* const s_toff = s_row + 80;           // [64] tile slot index
        for (int t0 = 0; t0 < nt; t0 += 64) {
            int myCnt = 0, myTile = 0;
            if (t0 + lane < nt) {
                const int t = t0 + lane;
                myTile = (ty0 + t / ntx) * G.tilesX + tx0 + t % ntx;
                myCnt = min(tileCnt[tileBase + myTile], kTileCap);
            }
            int incl = myCnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
            const int total = __shfl(incl, 63, 64);
            sync();                               // the previous round's readers are done with s_pref / s_toff
            if (tid < 64) { s_pref[lane] = incl - myCnt; s_toff[lane] = myTile; if (lane == 63) s_pref[64] = total; }
            sync();
            for (int f0 = 0; f0 < total; f0 += NTHR * U) {
                unsigned ev[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int f = f0 + u * NTHR + tid;
                    ev[u] = 0u;                   // score 0 < th: never kept
                    if (f < total) {
                        int j = 0;
#pragma unroll
                        for (int st = 32; st > 0; st >>= 1) if (s_pref[j + st] <= f) j += st;      // s_pref[64] = total > f: j + st <= 63 always holds where it matters
                        ev[u] = tileList[(tileBase + s_toff[j]) * kTileCap + (f - s_pref[j])];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (f0 + u * NTHR >= total) break;               // uniform
                    const unsigned e = ev[u];
                    const int ex = (e >> 8) & 0xfff, ey = e >> 20;
                    const bool keep = (e & 0xffu) >= th && ex >= cx0 && ex < cx1 && ey >= cy0 && ey < cy1;
                    const unsigned long long mask = __ballot(keep);
                    if constexpr (NTHR == 64) {
                        if (keep) {
                            const int idx = m + __popcll(mask & ((1ull << lane) - 1ull));
                            if (idx < cap) keys[idx] = e;
                        }
                        m += __popcll(mask);
                    } else {
                        // order is irrelevant here (the sort restores it): one LDS atomic per wave reserves its slots
                        int base = 0;
                        if (lane == 0 && mask) base = atomicAdd(&s_m, __popcll(mask));
                        base = __shfl(base, 0);
                        if (keep) {
                            const int idx = base + __popcll(mask & ((1ull << lane) - 1ull));
                            if (idx < cap) keys[idx] = e;
                        }
                    }
                }
            }
        }
    }
    if constexpr (NTHR != 64) { sync(); m = s_m; }
    if (tid == 0 && m != nT) atomicOr(status, 1);                    // internal consistency
    if (m != nT) return;
    {
        // b) row-major order of the packed positions (y<<20 | x<<8 | score).  A cell is a few dozen rows with a handful of survivors
        //    each, so a two-level counting sort -- rows by histogram + prefix sum, then every survivor's rank among the survivors
        //    of its own row -- costs O(m * row length) comparisons instead of the bitonic network's m log^2 m (which was 41 % of this
        //    kernel); cells taller than kSelRows rows keep the bitonic sort.  Both give the same list: the packed positions are unique.
        const int nrows = cy1 - cy0;
        if (nrows <= kSelRows) {
            unsigned* arrival = (unsigned*)ord;                      // `ord` is free until step c): arrival index, grouped copy
            unsigned* grouped = arrival + cap;
            for (int r = tid; r <= nrows; r += NTHR) s_row[r] = 0;
            sync();
            for (int k = tid; k < m; k += NTHR) arrival[k] = (unsigned)atomicAdd(&s_row[(int)(keys[k] >> 20) - cy0], 1);
            sync();
            if (tid < 64) {                                          // exclusive prefix sum over the rows, 64 at a time
                int carry = 0;
                for (int b0 = 0; b0 <= nrows; b0 += 64) {
                    const int r = b0 + lane;
                    const int c = r < nrows ? s_row[r] : 0;
                    int incl = c;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                    if (r <= nrows) s_row[r] = carry + incl - c;
                    carry += __shfl(incl, 63, 64);
                }
            }
            sync();
            for (int k = tid; k < m; k += NTHR) { const unsigned e = keys[k]; grouped[s_row[(int)(e >> 20) - cy0] + arrival[k]] = e; }
            sync();
            for (int p = tid; p < m; p += NTHR) {
                const unsigned e = grouped[p];
                const int r = (int)(e >> 20) - cy0;
                const int b = s_row[r], en = s_row[r + 1];
                int rank = 0;
                for (int j = b; j < en; j++) rank += grouped[j] < e ? 1 : 0;      // same row: the order of x (positions are unique)
                keys[b + rank] = e;
            }
            sync();
        } else {
            int n2 = 64;
            while (n2 < m) n2 <<= 1;
            for (int k = m + tid; k < n2; k += NTHR) keys[k] = 0xffffffffu;
            sync();
            for (int k = 2; k <= n2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < n2 / 2; i += NTHR) {
                        const int l = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                        const int r = l | j;
                        const unsigned a = keys[l], b = keys[r];
                        const bool up = (l & k) == 0;
                        if ((a > b) == up) { keys[l] = b; keys[r] = a; }
                    }
                    sync();
                }
        }
        // c) 64-bit keys: response (x quality factor) | y | x
        for (int k = tid; k < m; k += NTHR) {
            const unsigned e = keys[k];
            const unsigned y = e >> 20, x = (e >> 8) & 0xfffu;
            float resp = (float)(e & 0xffu);
            if (mode) {
                const float cost = (float)Q[(size_t)y * G.pitch + x];
                resp *= 2 * (1.0f / (1.0f + cost / 255.0f)) - 1;
            }
            ord[k] = ((u64)__float_as_uint(resp) << 32) | (y << 16) | x;
        }
        sync();
        // d) retainBest (wave 0; the stop lists overlay `keys`, which every wave has finished reading)
        if (nR > 0 && nT > nR && tid < 64) sel_nth_element_wave<typename STORE::WaveSync>(ord, nT, nR - 1 + cfg->varRetain, stopA, stopB, lane);
        sync();
        for (int k = tid; k < kept; k += NTHR) dst[k] = ord[k];
    }
}
// tier 0 (<= kCellCapTiny survivors: in plain ORB extraction every cell): one wave per cell, WPB cells per workgroup -- a quarter of
// the workgroups to dispatch for the same waves in flight
template <int CAP, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_cell_select(const Config* __restrict__ cfg, const unsigned* __restrict__ tileList,
                                                        const int* __restrict__ tileCnt, const CellInfo* __restrict__ cellInfo,
                                                        const uint8_t* __restrict__ qpyr, const uint8_t* __restrict__ useCost,
                                                        u64* __restrict__ lvlList, int* __restrict__ status, int nLo, int nHi)
{
    __shared__ SelShared<CAP> S[WPB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gc = blockIdx.x * WPB + wave;
    if (gc >= cfg->nCellsTotal) return;
    cell_select_one<64>(cfg, tileList, tileCnt, cellInfo, qpyr, useCost, lvlList, status, nLo, nHi, blockIdx.y, gc, threadIdx.x & 63, S[wave]);
}
// tiers 1, 2: the workgroups walk k_quota's work list of this tier (img * nCellsTotal + cell)
template <int CAP, int NTHR>
__global__ __launch_bounds__(NTHR) void k_cell_select_list(const Config* __restrict__ cfg, const unsigned* __restrict__ tileList,
                                                        const int* __restrict__ tileCnt, const CellInfo* __restrict__ cellInfo,
                                                        const uint8_t* __restrict__ qpyr, const uint8_t* __restrict__ useCost,
                                                        u64* __restrict__ lvlList, int* __restrict__ status, int nLo, int nHi,
                                                        const int* __restrict__ count, const int* __restrict__ list, int cap)
{
    __shared__ SelShared<CAP> S;
    const int n = min(*count, cap);
    for (int w = blockIdx.x; w < n; w += gridDim.x) {
        const int e = list[w];
        cell_select_one<NTHR>(cfg, tileList, tileCnt, cellInfo, qpyr, useCost, lvlList, status, nLo, nHi, e / cfg->nCellsTotal, e % cfg->nCellsTotal,
                              threadIdx.x, S);
        sel_sync<NTHR, SyncLds>();
    }
}
// Cells with more than kCellCapBig survivors: the same walk over k_quota's third list with every list of the cell in a global
// scratch slot of slotCap survivors (one slot per workgroup, kHugeSlots workgroups).  Rare by construction -- it exists so that
// such an image costs time instead of an error.  1024 threads gather and sort; wave 0 replays the introselect.
constexpr int kHugeThreads = 1024;
__global__ __launch_bounds__(kHugeThreads) void k_cell_select_huge(const Config* __restrict__ cfg, const unsigned* __restrict__ tileList,
                                                                  const int* __restrict__ tileCnt, const CellInfo* __restrict__ cellInfo,
                                                                  const uint8_t* __restrict__ qpyr, const uint8_t* __restrict__ useCost,
                                                                  u64* __restrict__ lvlList, int* __restrict__ status,
                                                                  const int* __restrict__ hugeCount, const int* __restrict__ hugeList,
                                                                  unsigned* __restrict__ scratch, int slotCap)
{
    __shared__ SelCounts counts;
    unsigned* const keys = scratch + (size_t)blockIdx.x * ((size_t)slotCap * 4);
    SelGlobal S{keys, (u64*)(keys + 2 * (size_t)slotCap), counts, slotCap};
    const int n = min(*hugeCount, kHugeListCap);
    for (int w = blockIdx.x; w < n; w += gridDim.x) {
        const int e = hugeList[w];
        cell_select_one<kHugeThreads>(cfg, tileList, tileCnt, cellInfo, qpyr, useCost, lvlList, status, kCellCapBig, 0x7fffffff, e / cfg->nCellsTotal,
                                      e % cfg->nCellsTotal, threadIdx.x, S);
        __syncthreads();                                 // this cell done with the slot and the counts
    }
}
__global__ __launch_bounds__(256) void k_level_select(const Config* __restrict__ cfg, const int* __restrict__ lvlTotal,
                                                     u64* __restrict__ lvlList, unsigned* __restrict__ slotPos,
                                                     float* __restrict__ slotResp, int* __restrict__ lvlCount, int LCAP)
{
    // r06: the LDS copy of a level's list is sized by the launch (LCAP = four times the largest nDesired of the geometry, at most 4096; a longer list takes the
    // global path below as before) instead of 4096 entries = 49 KB per workgroup = three workgroups per CU for 2,048 (level, image) workgroups
    extern __shared__ __attribute__((aligned(16))) u64 s_list[];
    unsigned short* const s_stopA = (unsigned short*)(s_list + LCAP);
    unsigned short* const s_stopB = s_stopA + LCAP;
    const int img = blockIdx.y, level = blockIdx.x, tid = threadIdx.x;
    const LevelGeom& G = cfg->lv[level];
    if (!G.valid) { if (tid == 0) lvlCount[img * kMaxLevels + level] = 0; return; }
    int total = lvlTotal[img * kMaxLevels + level];
    u64* Lg = lvlList + (size_t)img * cfg->candTotal + G.candBase;
    u64* L = Lg;
    if (total > G.nDesired) {
        if (total <= LCAP) {
            for (int k = tid; k < total; k += 256) s_list[k] = Lg[k];
            L = s_list;
            __syncthreads();
        }
        if (L == s_list) { if (tid < 64) sel_nth_element_wave<SyncLds>(s_list, total, G.nDesired - 1 + cfg->varRetain, s_stopA, s_stopB, tid); }
        else if (tid == 0) sel_nth_element(L, total, G.nDesired - 1 + cfg->varRetain);   // :1162-1166 (global fallback)
        total = G.nDesired;
        __syncthreads();
    }
    for (int k = tid; k < total; k += 256) {
        const u64 e = L[k];
        slotPos[(size_t)img * cfg->nfeatures + G.kpBase + k] = (unsigned)e;
        slotResp[(size_t)img * cfg->nfeatures + G.kpBase + k] = __uint_as_float((unsigned)(e >> 32));
    }
    if (tid == 0) lvlCount[img * kMaxLevels + level] = total;
}

// testing hook: the device's retainBest on caller-supplied responses, so the introselect replays can be checked against libstdc++
// on arbitrary / adversarial inputs.  n <= kCellCapBig: the wave-cooperative replay on LDS lists, as the tier kernels and
// k_level_select run it.  Longer: the lists in global memory (lists: u64[2 * n] keys, u32[2 * n] stops) -- the wave-cooperative
// replay with the workgroup fence, as the huge tier runs it, and k_level_select's one-thread replay on a copy of the same keys;
// *differ is set where the two orders disagree.
__global__ __launch_bounds__(64) void k_test_retain_best(const float* __restrict__ resp, int n, int nPoints, int* __restrict__ order,
                                                        u64* __restrict__ lists, int* __restrict__ differ)
{
    __shared__ __attribute__((aligned(16))) u64 list[kCellCapBig];
    __shared__ unsigned short sa[kCellCapBig], sb[kCellCapBig];
    const int lane = threadIdx.x;
    const bool select = nPoints > 0 && n > nPoints;
    if (n <= kCellCapBig) {
        for (int i = lane; i < n; i += 64) list[i] = ((u64)__float_as_uint(resp[i]) << 32) | (unsigned)i;
        wave_sync_lds();
        if (select) sel_nth_element_wave<SyncLds>(list, n, nPoints - 1, sa, sb, lane);
        for (int i = lane; i < n; i += 64) order[i] = (int)(unsigned)list[i];
        return;
    }
    u64* const byWave = lists;
    u64* const byOne = lists + n;
    unsigned* const ga = (unsigned*)(lists + 2 * (size_t)n);
    for (int i = lane; i < n; i += 64) byWave[i] = byOne[i] = ((u64)__float_as_uint(resp[i]) << 32) | (unsigned)i;
    SyncGlobal()();
    if (select) {
        sel_nth_element_wave<SyncGlobal>(byWave, n, nPoints - 1, ga, ga + n, lane);
        if (lane == 0) sel_nth_element(byOne, n, nPoints - 1);
        SyncGlobal()();
    }
    for (int i = lane; i < n; i += 64) {
        order[i] = (int)(unsigned)byWave[i];
        if (byWave[i] != byOne[i]) *differ = 1;
    }
}
void launch_test_retain_best(const float* dResp, int n, int nPoints, int* dOrder, unsigned long long* dLists, int* dDiffer, hipStream_t s)
{
    hipLaunchKernelGGL(k_test_retain_best, dim3(1), dim3(64), 0, s, dResp, n, nPoints, dOrder, dLists, dDiffer);
}

void launch_select(const Config& hc, const Config* dc, const Buffers& b, int nImg, hipStream_t s)
{
    if (hc.introspection)
        hipLaunchKernelGGL(k_cell_qsum, dim3((hc.nCellsTotal + 3) / 4, nImg), dim3(256), 0, s, dc, b.qpyr, b.useCost, b.cellInfo);
    const int tierCap = nImg * hc.nCellsTotal;
    int cap = 4;
    for (int l = 0; l < hc.nlevels; l++) cap = std::max(cap, (hc.lv[l].nCells + 3) & ~3);
    const size_t quotaLds = (size_t)cap * (7 * 4 + 1) + 64;                     // six int / float arrays + the prefix's tail + the byte flags (k_quota)
    hipLaunchKernelGGL(k_quota, dim3(hc.nlevels, nImg), dim3(256), quotaLds, s, dc, b.cellCnt, b.qpyr, b.useCost,
                       b.cellInfo, b.lvlTotal, b.hugeCount, b.hugeList, b.tierList, tierCap, b.status, cap);
    // three tiers by survivor count: the kernel is a chain of dependent LDS steps at one wave per cell, so its throughput is the
    // number of cells in flight per CU = LDS per workgroup: 5 KB (<= 256 survivors), 14 KB (<= 1024), 51 KB (<= 4096, four waves; a 2048 tier of two waves measured slower: 77 + 42 vs 109 us)
    // r04: tier 0 four cells per workgroup; tiers 1 / 2 from k_quota's work lists with a fixed grid (a full grid per tier cost 80-110 us
    // of workgroup dispatch per launch even when the tier was empty, as it is for every cell of a plain ORB extraction)
    constexpr int kSelWPB = 4;
    hipLaunchKernelGGL((k_cell_select<kCellCapTiny, kSelWPB>), dim3((hc.nCellsTotal + kSelWPB - 1) / kSelWPB, nImg), dim3(64 * kSelWPB), 0, s, dc,
                       b.tileList, b.tileCnt, b.cellInfo, b.qpyr, b.useCost, b.lvl, b.status, 0, kCellCapTiny);
    const int gridList = std::max(1, std::min(tierCap, 8192));
    hipLaunchKernelGGL((k_cell_select_list<kCellCapSmall, 64>), dim3(gridList), dim3(64), 0, s, dc, b.tileList, b.tileCnt,
                       b.cellInfo, b.qpyr, b.useCost, b.lvl, b.status, kCellCapTiny, kCellCapSmall, b.hugeCount + 1, b.tierList, tierCap);
    hipLaunchKernelGGL((k_cell_select_list<kCellCapBig, 256>), dim3(std::min(gridList, 2048)), dim3(256), 0, s, dc, b.tileList, b.tileCnt,
                       b.cellInfo, b.qpyr, b.useCost, b.lvl, b.status, kCellCapSmall, kCellCapBig, b.hugeCount + 2,
                       b.tierList + tierCap, tierCap);
    if (b.hugeScratch)       // geometry allows cells with more than kCellCapBig strict maxima: walk k_quota's (usually empty) list
        hipLaunchKernelGGL(k_cell_select_huge, dim3(kHugeSlots), dim3(kHugeThreads), 0, s, dc, b.tileList, b.tileCnt, b.cellInfo,
                           b.qpyr, b.useCost, b.lvl, b.status, b.hugeCount, b.hugeList, b.hugeScratch, hc.maxCandCap);
    int maxDesired = 1;
    for (int l = 0; l < hc.nlevels; l++) maxDesired = std::max(maxDesired, hc.lv[l].nDesired);
    const int lcap = std::min(4096, (4 * maxDesired + 256 + 63) & ~63);
    hipLaunchKernelGGL(k_level_select, dim3(hc.nlevels, nImg), dim3(256), (size_t)lcap * 12, s, dc, b.lvlTotal, b.lvl, b.slotPos, b.slotResp,
                       b.lvlCount, lcap);
}

}  // namespace ivf
