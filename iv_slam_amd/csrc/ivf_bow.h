// ivf_bow.h -- the one device text of everything the three BoW units repeat: the per-call DBoW2 transform (ivf_match.hip, which alone
// knows struct ivf_vocabulary), the batched TrackReferenceKeyFrame matcher (ivf_track_bow.hip) and the batched mBowVec / relocalization
// candidates (ivf_track_db.hip).  The vocabulary-tree descent of one descriptor and of one record slot, the view through which the tracker's
// units reach the vocabulary, the sort of unique 64-bit keys with its run starts, the lookup in an ascending list, and the
// kernel-argument struct of the tracker handle's feature-vector scratch.
#pragma once
#include "ivf_grid.h"

namespace ivf {

// DBoW2 vocabulary-tree descent (TemplatedVocabulary.h:1217-1259) of ONE descriptor by 16 consecutive lanes (sub = lane & 15): one child
// per lane per round, (distance << 16 | position) min-reduction across the 16 lanes = "first minimum in child order" (at most 65535
// children under a node: ivf_vocabulary_create).  All 16 lanes must hold the same descriptor; every lane returns the leaf and the node
// passed at level nidLevel (0 when the leaf lies above that level; the caller maps nidLevel <= 0 to the root).
__device__ __forceinline__ void bow_descend(const int* __restrict__ childStart, const int* __restrict__ child, const uint8_t* __restrict__ nodeDesc,
                                            const uint4 a0, const uint4 a1, int sub, int nidLevel, int& leaf, int& nid)
{
    int node = 0, level = 0;
    nid = 0;
    for (;;) {
        const int c0 = childStart[node], c1 = childStart[node + 1];
        if (c1 == c0) break;                                              // leaf (uniform within the 16 lanes)
        ++level;
        unsigned best = 0xffffffffu;
        for (int c = c0 + sub; c < c1; c += 16) {
            const int id = child[c];
            const uint4* pn = (const uint4*)(nodeDesc + (size_t)id * 32);
            const unsigned key = ((unsigned)hamming256(a0, a1, pn[0], pn[1]) << 16) | (unsigned)(c - c0);
            best = min(best, key);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 16));
        node = child[c0 + (int)(best & 0xffffu)];
        if (level == nidLevel) nid = node;
    }
    leaf = node;
}

// ... of the keypoints of ONE record slot by one 256-thread workgroup, 16 keypoints per workgroup: keypoint f = 16 * block + tid / 16 of
// the n descriptors at desc.  A workgroup past the end returns at once; a dead lane group of the last one descends with keypoint 0's
// descriptor (no divergence inside the descent) and stores nothing; lane sub == 0 of a live keypoint calls store(f, leaf, nid), nid
// already mapped to the root where nidLevel <= 0.
template <class Store>
DEVINL void bow_descend_slot(const int* __restrict__ childStart, const int* __restrict__ child, const uint8_t* __restrict__ nodeDesc,
                             const uint8_t* __restrict__ desc, int n, int block, int nidLevel, Store store)
{
    if (block * 16 >= n) return;
    const int f = block * 16 + ((int)threadIdx.x >> 4), sub = threadIdx.x & 15;
    const bool live = f < n;
    const uint4* pf = (const uint4*)(desc + (size_t)(live ? f : 0) * 32);
    const uint4 a0 = pf[0], a1 = pf[1];
    int leaf, nid;
    bow_descend(childStart, child, nodeDesc, a0, a1, sub, nidLevel, leaf, nid);
    if (live && sub == 0) store(f, leaf, nidLevel <= 0 ? 0 : nid);
}

// what ivf_track_bow.hip and ivf_track_db.hip need of a vocabulary: the tree in HBM and, per node, the word id and the weight as
// ivf_vocabulary_create received them (mBowVec) and wordLive = weight > 0
struct VocabularyView {
    int device, nNodes, depth;
    const int *childStart, *child;
    const uint8_t *nodeDesc, *wordLive;
    const int* nodeWord;
    const double* nodeWeight;
};
int vocabulary_view(const ivf_vocabulary* v, VocabularyView* out);
// a stopped word (weight 0) adds neither to mBowVec nor to mFeatVec (TemplatedVocabulary.h:1157: `if(w > 0)`): the one question of it,
// one byte instead of the f64 weight
DEVINL bool word_live(const VocabularyView& V, int leaf) { return V.wordLive[leaf] != 0; }

// ---- the stable sort of up to npad ids in LDS as unique 64-bit keys (id << 32 | index), and the runs of equal ids in the result.
// npad: the power of two >= max(n, 256) the bitonic network runs on (n <= nfeatures <= 4096: at most 32 KB of keys), for the launch
// (n = nfeatures, with the bytes of the key array) and for the workgroup (n = the record's count) alike
__host__ __device__ inline unsigned key_sort_pad(int n, size_t* ldsBytes = nullptr)
{
    unsigned npad = 256;
    while ((int)npad < n) npad <<= 1;
    if (ldsBytes) *ldsBytes = (size_t)npad * sizeof(unsigned long long);
    return npad;
}
// what the sort leaves to an epilogue: the first m sorted keys are live; this thread owns positions j0 .. j0 + per - 1, the first run
// that starts among them is run k of total()
struct KeyRuns {
    const unsigned long long* key; const int* part;
    int m, per, j0, k;
    DEVINL unsigned id(int j) const { return (unsigned)(key[j] >> 32); }
    DEVINL bool starts(int j) const { return j < m && (j == 0 || id(j - 1) != id(j)); }
    DEVINL int total() const { return part[255]; }
};
constexpr unsigned long long kNoKey = ~0ull;                 // padding / an element that takes no part: behind every live key
DEVINL unsigned long long sort_key(int id, unsigned i) { return ((unsigned long long)(unsigned)id << 32) | i; }
// One 256-thread workgroup: key(i) -> sort_key(id of element i < n, i), or kNoKey when the element takes no part.  The keys are unique,
// so sorting them is the stable sort of the ids: std::map order with the elements of one id in index order.  part [256]: the scan of
// the run starts per thread.
template <class Key>
DEVINL KeyRuns sort_keys_and_runs(unsigned long long* s_key, unsigned npad, int n, int tid, Key key, int* part)
{
    __shared__ int s_m;
    if (tid == 0) s_m = 0;
    __syncthreads();
    int mine = 0;
    for (unsigned i = tid; i < npad; i += 256) {
        const unsigned long long k = (int)i < n ? key(i) : kNoKey;
        mine += k != kNoKey ? 1 : 0;
        s_key[i] = k;
    }
    atomicAdd(&s_m, mine);
    __syncthreads();
    for (unsigned k = 2; k <= npad; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = tid; t < npad / 2; t += 256) {
                const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = s_key[i], b = s_key[l];
                if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[l] = a; }
            }
            __syncthreads();
        }
    KeyRuns R{s_key, part, s_m, (int)(npad >> 8), 0, 0};
    R.j0 = tid * R.per;
    int cnt = 0;
    for (int j = R.j0; j < R.j0 + R.per; j++) cnt += R.starts(j) ? 1 : 0;
    part[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    R.k = part[tid] - cnt;
    return R;
}

// ---- position of v in the ascending list s[0 .. n), or -1.  Ids (nodes, words) are non-negative and the lists come out of the sort
// above, which orders them as unsigned: the compare is unsigned too.
DEVINL int sorted_find(const int* s, int n, int v)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((unsigned)s[mid] < (unsigned)v) lo = mid + 1; else hi = mid; }
    return lo < n && s[lo] == v ? lo : -1;
}

// The handle's scratch of ivf_tracker_search_by_bow (struct ivf_tracker, ivf_tracker.h), allocated by ivf_tracker_create: slot s = 2 * pair + side (0 = keyframe, 1 = current
// frame).  nodeKey [slots][nf]: node id per keypoint (-1: stopped word); the feature vector in CSR form: fvNode [slots][nf] ascending,
// fvStart [slots][nf + 1], fvIdx [slots][nf] ascending inside a node, fvN [slots] nodes.
struct TrackerBowScratch { int *nodeKey, *fvNode, *fvStart, *fvIdx, *fvN; };
// slot s of that scratch from its nodeKey row, by one 256-thread workgroup: the n keypoints of the slot's record sorted into std::map
// order of the nodes with addFeature's push order inside a node (FeatureVector.cpp:31-45).  s_key [key_sort_pad(n)] and part [256] in LDS.
DEVINL void featvec_of_slot(const TrackerBowScratch& B, int s, int nf, int n, unsigned long long* s_key, int* part, int tid)
{
    const int* keyIn = B.nodeKey + (size_t)s * nf;
    const KeyRuns R = sort_keys_and_runs(s_key, key_sort_pad(n), n, tid, [&](unsigned i) { const int k = keyIn[i]; return k >= 0 ? sort_key(k, i) : kNoKey; }, part);
    int k = R.k;
    int* nodeOut = B.fvNode + (size_t)s * nf;
    int* startOut = B.fvStart + (size_t)s * (nf + 1);
    int* idxOut = B.fvIdx + (size_t)s * nf;
    for (int j = R.j0; j < R.j0 + R.per; j++) {
        if (j >= R.m) break;
        idxOut[j] = (int)(unsigned)s_key[j];
        if (R.starts(j)) { nodeOut[k] = (int)R.id(j); startOut[k] = j; k++; }
    }
    if (tid == 0) { const int total = R.total(); startOut[total] = R.m; B.fvN[s] = total; }
}

}  // namespace ivf
