// ivf_bow.h -- what the per-call DBoW2 transform (ivf_match.hip, which alone knows struct ivf_vocabulary) and the batched
// TrackReferenceKeyFrame matcher (ivf_track_bow.hip) share, and with them the batched mBowVec of ivf_track_db.hip: the one device text of
// the vocabulary-tree descent, the view through which the tracker's units reach the vocabulary, and the kernel-argument struct of the
// tracker handle's feature-vector scratch.
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

// what ivf_track_bow.hip and ivf_track_db.hip need of a vocabulary: the tree in HBM and, per node, whether a descriptor that ends there
// enters the feature vector at all (weight > 0: TemplatedVocabulary.h:1157 skips stopped words); for mBowVec (ivf_track_db.hip) the word
// id and the weight of every node as ivf_vocabulary_create received them
struct VocabularyView {
    int device, nNodes, depth;
    const int *childStart, *child;
    const uint8_t *nodeDesc, *wordLive;
    const int* nodeWord;
    const double* nodeWeight;
};
int vocabulary_view(const ivf_vocabulary* v, VocabularyView* out);

// The handle's scratch of ivf_tracker_search_by_bow (struct ivf_tracker, ivf_tracker.h), allocated by ivf_tracker_create: slot s = 2 * pair + side (0 = keyframe, 1 = current
// frame).  nodeKey [slots][nf]: node id per keypoint (-1: stopped word); the feature vector in CSR form: fvNode [slots][nf] ascending,
// fvStart [slots][nf + 1], fvIdx [slots][nf] ascending inside a node, fvN [slots] nodes.
struct TrackerBowScratch { int *nodeKey, *fvNode, *fvStart, *fvIdx, *fvN; };

}  // namespace ivf
