// ivf_track_create.hip -- batched, device-resident LocalMapping::CreateNewMapPoints (ORB/src/LocalMapping.cc:273-525), stereo / RGB-D
// branch, on the tracker handle (ivf_tracker.h): for every current keyframe of a batch and each of its covisible neighbours in rank order
//   * the baseline gate (:311-319), LocalMapping::ComputeF12 (:609-626) and the epipole (ORB/src/ORBmatcher.cc:670-676);
//   * KeyFrame::ComputeBoW reduced to mFeatVec, as ivf_track_bow.hip computes it, and ORBmatcher(0.6, false).SearchForTriangulation
//     (ORBmatcher.cc:663-829; mbCheckOrientation is false there, bOnlyStereo too);
//   * per match the parallax decision, the 4x4 linear triangulation or Frame::UnprojectStereo, the two depth signs, the two reprojection
//     gates and the scale-consistency gate (:352-497);
//   * the new point's record: MapPoint(x3D, ...), ComputeDistinctiveDescriptors and UpdateNormalAndDepth for two observations
//     (ORB/src/MapPoint.cc:247-376) and IV-SLAM's SetQualityScore(min(mvKeyQualScore[idx1], mvKeyQualScore[idx2])) (:512-517).
// Nothing crosses PCIe.  The frozen arithmetic is DESIGN.md section 3 "CreateNewMapPoints"; tests/create_points_ref.py restates it.
//
// Kernels (gfx950, wave = 64; no workgroup waits for another, every loop is bounded by nfeatures, the node count or max_neigh):
//   k_create_nodes    every record slot (keyframe k: slot k * (1 + max_neigh), its neighbour r: + 1 + r) through bow_descend_slot
//   k_create_featvec  one workgroup per slot: featvec_of_slot (ivf_bow.h) -> the CSR feature vector in the handle's scratch
//   k_create_points   one workgroup (8 waves) per keyframe walks the neighbour ranks: the ranks of one keyframe depend on each other
//                     (a keypoint that received a point is skipped by the later ranks, AddMapPoint then ORBmatcher.cc:708), the
//                     keypoints of one rank do not (vbMatched2 is tested and never set).  Per rank: node merge; a wave takes one
//                     current keypoint at a time with the neighbour's features of the node across its lanes, every gate per lane, the
//                     LAST equal minimum (last_min_key, ivf_search.h); vMatchedIndices by compact_ordered; one lane per match runs
//                     the triangulation with its 4x4 Jacobi in registers (jacobi_rotation, ivf_solve.h); the created points are
//                     ranked in match order by a second compact_ordered.
#include "ivf_search.h"
#include "ivf_solve.h"

using namespace ivf;

namespace {

constexpr int kCreateThreads = 512;

struct CreateParams {
    TrackParams T;
    float sigma2[kMaxLevels];                                  // mvLevelSigma2
    float ratioFactor;                                         // 1.5f * mfScaleFactor (LocalMapping.cc:298)
    int nidLevel, maxNeigh;
};

// the record of slot s, or null: j == 0 the keyframe, else neighbour j - 1
DEVINL const uint8_t* slot_record(const CreateParams& P, const uint8_t* __restrict__ records, const int* __restrict__ kf, const int* __restrict__ neigh, int s)
{
    const int k = s / (1 + P.maxNeigh), j = s - k * (1 + P.maxNeigh);
    const int r = j == 0 ? kf[k] : neigh[(size_t)k * P.maxNeigh + (j - 1)];
    return rec_ok(P.T.nRecords, r) ? records + (size_t)r * P.T.recBytes : nullptr;
}

__global__ __launch_bounds__(256) void k_create_nodes(CreateParams P, VocabularyView V, const uint8_t* __restrict__ records, const int* __restrict__ kf,
                                                     const int* __restrict__ neigh, int* __restrict__ nodeKey)
{
    const int s = blockIdx.y;
    const uint8_t* rec = slot_record(P, records, kf, neigh, s);
    if (!rec) return;
    bow_descend_slot(V.childStart, V.child, V.nodeDesc, rec_desc(rec, P.T.nf), rec_count(rec, P.T.nf), blockIdx.x, P.nidLevel,
                     [&](int f, int leaf, int nid) { nodeKey[(size_t)s * P.T.nf + f] = word_live(V, leaf) ? nid : -1; });
}

__global__ __launch_bounds__(256) void k_create_featvec(CreateParams P, const uint8_t* __restrict__ records, const int* __restrict__ kf,
                                                       const int* __restrict__ neigh, TrackerBowScratch B)
{
    extern __shared__ unsigned long long s_key[];             // [npad]: node id << 32 | feature index
    __shared__ int part[256];
    const int s = blockIdx.x;
    const uint8_t* rec = slot_record(P, records, kf, neigh, s);
    if (!rec) return;
    featvec_of_slot(B, s, P.T.nf, rec_count(rec, P.T.nf), s_key, part, threadIdx.x);
}

// cv::Mat::dot / cv::norm on CV_32F: double accumulation, left to right
DEVINL double dot3(const float* a, const float* b) { return (double)a[0] * (double)b[0] + (double)a[1] * (double)b[1] + (double)a[2] * (double)b[2]; }
DEVINL double norm3(const float* a) { return sqrt(dot3(a, a)); }

// LocalMapping::ComputeF12 (:609-626) in closed form, f64 from the float poses and intrinsics, narrowed once
DEVINL void compute_f12(const TrackParams& T, const float* R1f, const float* t1f, const float* R2f, const float* t2f, float* F12)
{
    double R1[9], R2[9], t1[3], t2[3], R12[9], t12[3], E[9], M[9];
    for (int i = 0; i < 9; i++) { R1[i] = (double)R1f[i]; R2[i] = (double)R2f[i]; }
    for (int i = 0; i < 3; i++) { t1[i] = (double)t1f[i]; t2[i] = (double)t2f[i]; }
    const double fx = (double)T.fx, fy = (double)T.fy, cx = (double)T.cx, cy = (double)T.cy;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R12[3 * i + j] = R1[3 * i] * R2[3 * j] + R1[3 * i + 1] * R2[3 * j + 1] + R1[3 * i + 2] * R2[3 * j + 2];
    for (int i = 0; i < 3; i++) t12[i] = t1[i] - (R12[3 * i] * t2[0] + R12[3 * i + 1] * t2[1] + R12[3 * i + 2] * t2[2]);
    for (int j = 0; j < 3; j++) {
        E[j] = t12[1] * R12[6 + j] - t12[2] * R12[3 + j];
        E[3 + j] = t12[2] * R12[j] - t12[0] * R12[6 + j];
        E[6 + j] = t12[0] * R12[3 + j] - t12[1] * R12[j];
    }
    for (int j = 0; j < 3; j++) {                              // K1^-T E
        M[j] = E[j] / fx; M[3 + j] = E[3 + j] / fy;
        M[6 + j] = (E[6 + j] - cx * M[j]) - cy * M[3 + j];
    }
    for (int i = 0; i < 3; i++) {                              // ... K2^-1
        const double f0 = M[3 * i] / fx, f1 = M[3 * i + 1] / fy;
        F12[3 * i] = (float)f0; F12[3 * i + 1] = (float)f1; F12[3 * i + 2] = (float)((M[3 * i + 2] - cx * f0) - cy * f1);
    }
}

// cos(2 atan2(b / 2, depth)) (:378, :380) as (d^2 - h^2) / (d^2 + h^2), h = b / 2, in f64, narrowed
DEVINL float stereo_cos(float b, float depth)
{
    const double h = (double)b * 0.5, d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

// the right singular vector of the smallest singular value of the row-major 4x4 A, in registers: every index is a compile-time constant
DEVINL void jacobi_smallest4(const float* Af, float* v)
{
    double A[16], V[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { A[i] = (double)Af[i]; V[i] = (i >> 2) == (i & 3) ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) { const double x = A[4 * k + p], y = A[4 * k + q]; a = a + x * x; b = b + y * y; g = g + x * y; }
                double c, s;
                if (!jacobi_rotation(a, b, g, c, s)) continue;
                rotated = true;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double x = A[4 * k + p], y = A[4 * k + q];
                    A[4 * k + p] = c * x - s * y; A[4 * k + q] = s * x + c * y;
                    const double vx = V[4 * k + p], vy = V[4 * k + q];
                    V[4 * k + p] = c * vx - s * vy; V[4 * k + q] = s * vx + c * vy;
                }
            }
        if (!rotated) break;
    }
    double wBest = 0.0, vb[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; j++) {                              // the last of the descending, stable order: ties go to the larger column
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const double x = A[4 * k + j]; a = a + x * x; }
        const double w = sqrt(a);
        if (j == 0 || w <= wBest) {
            wBest = w;
#pragma unroll
            for (int k = 0; k < 4; k++) vb[k] = V[4 * k + j];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (float)vb[k];
}

// one reprojection gate (:428-479): false = refused; stereo: the keypoint has a right coordinate
DEVINL bool reprojection_ok(const CreateParams& P, const float* R, const float* t, const float* x3D, float z, const ivf_keypoint& kp, float ur, bool stereo)
{
    const float sigmaSquare = P.sigma2[clamp_octave(kp.octave)];
    const float x = (float)(dot3(R, x3D) + (double)t[0]), y = (float)(dot3(R + 3, x3D) + (double)t[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = P.T.fx * x * invz + P.T.cx, v = P.T.fy * y * invz + P.T.cy;
    const float errX = u - kp.x, errY = v - kp.y;
    if (!stereo) return !((double)(errX * errX + errY * errY) > 5.991 * (double)sigmaSquare);
    const float u_r = u - P.T.bf * invz;
    const float errX_r = u_r - ur;
    return !((double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)sigmaSquare);
}

struct Side { const float *R, *t, *Ow; ivf_keypoint kp; float ur, depth; };

// LocalMapping.cc:352-497 for one match -> the stage code; on a created point x3D, normal1 / normal2 (x3D - Ow) and dist1 / dist2
DEVINL int triangulate(const CreateParams& P, const Side& s1, const Side& s2, float* x3D, float* normal1, float* normal2, float& dist1, float& dist2)
{
    const TrackParams& T = P.T;
    const bool bStereo1 = s1.ur >= 0, bStereo2 = s2.ur >= 0;
    const float xn1[3] = {(s1.kp.x - T.cx) * T.invfx, (s1.kp.y - T.cy) * T.invfy, 1.0f};
    const float xn2[3] = {(s2.kp.x - T.cx) * T.invfx, (s2.kp.y - T.cy) * T.invfy, 1.0f};
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float Rwc1[9], Rwc2[9], ray1[3], ray2[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { Rwc1[3 * i + j] = s1.R[3 * j + i]; Rwc2[3 * i + j] = s2.R[3 * j + i]; }
    mul_add(Rwc1, xn1, zero, ray1);
    mul_add(Rwc2, xn2, zero, ray2);
    const float cosParallaxRays = (float)(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = stereo_cos(T.b, s1.depth);
    else if (bStereo2) cosParallaxStereo2 = stereo_cos(T.b, s2.depth);
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;
    int made;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        float A[16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float a2 = j < 3 ? s1.R[6 + j] : s1.t[2], a0 = j < 3 ? s1.R[j] : s1.t[0], a1 = j < 3 ? s1.R[3 + j] : s1.t[1];
            const float b2 = j < 3 ? s2.R[6 + j] : s2.t[2], b0 = j < 3 ? s2.R[j] : s2.t[0], b1 = j < 3 ? s2.R[3 + j] : s2.t[1];
            A[j] = xn1[0] * a2 - a0; A[4 + j] = xn1[1] * a2 - a1; A[8 + j] = xn2[0] * b2 - b0; A[12 + j] = xn2[1] * b2 - b1;
        }
        float v[4];
        jacobi_smallest4(A, v);
        if (v[3] == 0) return IVF_CREATE_W_ZERO;
        x3D[0] = v[0] / v[3]; x3D[1] = v[1] / v[3]; x3D[2] = v[2] / v[3];
        made = IVF_CREATE_BY_SVD;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        unproject_stereo(T, s1.R, s1.t, s1.kp, s1.depth, x3D);
        made = IVF_CREATE_BY_STEREO1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        unproject_stereo(T, s2.R, s2.t, s2.kp, s2.depth, x3D);
        made = IVF_CREATE_BY_STEREO2;
    } else
        return IVF_CREATE_LOW_PARALLAX;
    const float z1 = (float)(dot3(s1.R + 6, x3D) + (double)s1.t[2]);
    if (z1 <= 0) return IVF_CREATE_Z1;
    const float z2 = (float)(dot3(s2.R + 6, x3D) + (double)s2.t[2]);
    if (z2 <= 0) return IVF_CREATE_Z2;
    if (!reprojection_ok(P, s1.R, s1.t, x3D, z1, s1.kp, s1.ur, bStereo1)) return bStereo1 ? IVF_CREATE_CHI2_1_STEREO : IVF_CREATE_CHI2_1_MONO;
    if (!reprojection_ok(P, s2.R, s2.t, x3D, z2, s2.kp, s2.ur, bStereo2)) return bStereo2 ? IVF_CREATE_CHI2_2_STEREO : IVF_CREATE_CHI2_2_MONO;
#pragma unroll
    for (int i = 0; i < 3; i++) { normal1[i] = x3D[i] - s1.Ow[i]; normal2[i] = x3D[i] - s2.Ow[i]; }
    dist1 = (float)norm3(normal1); dist2 = (float)norm3(normal2);
    if (dist1 == 0 || dist2 == 0) return IVF_CREATE_DIST_ZERO;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = T.scale[clamp_octave(s1.kp.octave)] / T.scale[clamp_octave(s2.kp.octave)];
    if (ratioDist * P.ratioFactor < ratioOctave) return IVF_CREATE_RATIO_LOW;
    if (ratioDist > ratioOctave * P.ratioFactor) return IVF_CREATE_RATIO_HIGH;
    return made;
}

struct CreateOut {
    ivf_local_point* point; int *neigh, *idx2, *order; float* quality; int* nNew;
    int* matches; uint8_t* stage;                              // nullable
};

__global__ __launch_bounds__(kCreateThreads) void k_create_points(CreateParams P, const uint8_t* __restrict__ records, const int* __restrict__ kfs,
                                                                 const int* __restrict__ neighs, const float* __restrict__ poses,
                                                                 const uint8_t* __restrict__ hasPoint, const float* __restrict__ keyQuality,
                                                                 const float* __restrict__ F12In, const int* __restrict__ kfOrder, TrackerBowScratch B,
                                                                 CreateOut O)
{
    extern __shared__ int s_mem[];
    const int nf = P.T.nf;
    int* s_match = s_mem;                                      // [nf] vMatches12 of this rank
    int* s_list = s_mem + nf;                                  // [nf] the common nodes (keyframe position | neighbour position << 12), then vMatchedIndices' idx1
    uint8_t* s_has = (uint8_t*)(s_mem + 2 * nf);               // [nf] GetMapPoint(idx1) != NULL, the keyframe's working copy
    uint8_t* s_stage = s_has + nf;                             // [nf] the stage code of this rank by idx1
    __shared__ int s_wcnt[kCreateThreads / 64];
    __shared__ int s_nCommon, s_next, s_pos[2];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int kf = kfs[k];
    const size_t row = (size_t)k * nf;
    const bool live = rec_ok(P.T.nRecords, kf);
    {   // the dense outputs: no point anywhere
        uint4* pz = (uint4*)(O.point + row);
        for (int i = tid; i < nf * 5; i += kCreateThreads) pz[i] = make_uint4(0, 0, 0, 0);
        for (int i = tid; i < nf; i += kCreateThreads) { O.neigh[row + i] = -1; O.idx2[row + i] = -1; O.order[row + i] = -1; O.quality[row + i] = 0.0f; }
    }
    const uint8_t* rec1 = live ? records + (size_t)kf * P.T.recBytes : nullptr;
    const int n1 = live ? rec_count(rec1, nf) : 0;
    for (int i = tid; i < nf; i += kCreateThreads) s_has[i] = i < n1 ? (uint8_t)(hasPoint[(size_t)kf * nf + i] != 0) : (uint8_t)1;
    float R1[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t1[3] = {0, 0, 0}, Ow1[3];
    if (live) load_pose(poses + (size_t)kf * 12, R1, t1);
    neg_rt_mul(R1, t1, Ow1);
    const size_t s1 = (size_t)k * (1 + P.maxNeigh);
    int nnew = 0;
    for (int r = 0; r < P.maxNeigh; r++) {
        const size_t drow = ((size_t)k * P.maxNeigh + r) * nf;
        const int nb = neighs[(size_t)k * P.maxNeigh + r];
        int rowStage = -1;                                     // >= 0: the neighbour is skipped and every keypoint of the row gets this code
        float R2[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t2[3] = {0, 0, 0}, Ow2[3];
        if (!live || !rec_ok(P.T.nRecords, nb)) rowStage = IVF_CREATE_NONE;
        else {
            load_pose(poses + (size_t)nb * 12, R2, t2);
            neg_rt_mul(R2, t2, Ow2);
            const float vBaseline[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
            const float baseline = (float)norm3(vBaseline);
            if (baseline < P.T.b) rowStage = IVF_CREATE_BASELINE;                                    // :317
        }
        if (rowStage >= 0) {                                   // uniform in the workgroup
            for (int i = tid; i < nf; i += kCreateThreads) {
                if (O.matches) O.matches[drow + i] = -1;
                if (O.stage) O.stage[drow + i] = (uint8_t)(i < n1 ? rowStage : IVF_CREATE_NONE);
            }
            continue;
        }
        const uint8_t* rec2 = records + (size_t)nb * P.T.recBytes;
        float F12[9];
        if (F12In) { for (int i = 0; i < 9; i++) F12[i] = F12In[((size_t)k * P.maxNeigh + r) * 9 + i]; }
        else compute_f12(P.T, R1, t1, R2, t2, F12);
        float C2[3];
        mul_add(R2, Ow1, t2, C2);                                                                   // ORBmatcher.cc:670-676
        const float invz = 1.0f / C2[2];
        const float ex = P.T.fx * C2[0] * invz + P.T.cx, ey = P.T.fy * C2[1] * invz + P.T.cy;
        for (int i = tid; i < nf; i += kCreateThreads) { s_match[i] = -1; s_stage[i] = IVF_CREATE_NONE; }
        if (tid == 0) { s_nCommon = 0; s_next = 0; s_pos[0] = 0x7fffffff; s_pos[1] = 0x7fffffff; }
        __syncthreads();
        // ---- which keyframe std::map<KeyFrame*, size_t> iterates first (MapPoint.cc:266): its position in kf_order
        if (kfOrder)
            for (int i = tid; i < P.T.nRecords; i += kCreateThreads) {
                const int o = kfOrder[i];
                if (o == kf) atomicMin(&s_pos[0], i);
                if (o == nb) atomicMin(&s_pos[1], i);
            }
        // ---- node merge (ORBmatcher.cc:697-795): a keyframe node takes part when the neighbour's ascending list holds the same id
        const size_t s2 = s1 + 1 + r;
        const int* node1 = B.fvNode + s1 * nf; const int* node2 = B.fvNode + s2 * nf;
        const int* start1 = B.fvStart + s1 * (nf + 1); const int* start2 = B.fvStart + s2 * (nf + 1);
        const int* idx1L = B.fvIdx + s1 * nf; const int* idx2L = B.fvIdx + s2 * nf;
        const int nn1 = B.fvN[s1], nn2 = B.fvN[s2];
        for (int a = tid; a < nn1; a += kCreateThreads) {
            const int b = sorted_find(node2, nn2, node1[a]);
            if (b >= 0) s_list[atomicAdd(&s_nCommon, 1)] = a | (b << 12);
        }
        __syncthreads();
        const int nCommon = s_nCommon;
        const bool kfFirst = kfOrder ? (s_pos[0] < s_pos[1] || (s_pos[0] == s_pos[1] && kf <= nb)) : kf <= nb;
        const ivf_keypoint* kp1 = rec_kps(rec1); const ivf_keypoint* kp2 = rec_kps(rec2);
        const uint8_t* d1 = rec_desc(rec1, nf); const uint8_t* d2 = rec_desc(rec2, nf);
        const float* ur1 = rec_uright(rec1, nf); const float* ur2 = rec_uright(rec2, nf);
        const float* z1 = rec_depth(rec1, nf); const float* z2 = rec_depth(rec2, nf);
        const uint8_t* has2 = hasPoint + (size_t)nb * nf;
        // ---- SearchForTriangulation: a wave takes the common nodes one at a time
        for (;;) {
            int c = 0;
            if (lane == 0) c = atomicAdd(&s_next, 1);
            c = __builtin_amdgcn_readfirstlane(c);
            if (c >= nCommon) break;
            const int e = s_list[c], a = e & 0xfff, b = e >> 12;
            const int ks = start1[a], ke = start1[a + 1], fs = start2[b], nFn = start2[b + 1] - fs;  // both runs hold at least one feature
            for (int j = ks; j < ke; j++) {
                const int i1 = idx1L[j];
                if (s_has[i1]) continue;                                                            // :708
                const uint4* pq = (const uint4*)(d1 + (size_t)i1 * 32);
                const uint4 qa = pq[0], qb = pq[1];
                const float x1 = kp1[i1].x, y1 = kp1[i1].y;
                const bool bStereo1 = ur1[i1] >= 0;
                const float la = x1 * F12[0] + y1 * F12[3] + F12[6], lb = x1 * F12[1] + y1 * F12[4] + F12[7], lc = x1 * F12[2] + y1 * F12[5] + F12[8];   // :149-151
                const float den = la * la + lb * lb;
                unsigned bestKey = 0xffffffffu;
                for (int q = 0; q < nFn; q += 64) {
                    const int pos = q + lane;
                    const int i2 = idx2L[fs + min(pos, nFn - 1)];
                    const uint4* pf = (const uint4*)(d2 + (size_t)i2 * 32);
                    const uint4 fa = pf[0], fb = pf[1];
                    const ivf_keypoint k2 = kp2[i2];
                    const bool bStereo2 = ur2[i2] >= 0;
                    const int dist = hamming256(qa, qb, fa, fb);
                    bool ok = pos < nFn && has2[i2] == 0 && dist <= 50;                             // :731, :744 (TH_LOW; dist > bestDist: the key)
                    const int o2 = clamp_octave(k2.octave);
                    if (!bStereo1 && !bStereo2) {                                                   // :749-755
                        const float distex = ex - k2.x, distey = ey - k2.y;
                        if (distex * distex + distey * distey < 100.0f * P.T.scale[o2]) ok = false;
                    }
                    const float num = la * k2.x + lb * k2.y + lc;                                   // CheckDistEpipolarLine (:146-163)
                    if (den == 0) ok = false;
                    else if (!((double)(num * num / den) < 3.84 * (double)P.sigma2[o2])) ok = false;
                    bestKey = min(bestKey, last_min_key(ok, dist, pos));
                }
                const unsigned best = wave_min_u32(bestKey);
                if (best != 0xffffffffu && lane == 0) s_match[i1] = idx2L[fs + last_min_position(best)];
            }
        }
        __syncthreads();
        // ---- vMatchedIndices (:821-826): idx1 ascending
        const int nMatch = compact_ordered<kCreateThreads>(n1, s_wcnt, tid, [&](int i) { return s_match[i] >= 0; }, [&](int i, int slot) { s_list[slot] = i; });
        // ---- one lane per match
        for (int m = tid; m < nMatch; m += kCreateThreads) {
            const int i1 = s_list[m], i2 = s_match[i1];
            const Side sd1{R1, t1, Ow1, kp1[i1], ur1[i1], z1[i1]}, sd2{R2, t2, Ow2, kp2[i2], ur2[i2], z2[i2]};
            float x3D[3], normal1[3], normal2[3], dist1, dist2;
            const int code = triangulate(P, sd1, sd2, x3D, normal1, normal2, dist1, dist2);
            s_stage[i1] = (uint8_t)code;
            if (code < IVF_CREATE_BY_SVD) continue;
            ivf_local_point mp;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                mp.pos[i] = x3D[i];
                mp.normal[i] = (normal1[i] / dist1 + normal2[i] / dist2) * 0.5f;                    // MapPoint.cc:353-374, n = 2
            }
            mp.max_distance = dist1 * P.T.scale[clamp_octave(sd1.kp.octave)];                       // mpRefKF = the current keyframe (:366-373)
            mp.min_distance = mp.max_distance / P.T.scale[P.T.nlevels - 1];
            const unsigned* pd = (const unsigned*)(kfFirst ? d1 + (size_t)i1 * 32 : d2 + (size_t)i2 * 32);   // MapPoint.cc:292-306 with N = 2: the first row
#pragma unroll
            for (int i = 0; i < 8; i++) ((unsigned*)mp.desc)[i] = pd[i];
            mp.flags = 2; mp.pad[0] = 0; mp.pad[1] = 0; mp.pad[2] = 0;
            O.point[row + i1] = mp;
            O.neigh[row + i1] = r; O.idx2[row + i1] = i2;
            float q = 1.0f;
            if (keyQuality) { const float qa = keyQuality[(size_t)kf * nf + i1], qb = keyQuality[(size_t)nb * nf + i2]; q = qb < qa ? qb : qa; }   // :513-516
            O.quality[row + i1] = q;
        }
        __syncthreads();
        // ---- creation order inside the rank = match order; AddMapPoint(pMP, idx1) (:505) for the ranks that follow
        nnew += compact_ordered<kCreateThreads>(nMatch, s_wcnt, tid, [&](int m) { return s_stage[s_list[m]] >= IVF_CREATE_BY_SVD; },
                                                [&](int m, int slot) { const int i1 = s_list[m]; O.order[row + i1] = nnew + slot; s_has[i1] = 1; });
        for (int i = tid; i < nf; i += kCreateThreads) {
            if (O.matches) O.matches[drow + i] = s_match[i];
            if (O.stage) O.stage[drow + i] = s_stage[i];
        }
        __syncthreads();
    }
    if (tid == 0) O.nNew[k] = live ? nnew : -1;
}

}  // namespace

extern "C" {

int ivf_tracker_create_map_points(ivf_tracker* t, const ivf_vocabulary* voc, int levelsup, const uint8_t* d_records, size_t record_bytes, int n_records,
                                  const int32_t* d_kf, int n_kf, const int32_t* d_neigh, int max_neigh, const float* d_poses,
                                  const uint8_t* d_has_point, const float* d_key_quality, const float* d_F12, const int32_t* d_kf_order,
                                  ivf_local_point* d_new_point, int32_t* d_new_neigh, int32_t* d_new_idx2, int32_t* d_new_order,
                                  float* d_new_quality, int32_t* d_n_new, int32_t* d_matches, uint8_t* d_stage, void* hip_stream)
{
    if (!t || !voc || !d_records || !d_kf || !d_neigh || !d_poses || !d_has_point || !d_new_point || !d_new_neigh || !d_new_idx2 || !d_new_order ||
        !d_new_quality || !d_n_new)
        return fail(IVF_E_INVALID, "null argument");
    if (((size_t)d_records & 15) != 0 || ((size_t)d_new_point & 15) != 0) return fail(IVF_E_INVALID, "the record block and the point array must be 16-byte aligned");
    if (levelsup < 0) return fail(IVF_E_INVALID, "levelsup %d is negative", levelsup);
    if (n_kf < 0 || max_neigh < 1) return fail(IVF_E_INVALID, "n_kf must be >= 0 and max_neigh >= 1");
    if ((long long)n_kf * max_neigh > t->cfg.max_pairs)
        return fail(IVF_E_CAPACITY, "%d keyframes x %d neighbours exceed the handle's %d pairs", n_kf, max_neigh, t->cfg.max_pairs);
    VocabularyView V;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin_with_vocabulary(t, voc, &V, true, record_bytes, n_records, n_kf, st);
    if (rc != IVF_OK) return rc;
    if (n_kf == 0) return IVF_OK;
    CreateParams P;
    P.T = t->P; P.T.nRecords = n_records;
    level_sigma2(P.T, P.sigma2);
    P.ratioFactor = 1.5f * (P.T.nlevels > 1 ? P.T.scale[1] : 1.0f);
    P.nidLevel = V.depth - levelsup; P.maxNeigh = max_neigh;
    const int nf = P.T.nf, slots = n_kf * (1 + max_neigh);                                          // <= 2 * max_pairs, the scratch's slots
    const TrackerBowScratch B = t->bow;
    size_t keyBytes;
    key_sort_pad(nf, &keyBytes);
    hipLaunchKernelGGL(k_create_nodes, dim3((nf + 15) / 16, slots), dim3(256), 0, st, P, V, d_records, d_kf, d_neigh, B.nodeKey);
    hipLaunchKernelGGL(k_create_featvec, dim3(slots), dim3(256), keyBytes, st, P, d_records, d_kf, d_neigh, B);
    const CreateOut O{d_new_point, d_new_neigh, d_new_idx2, d_new_order, d_new_quality, d_n_new, d_matches, d_stage};
    hipLaunchKernelGGL(k_create_points, dim3(n_kf), dim3(kCreateThreads), (size_t)nf * 10, st, P, d_records, d_kf, d_neigh, d_poses, d_has_point,
                       d_key_quality, d_F12, d_kf_order, B, O);
    return tracker_end(t, st);
}

}  // extern "C"
