// ivf_device.h -- shared host/device structures of the gfx950 front end (not part of the public C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>      // getenv behind IVF_EXP_ENV (experiment builds)
#include <vector>
#include "../../include/ivfront.h"

#define DEVINL __device__ __forceinline__

namespace ivf {

constexpr int kMaxLevels = IVF_MAX_LEVELS;
constexpr int kMaxCells = 2048;          // per level (LDS bookkeeping arrays in k_quota, 50 KB); the reference has ~N_level / 5 cells, i.e. ~10 000 features on one level
constexpr int kEdge = 19;                // EDGE_THRESHOLD (ORB/src/ORBextractor.cc:75)

// Geometry of one pyramid level.  All of it depends only on (params, image size), so the host
// computes it once (ORB/src/ORBextractor.cc:884-922) and the kernels read it as uniform data.
struct LevelGeom {
    int w, h, pitch;        // level size; row pitch in bytes (multiple of 64)
    int off;                // byte offset of the level inside one image's pyramid blob
    int nDesired;           // mnFeaturesPerLevel[level]
    int cols, rows, cellW, cellH, nCells, nfeaturesCell;
    int maxBX, maxBY;       // w-19, h-19
    int domH[2];            // FAST rows scanned per cell in non-last cell rows: [0] plain, [1] stale-hY (Appendix D-2)
    int domHLast;           // ... in the last cell row
    int winHLast;           // hY of the last cell row (cost-map pre-pass window)
    int cellBase;           // first cell of this level in per-image cell arrays
    int candBase, candCap;  // candidate scratch: element offset of the level, capacity per cell
    int kpBase;             // first keypoint slot of this level (prefix sum of nDesired)
    int scaledPatch;        // (int)(31*scale)
    int tileBase, tilesX, tilesY;   // FAST tile enumeration (scan region x>=16, y>=19)
    int btileBase, btilesX, btilesY; // blur tile enumeration (whole plane)
    int rtX, rtY;           // offsets into the packed cv::resize coefficient table (level >= 1)
    int valid;              // 0: level yields no keypoints
    float scale;            // mvScaleFactor[level]
    unsigned cellWMagic, cellHMagic;   // floor(2^32 / cellW) + 1: n / cellW = umulhi(n, magic), exact for n < 2^16 (cells are at most 4096 px)
};

struct Config {
    int nlevels, w, h;
    int nfeatures, iniTh, minTh, introspection;
    int pyrBytes;           // bytes of one image's pyramid blob
    int candTotal;          // candidate scratch elements per image
    int nCellsTotal;        // cells per image over all levels
    int nTiles;             // FAST tiles per image
    int nBlurTiles;         // blur tiles per image
    int varBlur, varRetain, varAtan;   // OpenCV-version switches (ivf_extractor_set_opencv_variant): 0 = OpenCV >= 3.4.2 / 4.x
    int maxCandCap;         // largest per-cell bound on strict 3x3 maxima over the levels (k_cell_select_huge slot size)
    int umax[16];
    float scale[kMaxLevels], invScale[kMaxLevels];
    int cellBases[kMaxLevels];                           // lv[l].cellBase of the VALID levels side by side (INT_MAX for an invalid level and past nlevels): one wide scalar load
    int tileBases[kMaxLevels], btileBases[kMaxLevels];   // lv[l].tileBase / btileBase side by side (INT_MAX past nlevels):
                                                         // a tile finds its level with one wide uniform load
    LevelGeom lv[kMaxLevels];
};

// cv::resize coefficient table entry: src index | coef0 << 16 | coef1 << 32 (11-bit fixed point, A-3); k_resize's entries also carry
// the second source index in bits 48-63 (the pyramid's are zero there)
typedef unsigned long long ResizeCoef;

// The one restatement of cv::resize's INTER_LINEAR axis rule (ivf_rectify.hip).  For every destination index d:
// s = cvFloor(f), f = (float)((d + 0.5) * scale - 0.5) with scale = 1. / ((double)dsize / ssize); idx0 = clip(s), idx1 = clip(s + 1),
// w0 = saturate_cast<short>((1 - (f - s)) * 2048), w1 = saturate_cast<short>((f - s) * 2048): the rows the vertical pass reads and their
// coefficients, which are not clipped.  Columns additionally set f - s to 0 where s < 0 or s >= ssize - 1, i.e. exactly where
// idx0 == idx1: there w0 = 2048, w1 = 0.
void resize_axis_table(int ssize, int dsize, int32_t* idx0, int32_t* idx1, int16_t* w0, int16_t* w1);
// appends the dsize entries of one axis to `tab`: idx0 | w0 << 16 | w1 << 32 (| idx1 << 48 when withIdx1); columns get the edge rule
void resize_axis_pack(int ssize, int dsize, bool columns, bool withIdx1, std::vector<ResizeCoef>& tab);

// The one text of cv::undistortPoints(src, dst, K, D, cv::Mat(), K) for one point, shared by the host entry points and
// k_undistort_keys (Frame::UndistortKeyPoints / ComputeImageBounds, ORB/src/Frame.cc:714, :740).  K and D are CV_32F in
// the reference (ORB/src/Tracking.cc:106-123): widened here once, every intermediate is double, the result is narrowed once.
// Five iterations whether converged or not (TermCriteria(MAX_ITER, 5, 0.01): the count only); RR = K * I is spelled out term by term.
// The library is built with -ffp-contract=off: host and device round every operation alike.
struct UndistortCam { double fx, fy, cx, cy, k[12]; };          // k = k1,k2,p1,p2,k3,k4,k5,k6,s1,s2,s3,s4 (missing ones 0)
inline UndistortCam undistort_cam(const ivf_camera& c)
{
    UndistortCam u{};
    u.fx = (double)c.fx; u.fy = (double)c.fy; u.cx = (double)c.cx; u.cy = (double)c.cy;
    for (int i = 0; i < 12; i++) u.k[i] = i < c.n_dist ? (double)c.dist[i] : 0.;
    return u;
}
__host__ __device__ inline void undistort_point(const UndistortCam& c, float px, float py, float& ox, float& oy)
{
    const double* k = c.k;
    const double ifx = 1. / c.fx, ify = 1. / c.fy;
    const double u = (double)px, v = (double)py;
    double x = (u - c.cx) * ifx, y = (v - c.cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) { x = (u - c.cx) * ifx; y = (v - c.cy) * ify; break; }
        const double dX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double dY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - dX) * icdist; y = (y0 - dY) * icdist;
    }
    const double xx = c.fx * x + 0. * y + c.cx, yy = 0. * x + c.fy * y + c.cy, ww = 1. / (0. * x + 0. * y + 1.);
    ox = (float)(xx * ww); oy = (float)(yy * ww);
}

#ifndef IVF_FAST_TH
#define IVF_FAST_TH 32        // 64 measured slower: 405 vs 348 us per 128 images (occupancy: 32 KB of LDS per workgroup, ragged level edges)
#endif
constexpr int kFastTW = 128, kFastTH = IVF_FAST_TH;    // FAST/NMS output tile (kFastTW + 2 <= 160, kFastTH + 2 <= 96: see k_fast_nms)
constexpr int kBlurTW = 128, kBlurTH = 32;    // blur output tile
constexpr int kTileCap = kFastTW * kFastTH / 4;   // at most one strict 3x3 maximum per 2x2 block
constexpr int kRowCap = 96;              // right keypoints listed per image row by k_stereo_rows (more: that row falls back to the full scan)
constexpr int kHugeSlots = 8;            // workgroups (= global scratch slots) of k_cell_select_huge
constexpr int kHugeListCap = 4096;       // cells with > 4096 survivors listed per launch

// per cell, from k_quota (k_cell_qsum parks the cell's cost-window sum in nTotal until then)
struct CellInfo { int nTotal, nRetain, prefix, useMin; };

struct Buffers {            // device pointers of one batch context
    uint8_t* pyr;           // [nImg][pyrBytes]  un-blurred pyramid (level 0 = ingested input)
    uint8_t* qpyr;          // [nImg][pyrBytes]  cost-map pyramid (introspection) or nullptr
    uint8_t* blur;          // [nImg][pyrBytes]  7x7 sigma-2 blurred pyramid
    unsigned* tileList;     // [nImg][nTiles][kTileCap] unordered NMS survivors of each FAST tile: y<<20 | x<<8 | score
    int* tileCnt;           // [nImg][nTiles] survivors per tile
    int* cellCnt;           // [nImg][nCellsTotal][2] survivors per cell: {score >= minTh, score >= iniTh}
    unsigned long long* lvl;    // [nImg][candTotal] per level: kept keys (respbits<<32 | y<<16 | x) of all cells, (i,j) order
    CellInfo* cellInfo;     // [nImg][nCellsTotal]
    int* lvlTotal;          // [nImg][kMaxLevels] length of each level list before the level-wide retainBest
    unsigned int* slotPos;  // [nImg][nfeatures] (y<<16|x) level coords
    float* slotResp;        // [nImg][nfeatures]
    int* lvlCount;          // [nImg][kMaxLevels]
    uint8_t* useCost;       // [nImg] bit 0 = cost pyramid gates this image's extraction, bit 1 = level 0 of the cost image feeds mvKeyQualScore
    ivf_keypoint* kps;      // [nImg][nfeatures]
    uint8_t* desc;          // [nImg][nfeatures][32]
    int* count;             // [nImg]
    float* quality;         // [nImg][nfeatures]  mvKeyQualScore (Frame.cc:130-143)
    float* uright;          // [nPairs][nfeatures]
    float* depth;           // [nPairs][nfeatures]
    int* sad;               // [nPairs][nfeatures]  best SAD distance or -1
    int* rowCnt;            // [nPairs][H]  right keypoints whose row band covers the row (k_stereo_rows)
    unsigned short* rowList;    // [nPairs][H][kRowCap]
    int* status;            // [1] device-side error flags, cleared by the host when read
    int* hugeCount;         // [3] cells with more than 4096 survivors in this launch (k_quota -> k_cell_select_huge); [1], [2]: lengths of the tier lists
    int* tierList;          // [2][nImg * nCellsTotal] cells with 257..1024 / 1025..4096 survivors: img * nCellsTotal + cell (k_quota -> k_cell_select_list)
    int* hugeList;          // [kHugeListCap] img * nCellsTotal + cell
    unsigned* hugeScratch;  // [kHugeSlots][4 * maxCandCap] dwords, or nullptr when no cell can exceed 4096 maxima
};

// arguments of the stereo matcher kernels: left/right data may live in one batch context
// (frontend: images interleaved L,R) or in two single-image contexts (two ivf_extractor handles)
struct StereoArgs {
    const uint8_t *pyrL, *pyrR; size_t pyrStride;          // bytes between consecutive pairs
    const ivf_keypoint *kpL, *kpR; const uint8_t *descL, *descR; const int *cntL, *cntR;
    size_t kpStride;        // elements (ivf_keypoint / 32-byte rows) between pairs
    int cntStride;
    float *uright, *depth; int* sad; int outStride;
    float bf, bb;
    int* rowCnt; unsigned short* rowList;                  // [nPairs][H], [nPairs][H][kRowCap]: right keypoints per image row, or null
};

// Environment switches.  The shipped library reads exactly the switches listed in INTEGRATION.md (documented, result-preserving:
// getenv is spelled out at those sites).  Every kernel-variant selector and tuning knob of the experiments behind DESIGN.md goes through
// IVF_EXP_ENV, which is getenv only in an experiment build (`make EXPERIMENT=1` -> libivfront_exp.so, loaded through IVFRONT_LIB by
// tools/ and by the kernel-variant tests) and a null constant in the product: the names are not even compiled in
// (tests/test_abi_cpu.py asserts the list of IVF_* strings in libivfront.so).
#ifdef IVF_EXPERIMENT
#define IVF_EXP_ENV(name) getenv(name)
#else
#define IVF_EXP_ENV(name) ((const char*)nullptr)
#endif

// every kernel launch of the library goes through hipLaunchKernelGGL: counted for bench.py's launches_per_step
void count_launch();
}  // namespace ivf
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...) do { ivf::count_launch(); hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__); } while (0)
namespace ivf {

// thread-local error message behind ivf_last_error() (ivf_api.hip)
int set_error(int code, const char* fmt, ...);

// host-side services of ivf_api.hip for the other translation units of the C-ABI: the calling thread's growable device / pinned
// scratch (pooled: see ScratchSlot) and the device-id check
int thread_scratch(int device, size_t need, uint8_t** out);
int thread_pinned(size_t need, uint8_t** out);
int have_device(int dev);

// One image of a front-end batch, as batch_image (ivf_api.hip) resolves it, and the frame made of it (ivf_match.hip, which alone knows struct ivf_frame):
// `count` keypoints of at most `cap` are valid once `done` has passed; kps = mvKeysUn (mvKeys unless the run had a camera); uright == depth == nullptr: no stereo
struct BatchImage { const ivf_keypoint *kps, *mvKeys; const uint8_t* desc; const float *uright, *depth, *quality; const int* count; int cap; hipEvent_t done; };
int frame_from_batch(int device, const BatchImage& src, const ivf_bounds& bounds, ivf_frame** out);

// launchers (ivf_kernels.hip)
void launch_stereo_args(const Config& hc, const Config* dc, const StereoArgs& A, int nPairs, hipStream_t s);
void launch_ingest(const Config& hc, const Config* dc, const uint8_t* src0, const uint8_t* src1, size_t imageStride, int rowStride,
                   int nImg, int nSides, uint8_t* dstBlob, const uint8_t* onlyFlagged, hipStream_t s, int sideMask = 3);
void launch_ingest_color(const Config& hc, const Config* dc, const uint8_t* src, size_t imageStride, int rowStride, int code, int nImg, int nSides, int side,
                         uint8_t* dstBlob, hipStream_t s);
void launch_pyramid(const Config& hc, const Config* dc, const ResizeCoef* dTab, uint8_t* blob, uint8_t* qblob, const uint8_t* useCost,
                    int nImg, hipStream_t s);
void launch_fast(const Config& hc, const Config* dc, const Buffers& b, int nImg, hipStream_t s);
void launch_blur(const Config& hc, const Config* dc, const Buffers& b, int nImg, hipStream_t s, bool skipEmptyLevels);
void launch_describe(const Config& hc, const Config* dc, const Buffers& b, int nImg, hipStream_t s);
void launch_stereo(const Config& hc, const Config* dc, const Buffers& b, int nPairs, float bf, float bb, hipStream_t s);
// kpsUn != nullptr: the records carry these keypoints (mvKeysUn of the left frames, addressed like b.kps: pair p at 2 * p * nf) instead of b.kps
void launch_pack_gather(const Buffers& b, const ivf_keypoint* kpsUn, int nf, int nPairs, uint8_t* block, size_t recBytes, hipStream_t s);
// launchers (ivf_select.hip); dLists, dDiffer: see k_test_retain_best
void launch_select(const Config& hc, const Config* dc, const Buffers& b, int nImg, hipStream_t s);
void launch_test_retain_best(const float* dResp, int n, int nPoints, int* dOrder, unsigned long long* dLists, int* dDiffer, hipStream_t s);
// k_undistort_keys (ivf_rectify.hip): frame f reads kps + f * kpStride and count[f * cntStride], writes out + f * outStride (elements)
void launch_undistort_keys(const UndistortCam& cam, bool passThrough, const ivf_keypoint* kps, size_t kpStride, const int* count, int cntStride,
                           int nFrames, int cap, ivf_keypoint* out, size_t outStride, hipStream_t s);
// gather record (ivf_frontend_pack_gather_block): {int32 n; int32 pad[3]; ivf_keypoint kps[nf]; uint8 desc[nf][32]; float uright[nf]; float depth[nf]}
__device__ __forceinline__ int rec_count(const uint8_t* r, int nf) { const int n = *(const int*)r; return n < 0 ? 0 : (n > nf ? nf : n); }
__device__ __forceinline__ const ivf_keypoint* rec_kps(const uint8_t* r) { return (const ivf_keypoint*)(r + 16); }
__device__ __forceinline__ const uint8_t* rec_desc(const uint8_t* r, int nf) { return r + 16 + (size_t)nf * 24; }
__device__ __forceinline__ const float* rec_uright(const uint8_t* r, int nf) { return (const float*)(r + 16 + (size_t)nf * 56); }
__device__ __forceinline__ const float* rec_depth(const uint8_t* r, int nf) { return (const float*)(r + 16 + (size_t)nf * 60); }
// The per-image flag byte through the scalar cache: gfx950 has no scalar byte load, so a plain `useCost [img]` is a vector load with an `s_waitcnt vmcnt(0)` in
// front of every scalar load that follows it at the head of a workgroup.  The flag array is allocated in whole dwords (Context::build).
__device__ __forceinline__ unsigned use_cost_of(const uint8_t* __restrict__ useCost, int img)
{
    const unsigned w = ((const unsigned*)useCost)[img >> 2];
    return (w >> (8 * (img & 3))) & 0xffu;
}

// sum over the wave without the LDS crossbar (r04; was six ds_bpermute round trips): row_shr 1/2/4/8 fold each row of 16 lanes into
// its lane 15, row_bcast15 / row_bcast31 fold the four rows into lane 63, which every lane then reads
__device__ __forceinline__ int wave_sum_i32(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}
// LDS operations of one wave execute in order: a wavefront-scope fence (compiler ordering) is all that one lane needs to
// read what another lane of the same wave wrote
__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// lane k's value to every lane (k uniform): v_readlane moves 32 bits, anything else goes through it dword by dword
template <class T> __device__ __forceinline__ T readlane_b32(T v, int k)
{
    static_assert(sizeof(T) == 4, "one dword");
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}
__device__ __forceinline__ float readlane_f32(float v, int k) { return readlane_b32(v, k); }
__device__ __forceinline__ double readlane_f64(double v, int k)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = readlane_b32((unsigned)b, k), hi = readlane_b32((unsigned)(b >> 32), k);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ uint4 readlane_u4(const uint4 v, int k)
{
    return make_uint4(readlane_b32(v.x, k), readlane_b32(v.y, k), readlane_b32(v.z, k), readlane_b32(v.w, k));
}
// The rotation-consistency filter of the batched searches, the one device text of it (k_track_greedy, k_bow_search): a match falls into
// one of 30 bins by the angle between its two keypoints (ORBmatcher.cc:244-251, :1476-1484), ComputeThreeMaxima (:1654-1695) keeps up to
// three bins, every match of another bin is taken back.
struct RotKeep {
    int ind1, ind2, ind3;
    __device__ __forceinline__ bool keeps(int bin) const { return bin == ind1 || bin == ind2 || bin == ind3; }
};
__device__ __forceinline__ int rot_bin(float rot)
{
    const float factor = 1.0f / 30.0f;                         // 1.0f / HISTO_LENGTH
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == 30) bin = 0;
    return bin;
}
__device__ __forceinline__ RotKeep rot_three_maxima(const int* hist)       // hist [30]: rotHist[b].size()
{
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int b = 0; b < 30; b++) {
        const int s = hist[b];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = b; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = b; }
        else if (s > max3) { max3 = s; ind3 = b; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    return RotKeep{ind1, ind2, ind3};
}
// cv::gemm on CV_32F operands: double accumulation of (double)a * (double)b, + (double)c, one narrowing
__device__ __forceinline__ void mul_add(const float* R, const float* p, const float* t, float* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
        out[i] = (float)((double)R[3 * i] * (double)p[0] + (double)R[3 * i + 1] * (double)p[1] + (double)R[3 * i + 2] * (double)p[2] + (double)t[i]);
}
// -R.t() * t (Frame::UpdatePoseMatrices, Frame.cc:549-555; ORBmatcher.cc:1385)
__device__ __forceinline__ void neg_rt_mul(const float* R, const float* t, float* out)
{
#pragma unroll
    for (int j = 0; j < 3; j++)
        out[j] = (float)(-((double)R[j] * (double)t[0] + (double)R[3 + j] * (double)t[1] + (double)R[6 + j] * (double)t[2]));
}

}  // namespace ivf

// error returns of the host code
#define fail ivf::set_error
#define HIPCHK(expr)                                                                                   \
    do { hipError_t e_ = (expr);                                                                        \
         if (e_ != hipSuccess) return fail(IVF_E_NO_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
