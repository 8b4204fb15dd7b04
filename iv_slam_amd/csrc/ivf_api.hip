// ivf_api.hip -- C-ABI of libivfront.so (include/ivfront.h), extraction side: the per-call extractor, stereo match and undistortion,
// the batched front end, the error state and the per-thread scratch pools.  The matcher searches, ivf_frame and the BoW calls are in
// ivf_match.hip.  Host side only; all image / descriptor compute is in ivf_kernels.hip and ivf_select.hip.  No CPU fallback exists.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <atomic>
#include <map>
#include <mutex>
#include <vector>
#include <algorithm>
#include "ivf_device.h"

using namespace ivf;

#ifdef IVF_EXPERIMENT
// ---- soak aid (tools/soak_frontend.py): host-visible progress words ----
// A 1-thread marker launch behind every stage of Context::run / ivf_frontend_run writes (run << 8 | stage) into a word of
// host-mapped memory the caller registered with ivf_debug_progress_words: when a child process of the soak sticks in
// ivf_frontend_sync, its parent reads from these words which stage each internal stream reached.  Words:
//   [k]      own batch on internal stream k:  1 ingest  2 pyramid  3 FAST  4 selection  5 join (blur awaited)  6 descriptors  7 stereo
//   [3 + k]  a LENT blur on internal stream k (batch of context k - 1): 1 fork passed  2 blur done
//   [6]      host: run << 8 | 1 enqueue entered, 2 enqueue done; [7] host: 0x10 + k = ivf_frontend_sync waits for stream k, 0x20 = returned
// Experiment builds only: the product has neither the words nor the launches.
namespace ivf {
__global__ void k_mark(int* w, int v) { __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
}
static int* g_markDev = nullptr;
static volatile int* g_markHost = nullptr;
#define IVF_MARK(st, word, stage, run) \
    do { if (g_markDev && (word) >= 0) hipLaunchKernelGGL(ivf::k_mark, dim3(1), dim3(1), 0, (st), g_markDev + (word), (int)(((run) << 8) | (stage))); } while (0)
#define IVF_MARK_HOST(word, v) do { if (g_markHost) g_markHost[(word)] = (int)(v); } while (0)
#else
#define IVF_MARK(st, word, stage, run) do { } while (0)
#define IVF_MARK_HOST(word, v) do { } while (0)
#endif

namespace {

thread_local std::string g_err;

inline int cvRoundF(float v) { return (int)lrintf(v); }
inline int cvFloorF(float v) { int i = (int)v; return i - (i > v); }
inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// ---- ORBextractor constructor tables (ORB/src/ORBextractor.cc:411-476) ----
struct Tables {
    ivf_extractor_params p;
    float scale[kMaxLevels], invScale[kMaxLevels], sigma2[kMaxLevels], invSigma2[kMaxLevels];
    int nfeat[kMaxLevels];
    int umax[16];
};
int make_tables(const ivf_extractor_params& p, Tables& t)
{
    if (p.nlevels < 1 || p.nlevels > kMaxLevels) return fail(IVF_E_INVALID, "nlevels %d outside [1,%d]", p.nlevels, kMaxLevels);
    if (p.nfeatures < 1 || p.nfeatures > 65534) return fail(IVF_E_INVALID, "nfeatures %d outside [1,65534]", p.nfeatures);
    if (!(p.scale_factor > 1.0f)) return fail(IVF_E_INVALID, "scale_factor must be > 1");
    if (p.min_th_fast < 1 || p.ini_th_fast < p.min_th_fast || p.ini_th_fast > 254)
        return fail(IVF_E_INVALID, "need 1 <= minThFAST <= iniThFAST <= 254");
    t.p = p;
    const double sf = (double)p.scale_factor;            // member is `double scaleFactor` (ORBextractor.h:110)
    t.scale[0] = 1.0f; t.sigma2[0] = 1.0f;
    for (int i = 1; i < p.nlevels; i++) {
        t.scale[i] = (float)((double)t.scale[i - 1] * sf);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < p.nlevels; i++) { t.invScale[i] = 1.0f / t.scale[i]; t.invSigma2[i] = 1.0f / t.sigma2[i]; }
    const float factor = (float)(1.0 / sf);
    float nDes = (float)p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)p.nlevels));
    int sum = 0;
    for (int l = 0; l < p.nlevels - 1; l++) { t.nfeat[l] = cvRoundF(nDes); sum += t.nfeat[l]; nDes *= factor; }
    t.nfeat[p.nlevels - 1] = std::max(p.nfeatures - sum, 0);
    const int HP = 15;
    int v, v0;
    const int vmax = (int)std::floor(HP * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(HP * std::sqrt(2.f) / 2);
    const double hp2 = HP * HP;
    for (v = 0; v <= vmax; ++v) t.umax[v] = (int)lrint(std::sqrt(hp2 - v * v));
    for (v = HP, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    return IVF_OK;
}

// One set of input planes, as the caller holds it: image i of the set at p + i * imageStride, rows rowStride bytes apart.
// code 0 = grey, 1 / 2 (| 4) = B,G,R / R,G,B interleaved (IVF_COLOR_*: k_ingest_color converts)
struct ImageSrc { const uint8_t* p; size_t imageStride; int rowStride; int code; };

// ---- one batch context: geometry + device buffers for a fixed (params, image size, capacity) ----
struct Context {
    int device = 0, maxImg = 0, nSides = 1;
    bool introspection = false;
    bool needsCost = false;             // cell rows overshoot a level: only the introspection path (stale hY) is defined there
    Config hc{};
    Config* dc = nullptr;
    ResizeCoef* dTab = nullptr;           // packed cv::resize coefficients, all levels
    Buffers b{};
    std::vector<void*> owned;           // every device allocation of the context (alloc): release() frees these
    uint8_t* dStage = nullptr;          // single-image host API staging (image + cost)
    uint8_t* hStage = nullptr;          // ... and its pinned host twin (+ room for the keypoints / descriptors coming back)
    size_t stageBytes = 0;
    static constexpr int kEvRing = 64;  // HIP event pairs around the FAST+NMS launch of the last kEvRing runs
    hipEvent_t evFast0[kEvRing] = {}, evFast1[kEvRing] = {};
    // r04: the blur (throughput-bound, needs only the pyramid) runs on a side stream beside the selection chain (quota, three tier
    // launches, level selection: latency-bound, ~285 us per 256 images) and joins in front of the descriptors.  The side stream is
    // LENT by the caller (the batched front end passes the internal stream of its next context): a stream of its own per context
    // cost configs[2] 15 % -- 10.4k -> 9.0k pairs/s just by existing, whether used or not: the runtime multiplexes streams onto a few
    // hardware queues, and three more streams put the FCN's stream behind front-end work
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    long long nRuns = 0;
    int markOwn = -1, markSide = -1;    // progress words of this context's stream / of the stream its blur is lent (experiment builds: IVF_MARK)

    int build(const Tables& t, int w, int h, int maxImages, int sides, int dev, bool withStereo, const int* variant = nullptr);
    int set_variant(const int* variant);
    void release();
    // one hipMalloc the context owns from here on; zero: cleared (blocking) as well
    template <class T> hipError_t alloc(T*& p, size_t bytes, bool zero = false)
    {
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        owned.push_back(p);
        return zero ? hipMemset(p, 0, bytes) : hipSuccess;
    }
    int ensure_qpyr(hipStream_t st);
    // side[sd]: the images of side sd (one side: side[0]); cost: the cost maps, or null.  perSide: one ingest launch per side even where
    // one launch could serve both (grey sides that share their strides) -- ivf_frontend_run_color, which has always ingested side by side
    int run(const ImageSrc (&side)[2], const ImageSrc* cost, int nImg, const uint8_t* dUseCostSrc, hipStream_t st,
            hipEvent_t inputsConsumed = nullptr, hipStream_t sideStream = nullptr, bool perSide = false);
    int check_status(int which = 0);
};

int Context::set_variant(const int* v)
{
    hc.varBlur = v[0] ? 1 : 0; hc.varRetain = v[1] ? 1 : 0; hc.varAtan = v[2] ? 1 : 0;
    if (dc) { HIPCHK(hipSetDevice(device)); HIPCHK(hipDeviceSynchronize()); HIPCHK(hipMemcpy(dc, &hc, sizeof(Config), hipMemcpyHostToDevice)); }
    return IVF_OK;
}

int Context::build(const Tables& t, int w, int h, int maxImages, int sides, int dev, bool withStereo, const int* variant)
{
    device = dev; maxImg = maxImages; nSides = sides;
    introspection = t.p.enable_introspection != 0;
    if (w < 1 || h < 1 || w > 4095 || h > 4095) return fail(IVF_E_INVALID, "image size %dx%d unsupported (max 4095)", w, h);
    Config& c = hc;
    memset(&c, 0, sizeof c);
    c.nlevels = t.p.nlevels; c.w = w; c.h = h; c.nfeatures = t.p.nfeatures;
    c.iniTh = t.p.ini_th_fast; c.minTh = t.p.min_th_fast; c.introspection = introspection ? 1 : 0;
    if (variant) { c.varBlur = variant[0] ? 1 : 0; c.varRetain = variant[1] ? 1 : 0; c.varAtan = variant[2] ? 1 : 0; }
    memcpy(c.umax, t.umax, sizeof c.umax);
    {   // k_describe carries umax as a packed constant (HALF_PATCH_SIZE = 15 is fixed): make sure it is this table
        const unsigned long long packed = 0x3689ABCDDEEEFFFFull;
        for (int i = 0; i < 16; i++)
            if ((int)((packed >> (4 * i)) & 15) != t.umax[i]) return fail(IVF_E_STATE, "umax table mismatch at %d", i);
    }
    const float imageRatio = (float)w / h;                       // ORBextractor.cc:884
    int off = 0, cellBase = 0, candBase = 0, kpBase = 0, tileBase = 0, btileBase = 0;
    for (int l = 0; l < c.nlevels; l++) {
        LevelGeom& G = c.lv[l];
        c.scale[l] = t.scale[l]; c.invScale[l] = t.invScale[l];
        G.scale = t.scale[l];
        G.w = cvRoundF((float)w * t.invScale[l]);                 // :1303
        G.h = cvRoundF((float)h * t.invScale[l]);
        if (G.w < 1 || G.h < 1) return fail(IVF_E_GEOMETRY, "pyramid level %d is empty for %dx%d", l, w, h);
        G.pitch = align_up(G.w, 64);
        G.off = off; off += G.pitch * G.h;
        G.nDesired = t.nfeat[l];
        G.kpBase = kpBase; kpBase += G.nDesired;
        G.scaledPatch = (int)(31 * t.scale[l]);                   // :1142
        G.cols = (int)std::sqrt((float)G.nDesired / (5 * imageRatio));   // :890
        G.rows = (int)(imageRatio * G.cols);                      // :891
        G.maxBX = G.w - kEdge; G.maxBY = G.h - kEdge;
        const int W = G.maxBX - kEdge, H = G.maxBY - kEdge;
        G.valid = (G.cols > 0 && G.rows > 0 && W > 0 && H > 0 && G.nDesired > 0) ? 1 : 0;
        G.btileBase = btileBase; G.btilesX = (G.w + kBlurTW - 1) / kBlurTW; G.btilesY = (G.h + kBlurTH - 1) / kBlurTH;
        btileBase += G.btilesX * G.btilesY;
        G.cellBase = cellBase; G.candBase = candBase; G.tileBase = tileBase;
        if (!G.valid) continue;
        G.cellW = (int)std::ceil((float)W / G.cols);              // :906-907
        G.cellH = (int)std::ceil((float)H / G.rows);
        G.nCells = G.rows * G.cols;
        G.cellWMagic = (unsigned)(0x100000000ull / (unsigned)G.cellW) + 1u;   // cellW, cellH >= 1 here; == 1 gives 0: see k_fast_nms
        G.cellHMagic = (unsigned)(0x100000000ull / (unsigned)G.cellH) + 1u;
        if (G.nCells > kMaxCells) return fail(IVF_E_INVALID, "level %d has %d cells (max %d)", l, G.nCells, kMaxCells);
        G.nfeaturesCell = (int)std::ceil((float)G.nDesired / G.nCells);   // :923
        // cell windows must stay inside [16, dim-16): otherwise the reference throws in rowRange/colRange
        // or reads outside the blurred clone (ORBextractor.cc:1033, 1276)
        // With introspection the stale-hY quirk gives every row the LAST row's window height, which is
        // negative or tiny exactly when the rows overshoot: the reference then runs (and finds nothing in those cells) as long
        // as a cost map comes with the image.  A per-call extractor with introspection on is therefore accepted and checked
        // per call; stereo contexts hold a non-introspective right side and are rejected here.
        const bool colsLeave = (G.cols - 1) * G.cellW > W, rowsLeave = (G.rows - 1) * G.cellH > H;
        const bool lastRowEmpty = H - (G.rows - 1) * G.cellH + 6 < 0;     // hY < 0 in the last row: stale negative height, rowRange throws
                                                                          // (hY == 0: empty windows, the level yields nothing -- k_quota)
        if (colsLeave || (rowsLeave && (!(introspection && sides == 1) || lastRowEmpty)))
            return fail(IVF_E_GEOMETRY, "level %d: %dx%d cells of %dx%d leave the %dx%d level", l, G.cols, G.rows,
                        G.cellW, G.cellH, G.w, G.h);
        if (rowsLeave) needsCost = true;
        G.domHLast = H - (G.rows - 1) * G.cellH;
        G.winHLast = G.domHLast + 6;
        G.domH[0] = G.cellH;
        G.domH[1] = G.domHLast;                                   // stale hY
        G.candCap = ((G.cellW + 1) / 2) * ((G.cellH + 1) / 2) + 1;
        c.maxCandCap = std::max(c.maxCandCap, G.candCap);
        cellBase += G.nCells; candBase += G.nCells * G.candCap;
        G.tilesX = (G.maxBX - 16 + kFastTW - 1) / kFastTW;
        G.tilesY = (G.maxBY - kEdge + kFastTH - 1) / kFastTH;
        tileBase += G.tilesX * G.tilesY;
    }
    c.pyrBytes = align_up(off + 64, 256);
    c.candTotal = std::max(candBase, 1);
    c.nCellsTotal = std::max(cellBase, 1);
    c.nTiles = tileBase;
    c.nBlurTiles = btileBase;
    for (int l = 0; l < kMaxLevels; l++) {
        c.cellBases[l] = (l < c.nlevels && c.lv[l].valid) ? c.lv[l].cellBase : INT_MAX;
        c.tileBases[l] = l < c.nlevels ? c.lv[l].tileBase : INT_MAX;
        c.btileBases[l] = l < c.nlevels ? c.lv[l].btileBase : INT_MAX;
    }

    // cv::resize coefficient table (OpenCV resize.cpp, INTER_LINEAR 8U), from the axis rule shared with
    // ivf_resize (resize_axis_table): per output column {clamped sx, a0, a1}, per output row {clipped sy, b0, b1}.
    // pyr_tile reads rows y0 and min(y0 + 1, h - 1): the second row of the table for every level pair, which only down-scales
    // (tests/test_resize_cpu.py checks that on the pyramids of the benchmark sizes).
    std::vector<ResizeCoef> tab;
    for (int l = 1; l < c.nlevels; l++) {
        LevelGeom& D = c.lv[l]; const LevelGeom& S = c.lv[l - 1];
        D.rtX = (int)tab.size();
        resize_axis_pack(S.w, D.w, true, false, tab);
        D.rtY = (int)tab.size();
        resize_axis_pack(S.h, D.h, false, false, tab);
    }
    if (tab.empty()) tab.push_back(0);

    HIPCHK(hipSetDevice(device));
    HIPCHK(alloc(dc, sizeof(Config)));
    HIPCHK(hipMemcpy(dc, &hc, sizeof(Config), hipMemcpyHostToDevice));
    HIPCHK(alloc(dTab, tab.size() * sizeof(ResizeCoef)));
    HIPCHK(hipMemcpy(dTab, tab.data(), tab.size() * sizeof(ResizeCoef), hipMemcpyHostToDevice));
    const size_t nI = (size_t)maxImg, nf = (size_t)c.nfeatures, blob = (size_t)c.pyrBytes * nI;
    HIPCHK(alloc(b.pyr, blob + 256));               // + slack: k_stereo_match / k_describe read whole dwords that may end a few bytes past a plane's last row
    HIPCHK(alloc(b.blur, blob + 256));
    HIPCHK(hipMemset(b.pyr, 0, blob));
    if (introspection) HIPCHK(alloc(b.qpyr, blob, true));
    HIPCHK(alloc(b.tileList, nI * std::max(c.nTiles, 1) * (size_t)kTileCap * sizeof(unsigned)));
    HIPCHK(alloc(b.tileCnt, nI * std::max(c.nTiles, 1) * sizeof(int)));
    HIPCHK(alloc(b.cellCnt, nI * c.nCellsTotal * 2 * sizeof(int)));
    HIPCHK(alloc(b.cellInfo, nI * c.nCellsTotal * sizeof(CellInfo)));
    HIPCHK(alloc(b.lvlTotal, nI * kMaxLevels * sizeof(int)));
    HIPCHK(alloc(b.lvl, nI * c.candTotal * sizeof(unsigned long long)));
    HIPCHK(alloc(b.slotPos, nI * nf * sizeof(unsigned)));
    HIPCHK(alloc(b.slotResp, nI * nf * sizeof(float)));
    HIPCHK(alloc(b.lvlCount, nI * kMaxLevels * sizeof(int), true));
    HIPCHK(alloc(b.useCost, (nI + 3) & ~(size_t)3, true));               // whole dwords: the kernels read the flags with scalar dword loads
    HIPCHK(alloc(b.kps, nI * nf * sizeof(ivf_keypoint)));
    HIPCHK(alloc(b.desc, nI * nf * 32));
    HIPCHK(alloc(b.count, nI * sizeof(int), true));
    HIPCHK(alloc(b.quality, nI * nf * sizeof(float)));
    if (withStereo) {
        const size_t nP = std::max<size_t>(nI / 2, 1);
        HIPCHK(alloc(b.uright, nP * nf * sizeof(float)));
        HIPCHK(alloc(b.depth, nP * nf * sizeof(float)));
        HIPCHK(alloc(b.sad, nP * nf * sizeof(int)));
        HIPCHK(alloc(b.rowCnt, nP * (size_t)h * sizeof(int)));
        HIPCHK(alloc(b.rowList, nP * (size_t)h * kRowCap * sizeof(unsigned short)));
    }
    HIPCHK(alloc(b.status, 4 * sizeof(int), true));
    b.hugeCount = b.status + 1;
    HIPCHK(alloc(b.tierList, 2 * nI * (size_t)c.nCellsTotal * sizeof(int)));
    if (c.maxCandCap > 4096) {          // kCellCapBig: cells of this geometry can outgrow the LDS selection paths
        HIPCHK(alloc(b.hugeList, (size_t)kHugeListCap * sizeof(int)));
        HIPCHK(alloc(b.hugeScratch, (size_t)kHugeSlots * 4 * c.maxCandCap * sizeof(unsigned)));
    }
    for (int i = 0; i < kEvRing; i++) { HIPCHK(hipEventCreate(&evFast0[i])); HIPCHK(hipEventCreate(&evFast1[i])); }
    HIPCHK(hipEventCreateWithFlags(&evFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&evJoin, hipEventDisableTiming));
    return IVF_OK;
}

void Context::release()
{
    (void)hipSetDevice(device);
    for (void* p : owned) (void)hipFree(p);
    if (hStage) (void)hipHostFree(hStage);
    for (int i = 0; i < kEvRing; i++) {
        if (evFast0[i]) (void)hipEventDestroy(evFast0[i]);
        if (evFast1[i]) (void)hipEventDestroy(evFast1[i]);
    }
    if (evFork) (void)hipEventDestroy(evFork);
    if (evJoin) (void)hipEventDestroy(evJoin);
    *this = Context();
}

// The cost blob of an extractor that ignores the map (enableIntrospection = 0): mvKeyQualScore still reads level 0 of a cost image that comes
// with the frame (Frame.cc:130-143).  Allocated by the first call that needs it; cleared in order on `st`, or blocking when st is null.
int Context::ensure_qpyr(hipStream_t st)
{
    if (b.qpyr) return IVF_OK;
    const size_t blob = (size_t)hc.pyrBytes * maxImg;
    HIPCHK(alloc(b.qpyr, blob));
    if (st) HIPCHK(hipMemsetAsync(b.qpyr, 0, blob, st));
    else HIPCHK(hipMemset(b.qpyr, 0, blob));
    return IVF_OK;
}

// Enqueue ORBextractor::operator() for nImg images (ORB/src/ORBextractor.cc:1224-1296)
int Context::run(const ImageSrc (&side)[2], const ImageSrc* cost, int nImg, const uint8_t* dUseCostSrc, hipStream_t st,
                 hipEvent_t inputsConsumed, hipStream_t sideStream, bool perSide)
{
    if (nImg < 1 || nImg > maxImg) return fail(IVF_E_INVALID, "batch of %d images outside [1,%d]", nImg, maxImg);
    HIPCHK(hipSetDevice(device));
    const bool useQ = introspection && cost != nullptr;
    if (needsCost && !useQ)
        return fail(IVF_E_GEOMETRY, "cell rows leave a pyramid level: this geometry is defined only with a cost map (stale hY, ORBextractor.cc:935-999)");
    if (const int rc = cost ? ensure_qpyr(st) : IVF_OK) return rc;
    if (cost) HIPCHK(hipMemcpyAsync(b.useCost, dUseCostSrc, nImg, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemsetAsync(b.useCost, 0, nImg, st));
    const ImageSrc &s0 = side[0], &s1 = side[nSides - 1];
    if (!perSide && !(s0.code & 3) && !(s1.code & 3) && s0.imageStride == s1.imageStride && s0.rowStride == s1.rowStride)
        launch_ingest(hc, dc, s0.p, s1.p, s0.imageStride, s0.rowStride, nImg, nSides, b.pyr, nullptr, st);
    else
        for (int sd = 0; sd < nSides; sd++) {
            const ImageSrc& q = side[sd];
            if (q.code & 3) launch_ingest_color(hc, dc, q.p, q.imageStride, q.rowStride, q.code, nImg, nSides, sd, b.pyr, st);
            else launch_ingest(hc, dc, q.p, q.p, q.imageStride, q.rowStride, nImg, nSides, b.pyr, nullptr, st, 1 << sd);
        }
    // r06: a cost map that already sits in the level-0 cost plane (ivf_frontend_cost_plane: the FCN wrote it there) needs no copy
    const bool costInPlace = cost && cost->p == b.qpyr + hc.lv[0].off && cost->imageStride == (size_t)nSides * hc.pyrBytes && cost->rowStride == hc.lv[0].pitch;
    if (cost && !costInPlace) launch_ingest(hc, dc, cost->p, cost->p, cost->imageStride, cost->rowStride, nImg, nSides, b.qpyr, b.useCost, st);
    if (inputsConsumed) HIPCHK(hipEventRecord(inputsConsumed, st));   // caller buffers are free from here on
    IVF_MARK(st, markOwn, 1, nRuns);
    launch_pyramid(hc, dc, dTab, b.pyr, useQ ? b.qpyr : nullptr, b.useCost, nImg, st);   // + ComputeQualityImagePyramid :1325-1357
    IVF_MARK(st, markOwn, 2, nRuns);
    HIPCHK(hipMemsetAsync(b.cellCnt, 0, (size_t)nImg * hc.nCellsTotal * 2 * sizeof(int), st));
    HIPCHK(hipMemsetAsync(b.hugeCount, 0, 3 * sizeof(int), st));
    const int slot = (int)(nRuns % kEvRing);
    HIPCHK(hipEventRecord(evFast0[slot], st));
    launch_fast(hc, dc, b, nImg, st);
    HIPCHK(hipEventRecord(evFast1[slot], st));
    IVF_MARK(st, markOwn, 3, nRuns);
    const long long thisRun = nRuns++;
    (void)thisRun;
    static const bool sideBlur = getenv("IVF_NO_SIDE_BLUR") == nullptr;
    if (sideBlur && sideStream && sideStream != st && nImg > 2) {       // not for single frames: there the two event hand-overs cost more than the overlap gives (extraction 0.35 -> 0.63 ms)
        // fork: the blur only needs the pyramid (in order behind it on st); the next run's blur cannot overtake this run's descriptors,
        // because its fork event is recorded on st behind them
        HIPCHK(hipEventRecord(evFork, st));
        HIPCHK(hipStreamWaitEvent(sideStream, evFork, 0));
        IVF_MARK(sideStream, markSide, 1, thisRun);
        launch_blur(hc, dc, b, nImg, sideStream, false);
        IVF_MARK(sideStream, markSide, 2, thisRun);
        // whatever fails from here on, the owning stream joins the side stream's work before this call returns: an un-joined blur
        // would still be writing b.blur when the context is reused or released
        const hipError_t eRec = hipEventRecord(evJoin, sideStream);
        if (eRec == hipSuccess) launch_select(hc, dc, b, nImg, st);
        IVF_MARK(st, markOwn, 4, thisRun);
        const hipError_t eWait = eRec == hipSuccess ? hipStreamWaitEvent(st, evJoin, 0) : eRec;
        if (eWait != hipSuccess) {
            (void)hipStreamSynchronize(sideStream);
            return fail(IVF_E_NO_DEVICE, "joining the side-stream blur failed: %s", hipGetErrorString(eWait));
        }
        IVF_MARK(st, markOwn, 5, thisRun);
    } else {
        launch_select(hc, dc, b, nImg, st);
        IVF_MARK(st, markOwn, 4, thisRun);
        launch_blur(hc, dc, b, nImg, st, true);
        IVF_MARK(st, markOwn, 5, thisRun);
    }
    launch_describe(hc, dc, b, nImg, st);
    IVF_MARK(st, markOwn, 6, thisRun);
    HIPCHK(hipGetLastError());
    return IVF_OK;
}

// Reads AND clears the device-side flags: an error is reported once, for the batch that raised it, and the handle stays
// usable (the flags used to be sticky: one bad image killed a streaming front end until it was re-created).
int Context::check_status(int which)
{
    int s = 0;
    HIPCHK(hipMemcpy(&s, b.status, sizeof(int), hipMemcpyDeviceToHost));
    if (!s) return IVF_OK;
    HIPCHK(hipMemset(b.status, 0, sizeof(int)));
    if (s & 4) return fail(IVF_E_CAPACITY, "batch context %d (run %lld): more than %d cells held over 4096 FAST survivors in one launch",
                           which, nRuns - 1, kHugeListCap);
    return fail(IVF_E_STATE, "batch context %d (run %lld): device-side consistency check failed (flags 0x%x)", which, nRuns - 1, s);
}

// Growable scratch per host thread: a device buffer (per-call entry points -- ivf_stereo_match, ivf_hamming_pairs, the matchers
// built on it, ivf_bow_transform, ivf_distinctive_descriptor -- upload their inputs here instead of paying a hipMalloc /
// hipFree set per call) and a pinned host buffer (row-wise unpacking of pitched device planes).
// Ordering assumption: every user works on the NULL stream and ends with a BLOCKING copy of its results, so two users on
// one thread can never overlap in a buffer.
// Ownership: the buffers live in slots of a process-wide pool.  A thread leases one slot on first use and its thread_local
// destructor only RETURNS the slot to the pool -- no HIP call at thread exit (for the main thread that would run during
// static destruction, possibly after the HIP runtime has gone) and no leak either: the reference starts two fresh
// std::threads per Frame (ORB/src/Frame.cc:116-124), and those now reuse the slots their predecessors gave back instead of
// pinning ~1 MB each for the life of the process.  The pool itself is never destroyed (freed with the process).
struct ScratchSlot { int device = -1; uint8_t* buf = nullptr; size_t cap = 0; uint8_t* pin = nullptr; size_t pinCap = 0; };
struct ScratchPool { std::mutex m; std::vector<ScratchSlot*> idle; int created = 0; };
ScratchPool& scratch_pool() { static ScratchPool* p = new ScratchPool; return *p; }
struct ScratchLease {
    ScratchSlot* s = nullptr;
    ~ScratchLease() { if (s) { ScratchPool& P = scratch_pool(); std::lock_guard<std::mutex> g(P.m); P.idle.push_back(s); s = nullptr; } }
};
ScratchSlot& my_scratch_slot()
{
    static thread_local ScratchLease lease;
    if (!lease.s) {
        ScratchPool& P = scratch_pool();
        std::lock_guard<std::mutex> g(P.m);
        if (!P.idle.empty()) { lease.s = P.idle.back(); P.idle.pop_back(); }
        else { lease.s = new ScratchSlot; P.created++; }
    }
    return *lease.s;
}
}  // namespace

namespace ivf {

int thread_scratch(int device, size_t need, uint8_t** out)
{
    ScratchSlot& sc = my_scratch_slot();
    if (sc.device != device || sc.cap < need) {
        if (sc.buf) { (void)hipSetDevice(sc.device); (void)hipDeviceSynchronize(); (void)hipFree(sc.buf); sc.buf = nullptr; sc.cap = 0; }
        HIPCHK(hipSetDevice(device));
        const size_t cap = std::max(need + need / 2, (size_t)1 << 20);
        HIPCHK(hipMalloc(&sc.buf, cap));
        sc.cap = cap; sc.device = device;
    }
    *out = sc.buf;
    return IVF_OK;
}

int thread_pinned(size_t need, uint8_t** out)
{
    ScratchSlot& sc = my_scratch_slot();
    if (sc.pinCap < need) {
        if (sc.pin) { (void)hipHostFree(sc.pin); sc.pin = nullptr; sc.pinCap = 0; }
        const size_t cap = std::max(need + need / 2, (size_t)1 << 20);
        HIPCHK(hipHostMalloc((void**)&sc.pin, cap, hipHostMallocDefault));
        sc.pinCap = cap;
    }
    *out = sc.pin;
    return IVF_OK;
}

int have_device(int dev)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(IVF_E_NO_DEVICE, "no HIP device available (%s); libivfront has no CPU path",
                                               e == hipSuccess ? "count 0" : hipGetErrorString(e));
    if (dev < 0 || dev >= n) return fail(IVF_E_INVALID, "device_id %d outside [0,%d)", dev, n);
    return IVF_OK;
}

}  // namespace ivf

static std::atomic<long long> g_launches{0};
void ivf::count_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }

int ivf::set_error(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

struct ivf_extractor {
    int var[3] = {0, 0, 0};              // OpenCV-version switches (blur, retain, atan)
    Tables t;
    int device;
    Context ctx;
    bool haveCtx = false;
    int w = 0, h = 0;
    bool lastHadCost = false, extracted = false;
    uint8_t* dOne = nullptr;            // device byte "1"
    // r04: every handle extracts on a stream of its own.  The reference runs the left and the right extractor on two host threads
    // (ORB/src/Frame.cc:116-124) so that they overlap; on the NULL stream the two launch sequences queued one behind the other
    // (bench.py latency_ms_batch1: 0.35 + 0.31 ms back to back).  ivf_extract returns only after its stream has drained, so every
    // later reader of the handle's buffers (ivf_stereo_match, pyramid copies: NULL stream) sees them complete.
    hipStream_t st = nullptr;
};

// kPipe batch contexts on kPipe internal streams: run k uses context k % kPipe, so the latency-bound tail of one batch
// (per-cell selection, descriptors, stereo) overlaps the throughput-bound head (ingest, pyramid, FAST, blur) of the
// next ones.  Results of a run stay valid until kPipe - 1 further runs have been enqueued.
#ifndef IVF_PIPE
#define IVF_PIPE 3
#endif
constexpr int kPipe = IVF_PIPE;         // batch contexts in flight
struct ivf_frontend {
    ivf_frontend_config cfg;
    Tables tl;
    Context ctx[kPipe];
    hipStream_t stream[kPipe] = {};
    hipEvent_t evIn[kPipe] = {}, evConsumed[kPipe] = {}, evDone[kPipe] = {};
    uint8_t* dFlags = nullptr;          // useCost flags when a cost batch is given: [L,R,L,R,...]
    int pairsOf[kPipe] = {};            // batch size of the run each context holds
    long long runs = 0;
    // Frame::UndistortKeyPoints inside the batch (ivf_frontend_set_camera): mvKeysUn of the left frames, one buffer per context
    bool camOn = false;                 // an undistorting camera is set: runs from now on fill kpsUn of their context
    ivf::UndistortCam cam{};
    ivf_keypoint* kpsUn[kPipe] = {};    // addressed like Buffers::kps ([2 * max_pairs][nfeatures], the left frame of pair p at 2 * p: the odd frames are
                                        // never written), so that every consumer of b.kps -- k_pack_gather -- runs unchanged; allocated by the first undistorting camera, owned by ctx[k]
    bool unOf[kPipe] = {};              // the run each context holds was made with a camera
    int last() const { return (int)((runs + kPipe - 1) % kPipe); }      // context of the most recent run
};

// context *k of the batch `age` runs back (0 = the last run; a batch is held until kPipe - 1 further runs were enqueued)
static int held_batch(const ivf_frontend* fe, int age, int* k)
{
    if (age < 0 || age >= kPipe || fe->runs <= age) return fail(IVF_E_STATE, "no batch of age %d is held", age);
    *k = (int)((fe->runs - 1 - age) % kPipe);
    return IVF_OK;
}

// Image (pair, side) of the batch context k holds: images are interleaved [L0,R0,L1,R1,...], the stereo results are per pair and belong
// to the left image.  kps is what a Frame reads, mvKeysUn (Frame.cc:424): kpsUn for the left image of a run made with a camera, else mvKeys.
static BatchImage batch_image(const ivf_frontend* fe, int k, int pair, int side)
{
    const Buffers& b = fe->ctx[k].b;
    const size_t nf = fe->ctx[k].hc.nfeatures, img = (size_t)pair * 2 + side;
    BatchImage im;
    im.mvKeys = b.kps + img * nf;
    im.kps = (side == 0 && fe->unOf[k]) ? fe->kpsUn[k] + img * nf : im.mvKeys;
    im.desc = b.desc + img * nf * 32;
    im.uright = side == 0 ? b.uright + (size_t)pair * nf : nullptr;
    im.depth = side == 0 ? b.depth + (size_t)pair * nf : nullptr;
    im.quality = b.quality + img * nf;
    im.count = b.count + img; im.cap = (int)nf; im.done = fe->evDone[k];
    return im;
}

extern "C" {

int ivf_version(void) { return 100; }
long long ivf_debug_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }
int ivf_debug_scratch_slots(void) { ScratchPool& P = scratch_pool(); std::lock_guard<std::mutex> g(P.m); return P.created; }
const char* ivf_last_error(void) { return g_err.c_str(); }
int ivf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ivf_extractor_create(const ivf_extractor_params* params, int device_id, ivf_extractor** out)
{
    if (!params || !out) return fail(IVF_E_INVALID, "null argument");
    *out = nullptr;
    Tables t;
    int rc = make_tables(*params, t);
    if (rc) return rc;
    rc = have_device(device_id);
    if (rc) return rc;
    ivf_extractor* e = new ivf_extractor();
    e->t = t; e->device = device_id;
    *out = e;
    return IVF_OK;
}

void ivf_extractor_destroy(ivf_extractor* e)
{
    if (!e) return;
    if (e->haveCtx) e->ctx.release();
    if (e->dOne) (void)hipFree(e->dOne);
    if (e->st) (void)hipStreamDestroy(e->st);
    delete e;
}

int ivf_extractor_set_opencv_variant(ivf_extractor* e, int blur, int retain_best, int atan2)
{
    if (!e) return fail(IVF_E_INVALID, "null handle");
    e->var[0] = blur; e->var[1] = retain_best; e->var[2] = atan2;
    return e->haveCtx ? e->ctx.set_variant(e->var) : IVF_OK;
}

int ivf_frontend_set_opencv_variant(ivf_frontend* fe, int blur, int retain_best, int atan2)
{
    if (!fe) return fail(IVF_E_INVALID, "null handle");
    const int v[3] = {blur, retain_best, atan2};
    for (int k = 0; k < kPipe; k++) { const int rc = fe->ctx[k].set_variant(v); if (rc) return rc; }
    return IVF_OK;
}

int ivf_extractor_get_levels(const ivf_extractor* e) { return e ? e->t.p.nlevels : fail(IVF_E_INVALID, "null handle"); }
float ivf_extractor_get_scale_factor(const ivf_extractor* e) { return e ? e->t.p.scale_factor : 0.f; }

int ivf_extractor_get_scale_tables(const ivf_extractor* e, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2)
{
    if (!e) return fail(IVF_E_INVALID, "null handle");
    const int n = e->t.p.nlevels;
    if (scale) memcpy(scale, e->t.scale, n * sizeof(float));
    if (inv_scale) memcpy(inv_scale, e->t.invScale, n * sizeof(float));
    if (sigma2) memcpy(sigma2, e->t.sigma2, n * sizeof(float));
    if (inv_sigma2) memcpy(inv_sigma2, e->t.invSigma2, n * sizeof(float));
    return IVF_OK;
}

int ivf_extractor_get_feature_tables(const ivf_extractor* e, int32_t* features_per_level, int32_t* umax16)
{
    if (!e) return fail(IVF_E_INVALID, "null handle");
    if (features_per_level) memcpy(features_per_level, e->t.nfeat, e->t.p.nlevels * sizeof(int));
    if (umax16) memcpy(umax16, e->t.umax, 16 * sizeof(int));
    return IVF_OK;
}

int ivf_extract(ivf_extractor* e, const uint8_t* image, int width, int height, int stride,
                const uint8_t* cost, int cost_stride, ivf_keypoint* kps, uint8_t* desc, int cap, int* n_out)
{
    if (!e || !n_out) return fail(IVF_E_INVALID, "null argument");
    *n_out = 0;
    if (!image || width <= 0 || height <= 0) return IVF_OK;      // empty image: silent return (:1227-1228)
    if (stride < width || (cost && cost_stride < width)) return fail(IVF_E_INVALID, "stride smaller than width");
    int rc = have_device(e->device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    if (!e->haveCtx || e->w != width || e->h != height) {
        if (e->haveCtx) { e->ctx.release(); e->haveCtx = false; }
        rc = e->ctx.build(e->t, width, height, 1, 1, e->device, true, e->var);
        if (rc) { e->ctx.release(); return rc; }
        // staging is part of the context: the handle only counts as built once all of it exists (release() frees what does)
        e->ctx.stageBytes = ((size_t)width * height * 2 + 15) & ~(size_t)15;       // keypoints / counters behind it stay 16-byte aligned
        if (e->ctx.alloc(e->ctx.dStage, e->ctx.stageBytes) != hipSuccess ||
            hipHostMalloc((void**)&e->ctx.hStage, e->ctx.stageBytes + (size_t)e->t.p.nfeatures * (sizeof(ivf_keypoint) + 32) + 64, hipHostMallocDefault) != hipSuccess ||
            (!e->dOne && (hipMalloc(&e->dOne, 1) != hipSuccess || hipMemset(e->dOne, 1, 1) != hipSuccess)) ||
            (!e->st && hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking) != hipSuccess)) {
            e->ctx.release();
            return fail(IVF_E_NO_DEVICE, "staging allocation failed for a %dx%d extractor", width, height);
        }
        e->haveCtx = true; e->w = width; e->h = height;
        HIPCHK(hipDeviceSynchronize());      // the context's buffers were cleared on the NULL stream: done before the handle's own stream touches them
    }
    e->extracted = false;
    Context& c = e->ctx;
    uint8_t* dImg = c.dStage;
    uint8_t* dCost = c.dStage + (size_t)width * height;
    // the caller's image is pageable memory (a cv::Mat): rows go through the handle's pinned staging buffer -- one host memcpy
    // and one DMA instead of a row-by-row pageable hipMemcpy2D (measured 2.9 ms of a 3.1 ms call); results come back the same way
    const size_t px = (size_t)width * height, nfe = (size_t)e->t.p.nfeatures;
    uint8_t* hImg = c.hStage; uint8_t* hCost = hImg + px;
    ivf_keypoint* hK = (ivf_keypoint*)(c.hStage + c.stageBytes); uint8_t* hD = (uint8_t*)(hK + nfe); int* hN = (int*)(hD + nfe * 32);
    for (int y = 0; y < height; y++) memcpy(hImg + (size_t)y * width, image + (size_t)y * stride, (size_t)width);
    const bool useCost = cost && e->t.p.enable_introspection;
    if (useCost) for (int y = 0; y < height; y++) memcpy(hCost + (size_t)y * width, cost + (size_t)y * cost_stride, (size_t)width);
    // from the first enqueue on, every way out of this call leaves the handle's stream DRAINED (r04 ADVICE): the next call memcpy's
    // into hStage and the NULL-stream readers (ivf_stereo_match, the pyramid copies) touch the context's buffers -- work of a call
    // that failed half-way must not still be in flight then (the stream is non-blocking: the NULL stream does not order it)
    struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{e->st};
    HIPCHK(hipMemcpyAsync(dImg, hImg, useCost ? 2 * px : px, hipMemcpyHostToDevice, e->st));
    const ImageSrc img{dImg, px, width, 0}, costSrc{dCost, px, width, 0};
    rc = c.run({img, img}, useCost ? &costSrc : nullptr, 1, e->dOne, e->st);
    if (rc) return rc;
    // counts are not known before the kernels finish: fetch the count and the full-capacity result arrays in one go (56 KB at N = 1000)
    HIPCHK(hipMemcpyAsync(hN, c.b.count, sizeof(int), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(hN + 1, c.b.status, sizeof(int), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(hK, c.b.kps, nfe * sizeof(ivf_keypoint), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(hD, c.b.desc, nfe * 32, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    const int n = *hN;
    if (hN[1]) { rc = c.check_status(); if (rc) return rc; }      // device-side flags raised: read, clear and report them
    e->lastHadCost = useCost; e->extracted = true;
    if (n > cap) { *n_out = n; return fail(IVF_E_CAPACITY, "%d keypoints exceed caller capacity %d", n, cap); }
    if (n > 0) {
        if (!kps || !desc) return fail(IVF_E_INVALID, "null output buffers");
        memcpy(kps, hK, (size_t)n * sizeof(ivf_keypoint));
        memcpy(desc, hD, (size_t)n * 32);
    }
    *n_out = n;
    return IVF_OK;
}

static int copy_level(const ivf_extractor* e, const uint8_t* blob, int level, uint8_t* dst, int dst_stride, int* width, int* height)
{
    if (!e || !e->extracted || !blob) return fail(IVF_E_STATE, "no pyramid: call ivf_extract first");
    if (level < 0 || level >= e->t.p.nlevels) return fail(IVF_E_INVALID, "level %d out of range", level);
    const LevelGeom& G = e->ctx.hc.lv[level];
    if (width) *width = G.w;
    if (height) *height = G.h;
    if (!dst) return IVF_OK;
    if (dst_stride < G.w) return fail(IVF_E_INVALID, "dst_stride smaller than level width");
    HIPCHK(hipSetDevice(e->device));
    // pitched level -> caller rows through the calling thread's pinned scratch (a pageable 2-D copy runs row by row)
    uint8_t* pin = nullptr;
    const size_t bytes = (size_t)G.pitch * G.h;
    const int prc = thread_pinned(bytes, &pin);
    if (prc) return prc;
    HIPCHK(hipMemcpy(pin, blob + G.off, bytes, hipMemcpyDeviceToHost));
    for (int y = 0; y < G.h; y++) memcpy(dst + (size_t)y * dst_stride, pin + (size_t)y * G.pitch, (size_t)G.w);
    return IVF_OK;
}
int ivf_extractor_pyramid_level(const ivf_extractor* e, int level, uint8_t* dst, int dst_stride, int* width, int* height)
{
    return copy_level(e, e ? e->ctx.b.pyr : nullptr, level, dst, dst_stride, width, height);
}
int ivf_extractor_quality_level(const ivf_extractor* e, int level, uint8_t* dst, int dst_stride, int* width, int* height)
{
    if (e && !e->lastHadCost) return fail(IVF_E_STATE, "last extract had no cost map");
    return copy_level(e, e ? e->ctx.b.qpyr : nullptr, level, dst, dst_stride, width, height);
}
int ivf_extractor_blur_level(const ivf_extractor* e, int level, uint8_t* dst, int dst_stride, int* width, int* height)
{
    if (e && e->extracted && level >= 0 && level < e->t.p.nlevels) {
        int cnt = 0;
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipMemcpy(&cnt, e->ctx.b.lvlCount + level, sizeof(int), hipMemcpyDeviceToHost));
        if (cnt == 0) return fail(IVF_E_STATE, "level %d had no keypoints in the last extract: not blurred (ORBextractor.cc:1267-1268)", level);
    }
    return copy_level(e, e ? e->ctx.b.blur : nullptr, level, dst, dst_stride, width, height);
}
int ivf_extractor_level_counts(const ivf_extractor* e, int32_t* counts)
{
    if (!e || !counts) return fail(IVF_E_INVALID, "null argument");
    if (!e->extracted) return fail(IVF_E_STATE, "call ivf_extract first");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpy(counts, e->ctx.b.lvlCount, e->t.p.nlevels * sizeof(int), hipMemcpyDeviceToHost));
    return IVF_OK;
}

int ivf_stereo_match(const ivf_extractor* left, const ivf_extractor* right,
                     const ivf_keypoint* kps_left, int n_left, const uint8_t* desc_left,
                     const ivf_keypoint* kps_right, int n_right, const uint8_t* desc_right,
                     float bf, float b, float* u_right, float* depth)
{
    if (!left || !right || !u_right || !depth || n_left < 0 || n_right < 0) return fail(IVF_E_INVALID, "bad argument");
    if (!left->extracted || !right->extracted) return fail(IVF_E_STATE, "both extractors must have run ivf_extract");
    if (left->device != right->device) return fail(IVF_E_INVALID, "extractors live on different devices");
    if (left->w != right->w || left->h != right->h || left->t.p.nlevels != right->t.p.nlevels)
        return fail(IVF_E_INVALID, "left/right geometry differs");
    const int nf = left->t.p.nfeatures;
    if (n_left > nf || n_right > 65534) return fail(IVF_E_CAPACITY, "too many keypoints");
    if (n_left == 0) return IVF_OK;
    HIPCHK(hipSetDevice(left->device));
    // caller-provided keypoints / descriptors are the matcher's inputs (mvKeys, mvDescriptors): upload them into the
    // calling thread's growable device scratch (no per-frame hipMalloc / hipFree, nothing to leak on an error path)
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t nR = (size_t)std::max(n_right, 1);
    const size_t szKL = up((size_t)nf * sizeof(ivf_keypoint)), szKR = up(nR * sizeof(ivf_keypoint)), szDL = up((size_t)nf * 32),
                 szDR = up(nR * 32);
    uint8_t* base = nullptr;
    int rc = thread_scratch(left->device, szKL + szKR + szDL + szDR + 256, &base);
    if (rc) return rc;
    ivf_keypoint* dKL = (ivf_keypoint*)base; ivf_keypoint* dKR = (ivf_keypoint*)(base + szKL);
    uint8_t* dDL = base + szKL + szKR; uint8_t* dDR = dDL + szDL; int* dCnt = (int*)(dDR + szDR);
    HIPCHK(hipMemcpyAsync(dKL, kps_left, (size_t)n_left * sizeof(ivf_keypoint), hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(dDL, desc_left, (size_t)n_left * 32, hipMemcpyHostToDevice, nullptr));
    if (n_right) {
        HIPCHK(hipMemcpyAsync(dKR, kps_right, (size_t)n_right * sizeof(ivf_keypoint), hipMemcpyHostToDevice, nullptr));
        HIPCHK(hipMemcpyAsync(dDR, desc_right, (size_t)n_right * 32, hipMemcpyHostToDevice, nullptr));
    }
    const int cnt[2] = {n_left, n_right};
    HIPCHK(hipMemcpyAsync(dCnt, cnt, sizeof cnt, hipMemcpyHostToDevice, nullptr));
    const Context& cl = left->ctx;
    StereoArgs A;
    A.pyrL = cl.b.pyr; A.pyrR = right->ctx.b.pyr; A.pyrStride = 0;
    A.kpL = dKL; A.kpR = dKR; A.descL = dDL; A.descR = dDR; A.cntL = dCnt; A.cntR = dCnt + 1;
    A.kpStride = 0; A.cntStride = 0;
    A.uright = cl.b.uright; A.depth = cl.b.depth; A.sad = cl.b.sad; A.outStride = nf;
    A.bf = bf; A.bb = b; A.rowCnt = cl.b.rowCnt; A.rowList = cl.b.rowList;
    launch_stereo_args(cl.hc, cl.dc, A, 1, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(u_right, cl.b.uright, (size_t)n_left * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(depth, cl.b.depth, (size_t)n_left * sizeof(float), hipMemcpyDeviceToHost));
    return IVF_OK;
}

// ---- Frame::UndistortKeyPoints / ComputeImageBounds (ORB/src/Frame.cc:696-756) ----
static int check_camera(const ivf_camera* cam)
{
    if (!cam) return fail(IVF_E_INVALID, "null camera");
    const int nd = cam->n_dist;
    if (!(nd == 0 || nd == 4 || nd == 5 || nd == 8 || nd == 12))
        return fail(IVF_E_INVALID, "distortion vector of %d coefficients (0, 4, 5, 8 or 12; tilt terms are not supported)", nd);
    return IVF_OK;
}
// mDistCoef.at<float>(0) == 0.0 is the reference's only test (Frame.cc:698, :730)
static bool camera_undistorts(const ivf_camera& cam) { return cam.n_dist > 0 && cam.dist[0] != 0.0f; }

int ivf_image_bounds(const ivf_camera* cam, int width, int height, ivf_bounds* out)
{
    if (!out) return fail(IVF_E_INVALID, "null argument");
    int rc = check_camera(cam);
    if (rc) return rc;
    if (width < 1 || height < 1) return fail(IVF_E_INVALID, "bad image size %dx%d", width, height);
    if (!camera_undistorts(*cam)) { *out = ivf_bounds{0.0f, 0.0f, (float)width, (float)height}; return IVF_OK; }      // Frame.cc:749-755
    const ivf::UndistortCam c = ivf::undistort_cam(*cam);
    const float cx[4] = {0.0f, (float)width, 0.0f, (float)width}, cy[4] = {0.0f, 0.0f, (float)height, (float)height};   // :732-736
    float x[4], y[4];
    for (int i = 0; i < 4; i++) ivf::undistort_point(c, cx[i], cy[i], x[i], y[i]);
    out->min_x = std::min(x[0], x[2]); out->max_x = std::max(x[1], x[3]);      // :743-746
    out->min_y = std::min(y[0], y[1]); out->max_y = std::max(y[2], y[3]);
    return IVF_OK;
}

int ivf_undistort_keypoints(const ivf_camera* cam, const ivf_keypoint* kps, int n, ivf_keypoint* out, int device_id)
{
    int rc = check_camera(cam);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!kps || !out))) return fail(IVF_E_INVALID, "bad argument");
    if (n == 0) return IVF_OK;
    if (!camera_undistorts(*cam)) { if (out != kps) memmove(out, kps, (size_t)n * sizeof(ivf_keypoint)); return IVF_OK; }   // Frame.cc:698-702
    rc = have_device(device_id);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device_id));
    const size_t bytes = (size_t)n * sizeof(ivf_keypoint);
    uint8_t* d = nullptr;
    rc = thread_scratch(device_id, bytes + 16, &d);
    if (rc) return rc;
    int* dCount = (int*)d;
    ivf_keypoint* dK = (ivf_keypoint*)(d + 16);
    HIPCHK(hipMemcpy(dCount, &n, sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dK, kps, bytes, hipMemcpyHostToDevice));
    launch_undistort_keys(ivf::undistort_cam(*cam), false, dK, 0, dCount, 0, 1, n, dK, 0, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dK, bytes, hipMemcpyDeviceToHost));
    return IVF_OK;
}

int ivf_undistort_keypoints_device(const ivf_camera* cam, const ivf_keypoint* d_kps, const int32_t* d_count, int n_frames, int cap,
                                   ivf_keypoint* d_out, void* hip_stream)
{
    int rc = check_camera(cam);
    if (rc) return rc;
    if (n_frames < 0 || cap < 0 || n_frames > 65535) return fail(IVF_E_INVALID, "n_frames %d outside [0,65535] or negative cap %d", n_frames, cap);
    if (n_frames == 0 || cap == 0) return IVF_OK;
    if (!d_kps || !d_count || !d_out) return fail(IVF_E_INVALID, "null argument");
    if ((((size_t)d_kps | (size_t)d_out) & 7) != 0) return fail(IVF_E_INVALID, "keypoint arrays must be 8-byte aligned");
    const bool on = camera_undistorts(*cam);
    if (!on && d_out == d_kps) return IVF_OK;
    launch_undistort_keys(ivf::undistort_cam(*cam), !on, d_kps, (size_t)cap, d_count, 1, n_frames, cap, d_out, (size_t)cap, (hipStream_t)hip_stream);
    HIPCHK(hipGetLastError());
    return IVF_OK;
}

// testing hook (see include/ivfront.h)
int ivf_test_retain_best(const float* responses, int n, int n_points, int32_t* order_out, int device_id)
{
    if (!responses || !order_out || n < 1 || n > 65536 || n_points < 0) return fail(IVF_E_INVALID, "bad argument (1 <= n <= 65536)");
    int rc = have_device(device_id);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device_id));
    // responses, order, and above 4096 elements the flag and the global lists of k_test_retain_best: u64[2 * n] + u32[2 * n]
    const bool global = n > 4096;
    const size_t szR = ((size_t)n * 4 + 255) & ~(size_t)255;
    uint8_t* scb = nullptr;
    rc = thread_scratch(device_id, 2 * szR + (global ? 256 + (size_t)n * 24 : 0), &scb);
    if (rc) return rc;
    float* dR = (float*)scb; int* dO = (int*)(scb + szR);
    int* dDiffer = global ? (int*)(scb + 2 * szR) : nullptr;
    unsigned long long* dLists = global ? (unsigned long long*)(scb + 2 * szR + 256) : nullptr;
    HIPCHK(hipMemcpyAsync(dR, responses, (size_t)n * sizeof(float), hipMemcpyHostToDevice, nullptr));
    if (global) HIPCHK(hipMemsetAsync(dDiffer, 0, sizeof(int), nullptr));
    launch_test_retain_best(dR, n, n_points, dO, dLists, dDiffer, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(order_out, dO, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    int differ = 0;
    if (global) HIPCHK(hipMemcpy(&differ, dDiffer, sizeof(int), hipMemcpyDeviceToHost));
    if (differ) return fail(IVF_E_STATE, "the wave-cooperative and the one-thread replay of nth_element disagree (n %d, n_points %d)", n, n_points);
    return IVF_OK;
}

// ---- batched stereo front end ----
// The kPipe internal streams of a device: created on first use, shared by every ivf_frontend on that device, never destroyed (no HIP
// call during static destruction).  The tail kernels of a batch are small and latency-bound: on high-priority streams they slot in
// beside whatever large kernels the caller's stream is running (the FCN of the next batch) instead of queueing behind them.
static int internal_streams(int device, hipStream_t (&out)[kPipe])
{
    struct Set { hipStream_t s[kPipe]; };
    static std::mutex* m = new std::mutex();
    static std::map<int, Set>* sets = new std::map<int, Set>();
    std::lock_guard<std::mutex> g(*m);
    auto it = sets->find(device);
    if (it == sets->end()) {
        HIPCHK(hipSetDevice(device));
        int prLo = 0, prHi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prLo, &prHi);
        static const bool noPrio = IVF_EXP_ENV("IVF_NO_STREAM_PRIORITY") != nullptr;
        Set st{};
        for (int k = 0; k < kPipe; k++)
            if ((noPrio ? hipStreamCreateWithFlags(&st.s[k], hipStreamNonBlocking)
                        : hipStreamCreateWithPriority(&st.s[k], hipStreamNonBlocking, prHi)) != hipSuccess) {
                for (int j = 0; j < k; j++) (void)hipStreamDestroy(st.s[j]);
                return fail(IVF_E_NO_DEVICE, "stream creation failed");
            }
        it = sets->emplace(device, st).first;
    }
    for (int k = 0; k < kPipe; k++) out[k] = it->second.s[k];
    return IVF_OK;
}

int ivf_frontend_create(const ivf_frontend_config* cfg, ivf_frontend** out)
{
    if (!cfg || !out) return fail(IVF_E_INVALID, "null argument");
    *out = nullptr;
    const ivf_extractor_params &L = cfg->left, &R = cfg->right;
    if (L.nfeatures != R.nfeatures || L.scale_factor != R.scale_factor || L.nlevels != R.nlevels ||
        L.ini_th_fast != R.ini_th_fast || L.min_th_fast != R.min_th_fast)
        return fail(IVF_E_INVALID, "left/right extractor parameters may differ only in enable_introspection");
    if (cfg->max_pairs < 1) return fail(IVF_E_INVALID, "max_pairs must be >= 1");
    if (!(cfg->b > 0.f) || !(cfg->bf > 0.f)) return fail(IVF_E_INVALID, "bf and b must be positive");
    Tables t;
    ivf_extractor_params p = L;
    p.enable_introspection = (L.enable_introspection || R.enable_introspection) ? 1 : 0;
    int rc = make_tables(p, t);
    if (rc) return rc;
    rc = have_device(cfg->device_id);
    if (rc) return rc;
    ivf_frontend* fe = new ivf_frontend();
    fe->cfg = *cfg; fe->tl = t;
    auto cleanup = [&](int code) { ivf_frontend_destroy(fe); return code; };
    for (int k = 0; k < kPipe; k++) {
        rc = fe->ctx[k].build(t, cfg->width, cfg->height, 2 * cfg->max_pairs, 2, cfg->device_id, true);
        if (rc) return cleanup(rc);
        fe->ctx[k].markOwn = k; fe->ctx[k].markSide = 3 + (k + 1) % kPipe;
        // r05: the kPipe internal streams come from a process-wide pool per device (internal_streams above) and are SHARED by every
        // front end on that device.  Streams are a scarce resource on this runtime -- it multiplexes them onto a few hardware queues
        // (three more streams cost configs[2] 15 % just by existing) -- so a second front end in the process
        // (bench.py's configs[1] leg beside the configs[2] one; Tracking's left / right / initialisation extractors) must not add any,
        // and a create-run-destroy loop no longer creates and destroys streams at all.  Two front ends that share streams serialise
        // against each other on them, which is what they would do on the GPU anyway.
        hipStream_t pool[kPipe];
        rc = internal_streams(cfg->device_id, pool);
        if (rc) return cleanup(rc);
        fe->stream[k] = pool[k];
        const unsigned evFlags = hipEventDisableTiming;
        if (hipEventCreateWithFlags(&fe->evIn[k], evFlags) != hipSuccess ||
            hipEventCreateWithFlags(&fe->evConsumed[k], evFlags) != hipSuccess ||
            hipEventCreateWithFlags(&fe->evDone[k], evFlags) != hipSuccess)
            return cleanup(fail(IVF_E_NO_DEVICE, "event creation failed"));
    }
    std::vector<uint8_t> flags(2 * (size_t)cfg->max_pairs);
    // bit 0: the cost pyramid gates this image's extraction; bit 1: mvKeyQualScore of the LEFT keypoints reads the cost image
    // whenever one is passed, whatever the extractor flags say (Frame.cc:130-143 tests only !imDepth.empty())
    for (int i = 0; i < cfg->max_pairs; i++) { flags[2 * i] = (L.enable_introspection ? 1 : 0) | 2; flags[2 * i + 1] = R.enable_introspection ? 1 : 0; }
    if (hipMalloc(&fe->dFlags, flags.size()) != hipSuccess ||
        hipMemcpy(fe->dFlags, flags.data(), flags.size(), hipMemcpyHostToDevice) != hipSuccess)
        return cleanup(fail(IVF_E_NO_DEVICE, "flag upload failed"));
    *out = fe;
    return IVF_OK;
}

void ivf_frontend_destroy(ivf_frontend* fe)
{
    if (!fe) return;
    (void)hipSetDevice(fe->cfg.device_id);
    // r06: wait for THIS handle's batches (their completion events), not for the device: the internal streams are shared by every front end of
    // the process on this device (internal_streams), so a device-wide wait made one camera's tear-down wait for the other's work.  Work the caller
    // put behind a batch on a lent stream (ivf_frontend_batch_stream) is the caller's to finish first, as ivfront.h says; the buffer releases below
    // go through hipFree, which itself does not return while the device still uses the allocation.
    for (int k = 0; k < kPipe; k++)
        if (fe->evDone[k]) (void)hipEventSynchronize(fe->evDone[k]);      // never recorded = complete
    if (fe->dFlags) (void)hipFree(fe->dFlags);
    for (int k = 0; k < kPipe; k++) {
        fe->ctx[k].release();
        // fe->stream[k] belongs to the process-wide pool: never destroyed
        if (fe->evIn[k]) (void)hipEventDestroy(fe->evIn[k]);
        if (fe->evConsumed[k]) (void)hipEventDestroy(fe->evConsumed[k]);
        if (fe->evDone[k]) (void)hipEventDestroy(fe->evDone[k]);
    }
    delete fe;
}

// One batch on the next context: side[0 / 1] the left / right images, cost the cost maps or null (Context::run)
static int frontend_run(ivf_frontend* fe, const ImageSrc (&side)[2], const ImageSrc* cost, int n_pairs, void* hip_stream, bool perSide)
{
    hipStream_t caller = (hipStream_t)hip_stream;
    const int k = (int)(fe->runs % kPipe);
    Context& c = fe->ctx[k];
    hipStream_t st = fe->stream[k];
    HIPCHK(hipSetDevice(fe->cfg.device_id));
    // order: everything the caller enqueued so far (it produced the inputs) -> this batch
    IVF_MARK_HOST(6, (fe->runs << 8) | 1);
    HIPCHK(hipEventRecord(fe->evIn[k], caller));
    HIPCHK(hipStreamWaitEvent(st, fe->evIn[k], 0));
    // the blur of this batch is lent the internal stream of the NEXT context: whatever older batch that stream still holds does not
    // depend on this one, and the next batch queues behind the blur
    int rc = c.run(side, cost, 2 * n_pairs, fe->dFlags, st, fe->evConsumed[k], fe->stream[(k + 1) % kPipe], perSide);
    if (rc) return rc;
    launch_stereo(c.hc, c.dc, c.b, n_pairs, fe->cfg.bf, fe->cfg.b, st);
    IVF_MARK(st, c.markOwn, 7, c.nRuns - 1);
    // Frame::UndistortKeyPoints (Frame.cc:145, :696-726): the left frames only (images are interleaved L,R: every second frame of b.kps)
    if (fe->camOn)
        launch_undistort_keys(fe->cam, false, c.b.kps, (size_t)2 * c.hc.nfeatures, c.b.count, 2, n_pairs, c.hc.nfeatures, fe->kpsUn[k],
                              (size_t)2 * c.hc.nfeatures, st);
    fe->unOf[k] = fe->camOn;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(fe->evDone[k], st));
    // the caller's stream may overwrite its input buffers once they have been ingested
    HIPCHK(hipStreamWaitEvent(caller, fe->evConsumed[k], 0));
    fe->pairsOf[k] = n_pairs;
    IVF_MARK_HOST(6, (fe->runs << 8) | 2);
    fe->runs++;
    return IVF_OK;
}

int ivf_frontend_run(ivf_frontend* fe, const uint8_t* d_left, const uint8_t* d_right, const uint8_t* d_cost,
                     size_t image_stride, int row_stride, int n_pairs, void* hip_stream)
{
    if (!fe || !d_left || !d_right) return fail(IVF_E_INVALID, "null argument");
    if (n_pairs < 1 || n_pairs > fe->cfg.max_pairs) return fail(IVF_E_INVALID, "n_pairs %d outside [1,%d]", n_pairs, fe->cfg.max_pairs);
    if (row_stride < fe->cfg.width || image_stride < (size_t)row_stride * (fe->cfg.height - 1) + fe->cfg.width)
        return fail(IVF_E_INVALID, "strides too small for %dx%d", fe->cfg.width, fe->cfg.height);
    const ImageSrc cost{d_cost, image_stride, row_stride, 0};
    return frontend_run(fe, {{d_left, image_stride, row_stride, 0}, {d_right, image_stride, row_stride, 0}}, d_cost ? &cost : nullptr, n_pairs,
                        hip_stream, false);
}

int ivf_frontend_cost_plane(ivf_frontend* fe, uint8_t** d_plane, size_t* image_stride, int* row_stride, void* hip_stream)
{
    if (!fe || !d_plane || !image_stride || !row_stride) return fail(IVF_E_INVALID, "null argument");
    const int k = (int)(fe->runs % kPipe);
    Context& c = fe->ctx[k];
    HIPCHK(hipSetDevice(fe->cfg.device_id));
    if (const int rc = c.ensure_qpyr(nullptr)) return rc;
    // the context's previous batch (three runs ago) read this plane: the caller's stream may write it once that batch is done
    if (fe->runs >= kPipe) HIPCHK(hipStreamWaitEvent((hipStream_t)hip_stream, fe->evDone[k], 0));
    *d_plane = c.b.qpyr + c.hc.lv[0].off;
    *image_stride = (size_t)2 * c.hc.pyrBytes;
    *row_stride = c.hc.lv[0].pitch;
    return IVF_OK;
}

int ivf_frontend_run_color(ivf_frontend* fe, const uint8_t* d_left, int left_code, size_t left_image_stride, int left_row_stride,
                           const uint8_t* d_right, int right_code, size_t right_image_stride, int right_row_stride,
                           const uint8_t* d_cost, size_t cost_image_stride, int cost_row_stride, int n_pairs, void* hip_stream)
{
    if (!fe || !d_left || !d_right) return fail(IVF_E_INVALID, "null argument");
    if (n_pairs < 1 || n_pairs > fe->cfg.max_pairs) return fail(IVF_E_INVALID, "n_pairs %d outside [1,%d]", n_pairs, fe->cfg.max_pairs);
    const ImageSrc side[2] = {{d_left, left_image_stride, left_row_stride, left_code}, {d_right, right_image_stride, right_row_stride, right_code}};
    for (int sd = 0; sd < 2; sd++) {
        const ImageSrc& q = side[sd];
        if (q.code < 0 || (q.code & 3) == 3 || q.code > 7 || (!(q.code & 3) && q.code))
            return fail(IVF_E_INVALID, "side %d: colour code %d is not 0 (grey), 1 (bytes B,G,R) or 2 (bytes R,G,B), the last two optionally + 4 (OpenCV <= 3 coefficients)", sd, q.code);
        const int ch = (q.code & 3) ? 3 : 1;
        if (q.rowStride < ch * fe->cfg.width || q.imageStride < (size_t)q.rowStride * (fe->cfg.height - 1) + (size_t)ch * fe->cfg.width)
            return fail(IVF_E_INVALID, "side %d: strides too small for %dx%d x %d channel(s)", sd, fe->cfg.width, fe->cfg.height, ch);
    }
    if (d_cost && (cost_row_stride < fe->cfg.width || cost_image_stride < (size_t)cost_row_stride * (fe->cfg.height - 1) + fe->cfg.width))
        return fail(IVF_E_INVALID, "cost strides too small for %dx%d", fe->cfg.width, fe->cfg.height);
    const ImageSrc cost{d_cost, cost_image_stride, cost_row_stride, 0};
    return frontend_run(fe, side, d_cost ? &cost : nullptr, n_pairs, hip_stream, true);
}

int ivf_frontend_sync(ivf_frontend* fe)
{
    if (!fe) return fail(IVF_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(fe->cfg.device_id));
    for (int k = 0; k < kPipe; k++) {
        IVF_MARK_HOST(7, 0x10 + k);
        HIPCHK(hipStreamSynchronize(fe->stream[k]));
        const int rc = fe->ctx[k].check_status(k);
        if (rc) return rc;
    }
    IVF_MARK_HOST(7, 0x20);
    return IVF_OK;
}

#ifdef IVF_EXPERIMENT
// soak aid, experiment builds only (not declared in include/ivfront.h): `words` = at least 8 ints of host memory the CALLER keeps
// alive (e.g. a MAP_SHARED file mapping its parent process also maps); registered with the runtime here, written by the marker
// launches from then on.  words == NULL switches the markers off again.
extern "C" __attribute__((visibility("default"))) int ivf_debug_progress_words(int* words, int n_words, int device_id)
{
    if (!words) { g_markDev = nullptr; g_markHost = nullptr; return IVF_OK; }
    if (n_words < 8) return fail(IVF_E_INVALID, "need at least 8 progress words");
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipHostRegister(words, (size_t)n_words * sizeof(int), hipHostRegisterMapped));
    void* d = nullptr;
    HIPCHK(hipHostGetDevicePointer(&d, words, 0));
    g_markDev = (int*)d; g_markHost = words;
    return IVF_OK;
}
#endif

int ivf_frontend_device_results(const ivf_frontend* fe, int side, const ivf_keypoint** d_kps, const uint8_t** d_desc,
                                const int32_t** d_count, const float** d_uright, const float** d_depth,
                                const float** d_quality, int* cap)
{
    if (!fe || side < 0 || side > 1) return fail(IVF_E_INVALID, "bad argument");
    // base of the side: pair p lies p * 2 * cap elements (counts: 2 p) further on, the stereo results p * cap
    const BatchImage im = batch_image(fe, fe->last(), 0, side);
    if (d_kps) *d_kps = im.mvKeys;
    if (d_desc) *d_desc = im.desc;
    if (d_count) *d_count = im.count;
    if (d_uright) *d_uright = im.uright;
    if (d_depth) *d_depth = im.depth;
    if (d_quality) *d_quality = im.quality;
    if (cap) *cap = im.cap;
    return IVF_OK;
}

// one image of a held batch to the host; undistorted: its mvKeysUn instead of mvKeys (the same unless the run had a camera)
static int fetch_image(ivf_frontend* fe, int age, int pair, int side, bool undistorted, ivf_keypoint* kps, uint8_t* desc, int cap, int* n_out,
                       float* uright, float* depth, float* quality)
{
    if (!fe || !n_out || side < 0 || side > 1) return fail(IVF_E_INVALID, "bad argument");
    int k = 0, rc = held_batch(fe, age, &k);
    if (rc) return rc;
    if (pair < 0 || pair >= fe->pairsOf[k]) return fail(IVF_E_INVALID, "pair %d outside the batch of %d", pair, fe->pairsOf[k]);
    rc = ivf_frontend_sync(fe);
    if (rc) return rc;
    const BatchImage im = batch_image(fe, k, pair, side);
    int n = 0;
    HIPCHK(hipMemcpy(&n, im.count, sizeof(int), hipMemcpyDeviceToHost));
    *n_out = n;
    if (n > cap) return fail(IVF_E_CAPACITY, "%d keypoints exceed caller capacity %d", n, cap);
    if (n == 0) return IVF_OK;
    if (kps) HIPCHK(hipMemcpy(kps, undistorted ? im.kps : im.mvKeys, (size_t)n * sizeof(ivf_keypoint), hipMemcpyDeviceToHost));
    if (desc) HIPCHK(hipMemcpy(desc, im.desc, (size_t)n * 32, hipMemcpyDeviceToHost));
    if (quality) HIPCHK(hipMemcpy(quality, im.quality, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (uright && im.uright) HIPCHK(hipMemcpy(uright, im.uright, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (depth && im.depth) HIPCHK(hipMemcpy(depth, im.depth, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return IVF_OK;
}

int ivf_frontend_fetch_of(ivf_frontend* fe, int age, int pair, int side, ivf_keypoint* kps, uint8_t* desc, int cap, int* n_out,
                          float* uright, float* depth, float* quality)
{
    return fetch_image(fe, age, pair, side, false, kps, desc, cap, n_out, uright, depth, quality);
}

int ivf_frontend_fetch(ivf_frontend* fe, int pair, int side, ivf_keypoint* kps, uint8_t* desc, int cap, int* n_out,
                       float* uright, float* depth, float* quality)
{
    if (fe && fe->runs == 0) return fail(IVF_E_INVALID, "pair %d outside the last batch of 0", pair);
    return ivf_frontend_fetch_of(fe, 0, pair, side, kps, desc, cap, n_out, uright, depth, quality);
}

// Frame::UndistortKeyPoints inside the batch (Frame.cc:145, :696-726)
int ivf_frontend_set_camera(ivf_frontend* fe, const ivf_camera* cam)
{
    if (!fe) return fail(IVF_E_INVALID, "null handle");
    if (cam) { const int rc = check_camera(cam); if (rc) return rc; }
    if (!cam || !camera_undistorts(*cam)) { fe->camOn = false; return IVF_OK; }     // Frame.cc:698-702: mvKeysUn = mvKeys
    HIPCHK(hipSetDevice(fe->cfg.device_id));
    const size_t bytes = (size_t)2 * fe->cfg.max_pairs * fe->ctx[0].hc.nfeatures * sizeof(ivf_keypoint);
    for (int k = 0; k < kPipe; k++)
        if (!fe->kpsUn[k]) HIPCHK(fe->ctx[k].alloc(fe->kpsUn[k], bytes));
    fe->cam = ivf::undistort_cam(*cam);       // passed to the kernel by value: batches already enqueued keep the camera they ran with
    fe->camOn = true;
    return IVF_OK;
}

int ivf_frontend_undistorted(const ivf_frontend* fe, int age, const ivf_keypoint** d_kps_un)
{
    if (!fe || !d_kps_un) return fail(IVF_E_INVALID, "null argument");
    int k = 0;
    if (const int rc = held_batch(fe, age, &k)) return rc;
    if (!fe->unOf[k]) return fail(IVF_E_STATE, "the batch of age %d ran without an undistorting camera: mvKeysUn == mvKeys", age);
    *d_kps_un = batch_image(fe, k, 0, 0).kps;
    return IVF_OK;
}

int ivf_frontend_fetch_undistorted(ivf_frontend* fe, int age, int pair, ivf_keypoint* kps_un, int cap, int* n_out)
{
    return fetch_image(fe, age, pair, 0, true, kps_un, nullptr, cap, n_out, nullptr, nullptr, nullptr);
}

float ivf_frontend_last_fast_ms(ivf_frontend* fe)
{
    double sum = 0; int n = 0;
    if (ivf_frontend_fast_ms_stats(fe, 1, &sum, &n) != IVF_OK || n < 1) return -1.f;
    return (float)sum;
}

int ivf_frontend_fast_ms_stats(ivf_frontend* fe, int last_n, double* sum_ms, int* n_out)
{
    if (!fe || !sum_ms || !n_out) return fail(IVF_E_INVALID, "null argument");
    *sum_ms = 0; *n_out = 0;
    HIPCHK(hipSetDevice(fe->cfg.device_id));
    // run r used context r % kPipe and that context's ring slot (r / kPipe) % kEvRing
    const long long keep = kPipe * (long long)Context::kEvRing;
    const long long avail = std::min<long long>(fe->runs, keep);
    const long long take = std::min<long long>(avail, last_n < 1 ? avail : last_n);
    for (long long r = fe->runs - take; r < fe->runs; r++) {
        Context& c = fe->ctx[r % kPipe];
        const int slot = (int)((r / kPipe) % Context::kEvRing);
        HIPCHK(hipEventSynchronize(c.evFast1[slot]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c.evFast0[slot], c.evFast1[slot]));
        *sum_ms += ms; (*n_out)++;
    }
    return IVF_OK;
}

int ivf_frontend_pack_gather_block_of(ivf_frontend* fe, int age, uint8_t* d_block, size_t block_bytes, size_t* record_bytes,
                                      void* hip_stream)
{
    if (!fe || !record_bytes) return fail(IVF_E_INVALID, "null argument");
    const size_t nf = fe->ctx[0].hc.nfeatures;
    const size_t rec = 16 + nf * sizeof(ivf_keypoint) + nf * 32 + 2 * nf * sizeof(float);
    *record_bytes = rec;
    if (!d_block) return IVF_OK;
    if (age < 0 || age >= kPipe) return fail(IVF_E_INVALID, "age %d outside [0,%d): results stay valid for %d further runs", age, kPipe, kPipe - 1);
    int k = 0;
    if (const int rc = held_batch(fe, age, &k)) return rc;
    const int np = fe->pairsOf[k];
    if (block_bytes < rec * np) return fail(IVF_E_CAPACITY, "gather block needs %zu bytes", rec * np);
    if (((size_t)d_block & 15) != 0) return fail(IVF_E_INVALID, "gather block must be 16-byte aligned");
    HIPCHK(hipSetDevice(fe->cfg.device_id));
    hipStream_t st = (hipStream_t)hip_stream;
    if (hip_stream == IVF_STREAM_OF_BATCH) st = fe->stream[k];        // in order behind the batch itself: nothing to wait for
    else HIPCHK(hipStreamWaitEvent(st, fe->evDone[k], 0));            // the batch ran on an internal stream
    launch_pack_gather(fe->ctx[k].b, batch_image(fe, k, 0, 0).kps, (int)nf, np, d_block, rec, st);
    HIPCHK(hipGetLastError());
    return IVF_OK;
}

void* ivf_frontend_batch_stream(ivf_frontend* fe, int age)
{
    int k = 0;
    if (!fe || held_batch(fe, age, &k)) return nullptr;
    return (void*)fe->stream[k];
}

// A resident frame straight from a batch (the frame itself: ivf::frame_from_batch, ivf_match.hip).  `age` as in
// ivf_frontend_pack_gather_block_of; side 0 = left (with uRight), 1 = right.
int ivf_frame_create_from_frontend(ivf_frontend* fe, int age, int pair, int side, const ivf_bounds* bounds, ivf_frame** out)
{
    if (!out) return fail(IVF_E_INVALID, "null argument");
    *out = nullptr;
    if (!fe || !bounds || side < 0 || side > 1) return fail(IVF_E_INVALID, "bad argument");
    if (!(bounds->max_x > bounds->min_x) || !(bounds->max_y > bounds->min_y)) return fail(IVF_E_INVALID, "empty image bounds");
    int k = 0;
    if (const int rc = held_batch(fe, age, &k)) return rc;
    if (pair < 0 || pair >= fe->pairsOf[k]) return fail(IVF_E_INVALID, "pair %d outside the batch of %d", pair, fe->pairsOf[k]);
    HIPCHK(hipSetDevice(fe->cfg.device_id));
    return frame_from_batch(fe->cfg.device_id, batch_image(fe, k, pair, side), *bounds, out);
}

int ivf_frontend_pack_gather_block(ivf_frontend* fe, uint8_t* d_block, size_t block_bytes, size_t* record_bytes, void* hip_stream)
{
    return ivf_frontend_pack_gather_block_of(fe, 0, d_block, block_bytes, record_bytes, hip_stream);
}

}  // extern "C"
