// ivf_match.hip -- the per-call half of the C-ABI (include/ivfront.h): every ORBmatcher search, the device-resident ivf_frame, the
// DBoW2 vocabulary / BoW vectors, the distinctive descriptor and the quality-score update.
// Each search builds its candidate lists and Hamming distances on the device (CandSource, node_pairs) and then replays the
// reference's order-dependent greedy logic on the host.  Its kernels (k_hamming_pairs, k_distinct_median, k_bow_transform, k_grid_build,
// k_grid_window) are file-local, at the top; the grid they and the batched tracker (ivf_track.hip, ivf_track_local.hip) share is ivf_grid.h,
// the descent k_bow_transform and the tracker's BoW units share ivf_bow.h.
#include <cmath>
#include <climits>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>
#include <algorithm>
#include "ivf_bow.h"

using namespace ivf;

// ---- kernels of this file (hand-written for gfx950, wave = 64) ------------------------------------------------------------------
namespace {

// DescriptorDistance (ORBmatcher.cc:1700-1716) of index pairs
__global__ void k_hamming_pairs(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                const int* __restrict__ pairs, int n, int* __restrict__ dist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* pa = (const uint4*)(a + (size_t)pairs[2 * i] * 32);
    const uint4* pb = (const uint4*)(b + (size_t)pairs[2 * i + 1] * 32);
    dist[i] = hamming256(pa[0], pa[1], pb[0], pb[1]);
}
void launch_hamming_pairs(const uint8_t* a, const uint8_t* b, const int* pairs, int n, int* dist, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_hamming_pairs, dim3((n + 255) / 256), dim3(256), 0, s, a, b, pairs, n, dist);
}

// ---- MapPoint::ComputeDistinctiveDescriptors (ORB/src/MapPoint.cc:281-305): per observed descriptor the median of
// its Hamming distances to all n (the 0 of the diagonal included) = sorted row [(int)(0.5*(n-1))].  Distances live in
// 0..256, so the median is read off a 257-bin LDS histogram instead of a sort: the smallest value whose cumulative count
// exceeds the index.  One workgroup per row.
__global__ __launch_bounds__(256) void k_distinct_median(const uint8_t* __restrict__ desc, int n, int* __restrict__ median)
{
    __shared__ int hist[257 + 7];
    const int i = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < 264; k += 256) hist[k] = 0;
    __syncthreads();
    const uint4* pi = (const uint4*)(desc + (size_t)i * 32);
    const uint4 a0 = pi[0], a1 = pi[1];
    for (int j = tid; j < n; j += 256) {
        const uint4* pj = (const uint4*)(desc + (size_t)j * 32);
        const int d = j == i ? 0 : hamming256(a0, a1, pj[0], pj[1]);
        atomicAdd(&hist[d], 1);
    }
    __syncthreads();
    if (tid == 0) {
        const int target = (int)(0.5 * (n - 1));
        int acc = 0, v = 0;
        for (; v < 257; v++) { acc += hist[v]; if (acc > target) break; }
        median[i] = v;
    }
}

void launch_distinct_median(const uint8_t* desc, int n, int* median, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_distinct_median, dim3(n), dim3(256), 0, s, desc, n, median);
}

// ---- DBoW2 vocabulary-tree descent (TemplatedVocabulary.h:1217-1259): the n descriptors as one record slot of bow_descend_slot (ivf_bow.h)
__global__ __launch_bounds__(256) void k_bow_transform(const int* __restrict__ childStart, const int* __restrict__ child,
                                                      const uint8_t* __restrict__ nodeDesc, const uint8_t* __restrict__ desc,
                                                      int n, int nidLevel, int* __restrict__ leaf, int* __restrict__ nodeAt)
{
    bow_descend_slot(childStart, child, nodeDesc, desc, n, blockIdx.x, nidLevel, [&](int f, int node, int nid) { leaf[f] = node; nodeAt[f] = nid; });
}

void launch_bow_transform(const int* childStart, const int* child, const uint8_t* nodeDesc, const uint8_t* desc, int n, int nidLevel,
                          int* leaf, int* nodeAt, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bow_transform, dim3((n * 16 + 255) / 256), dim3(256), 0, s, childStart, child, nodeDesc, desc, n, nidLevel, leaf, nodeAt);
}

// ---- the device-resident frame grid: ivf_grid.h's grid_build / grid_walk with int indices (what ivf_frame_grid returns) ----
// k_grid_build: ONE workgroup builds the grid of a frame.  start: [64*48 + 1], idx: [n].
__global__ __launch_bounds__(256) void k_grid_build(const ivf_keypoint* __restrict__ kps, int n, GridGeom G, int* __restrict__ start,
                                                   int* __restrict__ idx)
{
    __shared__ int cnt[kGC * kGR];
    __shared__ int part[256];
    __shared__ int blk[256];
    grid_build<int>(G, kps, n, start, idx, cnt, part, blk, threadIdx.x);
}
void launch_grid_build(const ivf_keypoint* kps, int n, const GridGeom& G, int* start, int* idx, hipStream_t s)
{
    hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(256), 0, s, kps, n, G, start, idx);
}

// k_grid_window: one wave per query.  The candidates that pass the window's filters are appended, ordered and ballot-compacted,
// as (index, distance) to the query's list (cap entries; count may exceed cap = overflow, the host then re-does that query
// through the host grid).
__global__ __launch_bounds__(256) void k_grid_window(const ivf_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                    const int* __restrict__ start, const int* __restrict__ idx, GridGeom G, int nq,
                                                    const float* __restrict__ qu, const float* __restrict__ qv,
                                                    const float* __restrict__ qr, const int* __restrict__ qminL,
                                                    const int* __restrict__ qmaxL, const uint8_t* __restrict__ qdesc,
                                                    const uint8_t* __restrict__ qvalid, int cap, int* __restrict__ count,
                                                    int2* __restrict__ cand)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= nq) return;
    int total = 0;
    if (!qvalid || qvalid[q]) {
        const uint4* qd = (const uint4*)(qdesc + (size_t)q * 32);
        grid_walk<int>(G, kps, desc, start, idx, qu[q], qv[q], qr[q], qminL[q], qmaxL[q], qd[0], qd[1], lane, [&](bool ok, int i2, int d) {
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int pos = total + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < cap) cand[(size_t)q * cap + pos] = make_int2(i2, d);
            }
            total += __popcll(m);
        });
    }
    if (lane == 0) count[q] = total;
}
void launch_grid_window(const ivf_keypoint* kps, const uint8_t* desc, const int* start, const int* idx, const GridGeom& G, int nq,
                        const float* qu, const float* qv, const float* qr, const int* qminL, const int* qmaxL, const uint8_t* qdesc,
                        const uint8_t* qvalid, int cap, int* count, int* cand, hipStream_t s)
{
    if (nq <= 0) return;
    hipLaunchKernelGGL(k_grid_window, dim3((nq + 3) / 4), dim3(256), 0, s, kps, desc, start, idx, G, nq, qu, qv, qr, qminL, qmaxL,
                       qdesc, qvalid, cap, count, (int2*)cand);
}
}  // namespace

// ---- Frame grid on the host (ORB/src/Frame.cc:415-430, 615-680): the CPU fallback of the searches that take host arrays ----
namespace {
struct Grid {
    std::vector<int> start, idx; float invW, invH;
    void build(const ivf_keypoint* k, int n, const ivf_bounds& bd)
    {
        invW = (float)kGC / (bd.max_x - bd.min_x); invH = (float)kGR / (bd.max_y - bd.min_y);
        start.assign(kGC * kGR + 1, 0); idx.assign(std::max(n, 1), 0);
        std::vector<int> cell(std::max(n, 1), -1);
        for (int i = 0; i < n; i++) {
            const int px = (int)roundf((k[i].x - bd.min_x) * invW), py = (int)roundf((k[i].y - bd.min_y) * invH);
            if (px < 0 || px >= kGC || py < 0 || py >= kGR) continue;
            cell[i] = px * kGR + py; start[cell[i] + 1]++;
        }
        for (int c = 0; c < kGC * kGR; c++) start[c + 1] += start[c];
        std::vector<int> fill(kGC * kGR, 0);
        for (int i = 0; i < n; i++) if (cell[i] >= 0) idx[start[cell[i]] + fill[cell[i]]++] = i;
    }
    template <class F> void query(const ivf_keypoint* k, const ivf_bounds& bd, float x, float y, float r, int minL, int maxL, F f) const
    {
        const int x0 = std::max(0, (int)floorf((x - bd.min_x - r) * invW)); if (x0 >= kGC) return;
        const int x1 = std::min(kGC - 1, (int)ceilf((x - bd.min_x + r) * invW)); if (x1 < 0) return;
        const int y0 = std::max(0, (int)floorf((y - bd.min_y - r) * invH)); if (y0 >= kGR) return;
        const int y1 = std::min(kGR - 1, (int)ceilf((y - bd.min_y + r) * invH)); if (y1 < 0) return;
        const bool chk = (minL > 0) || (maxL >= 0);
        for (int ix = x0; ix <= x1; ix++)
            for (int iy = y0; iy <= y1; iy++) {
                const int c = ix * kGR + iy;
                for (int j = start[c]; j < start[c + 1]; j++) {
                    const ivf_keypoint& kp = k[idx[j]];
                    if (chk) { if (kp.octave < minL) continue; if (maxL >= 0 && kp.octave > maxL) continue; }
                    if (fabsf(kp.x - x) < r && fabsf(kp.y - y) < r) f(idx[j]);
                }
            }
    }
};

// The rotation-consistency filter of every search that takes mbCheckOrientation: matches are binned by the angle between
// the two keypoints, ComputeThreeMaxima (ORBmatcher.cc:1654-1695) keeps up to three bins and every match of the others is taken back.
struct RotHist {
    static constexpr int HISTO_LENGTH = 30;
    std::vector<int> bins[HISTO_LENGTH];
    void add(float rot, int idx)
    {
        const float factor = 1.0f / HISTO_LENGTH;
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        if (bin >= 0 && bin < HISTO_LENGTH) bins[bin].push_back(idx);
    }
    // reject(idx) once per entry of every bin that is not one of the three maxima: bin order, then insertion order; an index
    // added twice is rejected twice (SearchByProjection(cur, last) counts such a match off twice, :1444-1511)
    template <class F> void reject_outliers(F reject) const
    {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < HISTO_LENGTH; i++) {
            const int s = (int)bins[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
        for (int i = 0; i < HISTO_LENGTH; i++)
            if (i != ind1 && i != ind2 && i != ind3)
                for (int idx : bins[i]) reject(idx);
    }
};

// A DBoW2::FeatureVector in CSR form (include/ivfront.h): `who` names it in the message, with a %s where the offending part goes
int check_feature_vector(const int32_t* node, const int32_t* start, const int32_t* idx, int nodes, int n, const char* who)
{
    char what[64];
    for (int a = 0; a + 1 < nodes; a++)
        if (node[a] >= node[a + 1]) { snprintf(what, sizeof what, who, "node ids"); return fail(IVF_E_INVALID, "%s must ascend", what); }
    for (int p = start[0]; p < start[nodes]; p++)
        if (idx[p] < 0 || idx[p] >= n) { snprintf(what, sizeof what, who, "feature index"); return fail(IVF_E_INVALID, "%s out of range", what); }
    return IVF_OK;
}

// The node merge of the BoW-guided searches (ORBmatcher.cc:187-265, :697-731): a two-pointer walk over two feature
// vectors whose nodes ascend.  Every eligible feature i1 of a shared node gets one run of (i1, i2) pairs, i2 over the eligible
// features of that node on side 2 in feature-vector order, and dist[] their Hamming distances from the device.
struct Run { int i1, first, len; };                         // pairs / dist [first, first + len)
struct AnyFeature { bool operator()(int) const { return true; } };
template <class E1, class E2 = AnyFeature>
int node_pairs(const uint8_t* desc1, int n1, const int32_t* node1, const int32_t* start1, const int32_t* idx1, int nodes1,
               const uint8_t* desc2, int n2, const int32_t* node2, const int32_t* start2, const int32_t* idx2, int nodes2,
               int device_id, std::vector<Run>& runs, std::vector<int>& pairs, std::vector<int>& dist, E1 eligible1, E2 eligible2 = E2())
{
    int a = 0, b = 0;
    while (a < nodes1 && b < nodes2) {
        if (node1[a] == node2[b]) {
            for (int p = start1[a]; p < start1[a + 1]; p++) {
                const int i1 = idx1[p];
                if (!eligible1(i1)) continue;
                Run r{i1, (int)pairs.size() / 2, 0};
                for (int q = start2[b]; q < start2[b + 1]; q++) {
                    const int i2 = idx2[q];
                    if (!eligible2(i2)) continue;
                    pairs.push_back(i1); pairs.push_back(i2); r.len++;
                }
                runs.push_back(r);
            }
            a++; b++;
        } else if (node1[a] < node2[b]) { while (a < nodes1 && node1[a] < node2[b]) a++; }
        else { while (b < nodes2 && node2[b] < node1[a]) b++; }
    }
    const int nPairs = (int)pairs.size() / 2;
    dist.assign(std::max(nPairs, 1), 0);
    return ivf_hamming_pairs(desc1, n1, desc2, n2, pairs.data(), nPairs, dist.data(), device_id);
}
}  // namespace

extern "C" {

int ivf_hamming(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

int ivf_hamming_pairs(const uint8_t* desc_a, int n_a, const uint8_t* desc_b, int n_b,
                      const int32_t* pairs, int n_pairs, int32_t* dist, int device_id)
{
    if (n_pairs == 0) return IVF_OK;
    if (!desc_a || !desc_b || !pairs || !dist || n_a < 1 || n_b < 1 || n_pairs < 0) return fail(IVF_E_INVALID, "bad argument");
    for (int i = 0; i < n_pairs; i++)
        if (pairs[2 * i] < 0 || pairs[2 * i] >= n_a || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= n_b)
            return fail(IVF_E_INVALID, "pair %d indexes outside the descriptor arrays", i);
    int rc = have_device(device_id);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device_id));
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t szA = up((size_t)n_a * 32), szB = up((size_t)n_b * 32), szP = up((size_t)n_pairs * 2 * sizeof(int)),
                 szD = up((size_t)n_pairs * sizeof(int));
    uint8_t* scb = nullptr;
    rc = thread_scratch(device_id, szA + szB + szP + szD, &scb);
    if (rc) return rc;
    uint8_t* dA = scb; uint8_t* dB = dA + szA; int* dP = (int*)(dB + szB); int* dD = (int*)((uint8_t*)dP + szP);
    HIPCHK(hipMemcpyAsync(dA, desc_a, (size_t)n_a * 32, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(dB, desc_b, (size_t)n_b * 32, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(dP, pairs, (size_t)n_pairs * 2 * sizeof(int), hipMemcpyHostToDevice, nullptr));
    launch_hamming_pairs(dA, dB, dP, n_pairs, dD, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(dist, dD, (size_t)n_pairs * sizeof(int), hipMemcpyDeviceToHost));
    return IVF_OK;
}

int ivf_features_in_area(const ivf_keypoint* kps, int n, const ivf_bounds* bounds, float x, float y, float r,
                         int min_level, int max_level, int32_t* out, int cap, int* n_out)
{
    if (!kps || !bounds || !n_out || n < 0) return fail(IVF_E_INVALID, "bad argument");
    Grid g; g.build(kps, n, *bounds);
    int c = 0;
    g.query(kps, *bounds, x, y, r, min_level, max_level, [&](int i) { if (out && c < cap) out[c] = i; c++; });
    *n_out = c;
    return c > cap ? fail(IVF_E_CAPACITY, "%d indices exceed capacity %d", c, cap) : IVF_OK;
}

// order-dependent greedy assignment + rotation histogram of SearchByProjection(cur, last), replayed in query order
// (ORBmatcher.cc:1444-1511): candidates of query i = cand[qStart[i] .. qStart[i+1]) in GetFeaturesInArea order
static int replay_projection(const ivf_keypoint* cur_kps, const float* cur_uright, int n_q, const float* q_ur, const float* q_radius,
                             const float* q_angle, const uint8_t* q_blocks, int check_orientation, const std::vector<int>& qStart,
                             const std::vector<int>& cand, const std::vector<int>& dist, int32_t* cur_assign, uint8_t* removed = nullptr)
{
    RotHist rotHist;
    int nm = 0;
    for (int i = 0; i < n_q; i++) {
        int bestDist = 256, bestIdx2 = -1;
        for (int p = qStart[i]; p < qStart[i + 1]; p++) {
            const int i2 = cand[p];
            if (cur_assign[i2] == -2) continue;
            if (cur_assign[i2] >= 0 && (!q_blocks || q_blocks[cur_assign[i2]])) continue;
            if (cur_uright[i2] > 0) { const float er = fabsf(q_ur[i] - cur_uright[i2]); if (er > q_radius[i]) continue; }
            if (dist[p] < bestDist) { bestDist = dist[p]; bestIdx2 = i2; }
        }
        if (bestIdx2 >= 0 && bestDist <= 100) {
            cur_assign[bestIdx2] = i; nm++;                       // a non-blocking earlier match is overwritten: its index stays in the histogram
            if (check_orientation) rotHist.add(q_angle[i] - cur_kps[bestIdx2].angle, bestIdx2);
        }
    }
    if (check_orientation) rotHist.reject_outliers([&](int j) { cur_assign[j] = -1; nm--; if (removed) removed[j] = 1; });
    return nm;
}

// best / second best + ratio test of SearchByProjection(F, mapPoints), greedy in map-point order (ORBmatcher.cc:86-126):
// candidates of map point i = cand[qStart[i] .. qStart[i+1]) in GetFeaturesInArea order
static int replay_map_points(const ivf_keypoint* cur_kps, const float* cur_uright, int n_q, const float* q_ur, const float* q_radius,
                             const uint8_t* q_blocks, float nn_ratio, const std::vector<int>& qStart, const std::vector<int>& cand,
                             const std::vector<int>& dist, int32_t* cur_assign)
{
    int nm = 0;
    for (int i = 0; i < n_q; i++) {
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (int p = qStart[i]; p < qStart[i + 1]; p++) {
            const int idx = cand[p];
            if (cur_assign[idx] == -2) continue;
            if (cur_assign[idx] >= 0 && (!q_blocks || q_blocks[cur_assign[idx]])) continue;
            if (cur_uright[idx] > 0) { const float er = fabsf(q_ur[i] - cur_uright[idx]); if (er > q_radius[i]) continue; }
            const int d = dist[p];
            if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestLevel2 = bestLevel; bestLevel = cur_kps[idx].octave; bestIdx = idx; }
            else if (d < bestDist2) { bestLevel2 = cur_kps[idx].octave; bestDist2 = d; }
        }
        if (bestIdx >= 0 && bestDist <= 100) {
            if (bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2) continue;
            cur_assign[bestIdx] = i; nm++;
        }
    }
    return nm;
}

// ---- device-resident frame: keypoints, descriptors and the 64x48 grid stay in HBM between searches -----------------
// A frame's device memory is ONE arena (keypoints | descriptors | uRight | grid start | grid index) with a stream of its own,
// and its query scratch a second one; both come from a per-process pool and go back to it in ivf_frame_destroy, so a tracker
// that makes a frame per image pays hipMalloc / hipStreamCreate only until the pool is warm (r02: five hipMalloc + a stream
// per frame = 0.5 ms).
namespace {
struct Arena { int device = -1; uint8_t* base = nullptr; size_t cap = 0; hipStream_t stream = nullptr; };
struct ArenaPool {
    std::mutex m; std::vector<Arena> idle;
    int acquire(int device, size_t need, Arena& out)
    {
        {
            std::lock_guard<std::mutex> g(m);
            int best = -1;
            for (int i = 0; i < (int)idle.size(); i++)
                if (idle[i].device == device && idle[i].cap >= need && (best < 0 || idle[i].cap < idle[best].cap)) best = i;
            if (best >= 0) { out = idle[best]; idle.erase(idle.begin() + best); return IVF_OK; }
        }
        Arena a; a.device = device;
        a.cap = ((need + need / 4) + 65535) & ~(size_t)65535;         // slack: frames of slightly different sizes share arenas
        if (hipMalloc(&a.base, a.cap) != hipSuccess) return fail(IVF_E_NO_DEVICE, "hipMalloc of a %zu-byte frame arena failed", a.cap);
        if (hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking) != hipSuccess) { (void)hipFree(a.base); return fail(IVF_E_NO_DEVICE, "stream creation failed"); }
        out = a;
        return IVF_OK;
    }
    void release(Arena& a)
    {
        if (!a.base) return;
        (void)hipStreamSynchronize(a.stream);                         // nothing of the old owner may still be in flight
        {
            std::lock_guard<std::mutex> g(m);
            if (idle.size() < 64) { idle.push_back(a); a = Arena(); return; }
        }
        (void)hipFree(a.base); (void)hipStreamDestroy(a.stream);
        a = Arena();
    }
};
ArenaPool* frame_pool_ptr() { static ArenaPool* p = new ArenaPool(); return p; }   // never destroyed: no HIP calls during static destruction
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

struct ivf_frame {
    int device = 0, n = 0;
    ivf_bounds bd{};
    GridGeom geom{};                    // of bd (Frame.cc:208-209)
    std::vector<ivf_keypoint> kps;      // host copies for the greedy replay (angle, uRight)
    std::vector<float> uright;
    std::vector<uint8_t> desc;          // host copy for the overflow fallback
    Arena mem, qmem;                    // frame data / query scratch (pooled)
    ivf_keypoint* dKps = nullptr; uint8_t* dDesc = nullptr; int *dStart = nullptr, *dIdx = nullptr;
    // query scratch, grown on demand
    int qCap = 0, cCap = 0;
    float *dQu = nullptr, *dQv = nullptr, *dQr = nullptr; int *dQmin = nullptr, *dQmax = nullptr; uint8_t *dQdesc = nullptr, *dQvalid = nullptr;
    int *dCount = nullptr, *dCand = nullptr;
    hipStream_t stream = nullptr;
    float* dUright = nullptr;           // frames made from a front-end batch: uRight stays on the device until a replay needs it
    bool hostKps = true, hostDesc = true;   // host mirrors present (false: fetched on first use, see frame_host)
};

// carve the frame arena for n keypoints
static int frame_alloc(ivf_frame* f, int n)
{
    const size_t nn = (size_t)std::max(n, 1);
    const size_t oK = 0, oD = oK + up256(nn * sizeof(ivf_keypoint)), oU = oD + up256(nn * 32), oS = oU + up256(nn * sizeof(float)),
                 oI = oS + up256((kGC * kGR + 1) * sizeof(int)), total = oI + up256(nn * sizeof(int));
    const int rc = frame_pool_ptr()->acquire(f->device, total, f->mem);
    if (rc) return rc;
    uint8_t* b = f->mem.base;
    f->dKps = (ivf_keypoint*)(b + oK); f->dDesc = b + oD; f->dUright = (float*)(b + oU); f->dStart = (int*)(b + oS); f->dIdx = (int*)(b + oI);
    f->stream = f->mem.stream;
    return IVF_OK;
}

// the greedy replays read angle / octave / uRight of the frame's keypoints on the host, the overflow fallback its descriptors:
// frames created from host arrays carry them; frames created from a front-end batch fetch them on first use (28 B per keypoint)
static int frame_host(ivf_frame* f, bool needDesc)
{
    if (!f->hostKps) {
        HIPCHK(hipSetDevice(f->device));
        f->kps.resize(std::max(f->n, 1)); f->uright.resize(std::max(f->n, 1));
        if (f->n > 0) {
            HIPCHK(hipMemcpyAsync(f->kps.data(), f->dKps, (size_t)f->n * sizeof(ivf_keypoint), hipMemcpyDeviceToHost, f->stream));
            HIPCHK(hipMemcpyAsync(f->uright.data(), f->dUright, (size_t)f->n * sizeof(float), hipMemcpyDeviceToHost, f->stream));
            HIPCHK(hipStreamSynchronize(f->stream));
        }
        f->hostKps = true;
    }
    if (needDesc && !f->hostDesc) {
        HIPCHK(hipSetDevice(f->device));
        f->desc.resize((size_t)std::max(f->n, 1) * 32);
        if (f->n > 0) HIPCHK(hipMemcpy(f->desc.data(), f->dDesc, (size_t)f->n * 32, hipMemcpyDeviceToHost));
        f->hostDesc = true;
    }
    return IVF_OK;
}

void ivf_frame_destroy(ivf_frame* f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    frame_pool_ptr()->release(f->mem);
    frame_pool_ptr()->release(f->qmem);
    delete f;
}

int ivf_frame_count(const ivf_frame* f)
{
    return f ? f->n : fail(IVF_E_INVALID, "null handle");
}

int ivf_frame_create(const ivf_keypoint* kps, const uint8_t* desc, const float* uright, int n, const ivf_bounds* bounds,
                     int device_id, ivf_frame** out)
{
    if (!out) return fail(IVF_E_INVALID, "null argument");
    *out = nullptr;
    if (!bounds || n < 0 || (n > 0 && (!kps || !desc || !uright))) return fail(IVF_E_INVALID, "bad argument");
    if (!(bounds->max_x > bounds->min_x) || !(bounds->max_y > bounds->min_y)) return fail(IVF_E_INVALID, "empty image bounds");
    int rc = have_device(device_id);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device_id));
    ivf_frame* f = new ivf_frame();
    f->device = device_id; f->n = n; f->bd = *bounds;
    f->geom = grid_geom(*bounds);
    f->kps.assign(kps, kps + n); f->uright.assign(uright, uright + n); f->desc.assign(desc, desc + (size_t)n * 32);
    rc = frame_alloc(f, n);
    if (rc) { ivf_frame_destroy(f); return rc; }
    if (n > 0) {
        if (hipMemcpyAsync(f->dKps, kps, (size_t)n * sizeof(ivf_keypoint), hipMemcpyHostToDevice, f->stream) != hipSuccess ||
            hipMemcpyAsync(f->dDesc, desc, (size_t)n * 32, hipMemcpyHostToDevice, f->stream) != hipSuccess) {
            ivf_frame_destroy(f);
            return fail(IVF_E_NO_DEVICE, "frame upload failed");
        }
    }
    launch_grid_build(f->dKps, n, f->geom, f->dStart, f->dIdx, f->stream);   // AssignFeaturesToGrid
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(f->stream) != hipSuccess) {
        ivf_frame_destroy(f);
        return fail(IVF_E_NO_DEVICE, "grid build failed");
    }
    *out = f;
    return IVF_OK;
}

int ivf_frame_grid(const ivf_frame* f, int32_t* cell_start, int32_t* cell_index)
{
    if (!f || !cell_start || !cell_index) return fail(IVF_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipMemcpy(cell_start, f->dStart, (kGC * kGR + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (f->n > 0) HIPCHK(hipMemcpy(cell_index, f->dIdx, (size_t)f->n * sizeof(int), hipMemcpyDeviceToHost));
    return IVF_OK;
}

// windows (GetFeaturesInArea) and distances (DescriptorDistance) of every query against the resident frame, on the device:
// candidates of query i = cand / dist [qStart[i] .. qStart[i+1]) in the reference's order
static int frame_candidates(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_radius,
                            const int32_t* q_min_level, const int32_t* q_max_level, const uint8_t* q_desc, const uint8_t* q_valid,
                            std::vector<int>& qStart, std::vector<int>& cand, std::vector<int>& dist)
{
    HIPCHK(hipSetDevice(f->device));
    static const int capEnv = getenv("IVF_FRAME_WINDOW_CAP") ? atoi(getenv("IVF_FRAME_WINDOW_CAP")) : 0;   // tests: force the overflow path
    const int cap = capEnv > 0 ? capEnv : 128;
    if (n_q > f->qCap || cap > f->cCap) {
        frame_pool_ptr()->release(f->qmem);
        f->qCap = 0;
        const size_t nq = (size_t)n_q + 256;
        const size_t o1 = up256(nq * 4), oDesc = 5 * o1, oValid = oDesc + up256(nq * 32), oCount = oValid + up256(nq), oCand = oCount + o1,
                     total = oCand + up256(nq * cap * 8);
        const int prc = frame_pool_ptr()->acquire(f->device, total, f->qmem);
        if (prc) return prc;
        uint8_t* b = f->qmem.base;
        f->dQu = (float*)b; f->dQv = (float*)(b + o1); f->dQr = (float*)(b + 2 * o1); f->dQmin = (int*)(b + 3 * o1); f->dQmax = (int*)(b + 4 * o1);
        f->dQdesc = b + oDesc; f->dQvalid = b + oValid; f->dCount = (int*)(b + oCount); f->dCand = (int*)(b + oCand);
        f->qCap = (int)nq; f->cCap = cap;
    }
    hipStream_t st = f->stream;
    const size_t nq = (size_t)n_q;
    HIPCHK(hipMemcpyAsync(f->dQu, q_u, nq * 4, hipMemcpyHostToDevice, st)); HIPCHK(hipMemcpyAsync(f->dQv, q_v, nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(f->dQr, q_radius, nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(f->dQmin, q_min_level, nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(f->dQmax, q_max_level, nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(f->dQdesc, q_desc, nq * 32, hipMemcpyHostToDevice, st));
    if (q_valid) HIPCHK(hipMemcpyAsync(f->dQvalid, q_valid, nq, hipMemcpyHostToDevice, st));
    launch_grid_window(f->dKps, f->dDesc, f->dStart, f->dIdx, f->geom, n_q, f->dQu, f->dQv, f->dQr, f->dQmin,
                       f->dQmax, f->dQdesc, q_valid ? f->dQvalid : nullptr, f->cCap, f->dCount, f->dCand, st);
    HIPCHK(hipGetLastError());
    std::vector<int> count(n_q), raw(nq * f->cCap * 2);
    HIPCHK(hipMemcpyAsync(count.data(), f->dCount, nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(raw.data(), f->dCand, nq * f->cCap * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    qStart.assign(n_q + 1, 0); cand.clear(); dist.clear();
    Grid g; bool haveGrid = false;
    for (int i = 0; i < n_q; i++) {
        qStart[i] = (int)cand.size();
        if (count[i] <= f->cCap) {
            for (int k = 0; k < count[i]; k++) { cand.push_back(raw[((size_t)i * f->cCap + k) * 2]); dist.push_back(raw[((size_t)i * f->cCap + k) * 2 + 1]); }
        } else {
            // a window with more candidates than the device list holds: this query again through the host grid
            if (!haveGrid) { const int hrc = frame_host(f, true); if (hrc) return hrc; g.build(f->kps.data(), f->n, f->bd); haveGrid = true; }
            g.query(f->kps.data(), f->bd, q_u[i], q_v[i], q_radius[i], q_min_level[i], q_max_level[i], [&](int i2) {
                cand.push_back(i2); dist.push_back(ivf_hamming(q_desc + (size_t)i * 32, f->desc.data() + (size_t)i2 * 32)); });
        }
    }
    qStart[n_q] = (int)cand.size();
    if (cand.empty()) { cand.push_back(0); dist.push_back(0); }
    return IVF_OK;
}

// Where the window candidates of a set of queries (Frame / KeyFrame::GetFeaturesInArea order, octave range applied) and their
// Hamming distances come from: a frame handed over as host arrays (host grid + k_hamming_pairs), or a device-resident
// ivf_frame (k_grid_window: windows AND distances on the device, nothing but the queries is uploaded).
namespace {
struct CandSource {
    const ivf_keypoint* kps = nullptr; const uint8_t* desc = nullptr; const float* uright = nullptr; int n = 0;
    const ivf_bounds* bd = nullptr; int device = 0; ivf_frame* frame = nullptr;
    static CandSource host(const ivf_keypoint* k, const uint8_t* d, const float* ur, int n, const ivf_bounds* b, int dev)
    { CandSource s; s.kps = k; s.desc = d; s.uright = ur; s.n = n; s.bd = b; s.device = dev; return s; }
    static int resident(ivf_frame* f, CandSource& s)
    {
        const int rc = frame_host(f, false); if (rc) return rc;
        s.kps = f->kps.data(); s.uright = f->uright.data(); s.n = f->n; s.bd = &f->bd; s.device = f->device; s.frame = f;
        return IVF_OK;
    }
    // candidates of query i = cand / dist [qStart[i] .. qStart[i+1]); lo / hi = GetFeaturesInArea's minLevel / maxLevel per query
    int get(int n_q, const float* q_u, const float* q_v, const float* q_radius, const int32_t* lo, const int32_t* hi,
            const uint8_t* q_desc, const uint8_t* q_valid, std::vector<int>& qStart, std::vector<int>& cand, std::vector<int>& dist) const
    {
        if (frame) return frame_candidates(frame, n_q, q_u, q_v, q_radius, lo, hi, q_desc, q_valid, qStart, cand, dist);
        Grid g; g.build(kps, n, *bd);
        std::vector<int> pairs;
        qStart.assign(n_q + 1, 0);
        for (int i = 0; i < n_q; i++) {
            qStart[i] = (int)pairs.size() / 2;
            if (q_valid && !q_valid[i]) continue;
            g.query(kps, *bd, q_u[i], q_v[i], q_radius[i], lo[i], hi[i], [&](int i2) { pairs.push_back(i); pairs.push_back(i2); });
        }
        qStart[n_q] = (int)pairs.size() / 2;
        const int nPairs = qStart[n_q];
        dist.assign(std::max(nPairs, 1), 0); cand.assign(std::max(nPairs, 1), 0);
        const int rc = ivf_hamming_pairs(q_desc, n_q, desc, n, pairs.data(), nPairs, dist.data(), device);
        if (rc) return rc;
        for (int p = 0; p < nPairs; p++) cand[p] = pairs[2 * p + 1];
        return IVF_OK;
    }
};
inline void level_window(int n_q, const int32_t* q_level, int below, int above, std::vector<int32_t>& lo, std::vector<int32_t>& hi)
{
    lo.resize(std::max(n_q, 1)); hi.resize(std::max(n_q, 1));
    for (int i = 0; i < n_q; i++) { lo[i] = q_level[i] - below; hi[i] = q_level[i] + above; }
}
}  // namespace

// ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) matching core (ORB/src/ORBmatcher.cc:1429-1511)
static int projection_impl(const CandSource& S, int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                           const int32_t* q_min_level, const int32_t* q_max_level, const float* q_angle, const uint8_t* q_desc,
                           const uint8_t* q_valid, const uint8_t* q_blocks, int check_orientation, int32_t* cur_assign,
                           uint8_t* cur_removed, int* nmatches)
{
    *nmatches = 0;
    if (n_q == 0 || S.n == 0) return IVF_OK;
    if (!q_u || !q_v || !q_ur || !q_radius || !q_min_level || !q_max_level || !q_angle || !q_desc)
        return fail(IVF_E_INVALID, "null query array");
    // 1. + 2. candidate windows in the reference's GetFeaturesInArea order (:1429-1437), their distances (:1459-1461)
    std::vector<int> qStart, cand, dist;
    const int rc = S.get(n_q, q_u, q_v, q_radius, q_min_level, q_max_level, q_desc, q_valid, qStart, cand, dist);
    if (rc) return rc;
    // 3. order-dependent greedy assignment + rotation histogram, replayed in query order (:1444-1511)
    *nmatches = replay_projection(S.kps, S.uright, n_q, q_ur, q_radius, q_angle, q_blocks, check_orientation, qStart, cand, dist, cur_assign,
                                  cur_removed);
    return IVF_OK;
}
int ivf_search_by_projection(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, const float* cur_uright, int n_cur,
                             const ivf_bounds* bounds, int n_q, const float* q_u, const float* q_v, const float* q_ur,
                             const float* q_radius, const int32_t* q_min_level, const int32_t* q_max_level,
                             const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid, const uint8_t* q_blocks,
                             int check_orientation, int32_t* cur_assign, int* nmatches, int device_id)
{
    return ivf_search_by_projection_ex(cur_kps, cur_desc, cur_uright, n_cur, bounds, n_q, q_u, q_v, q_ur, q_radius, q_min_level,
                                       q_max_level, q_angle, q_desc, q_valid, q_blocks, check_orientation, cur_assign, nullptr,
                                       nmatches, device_id);
}
int ivf_search_by_projection_ex(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, const float* cur_uright, int n_cur,
                                const ivf_bounds* bounds, int n_q, const float* q_u, const float* q_v, const float* q_ur,
                                const float* q_radius, const int32_t* q_min_level, const int32_t* q_max_level,
                                const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid, const uint8_t* q_blocks,
                                int check_orientation, int32_t* cur_assign, uint8_t* cur_removed, int* nmatches, int device_id)
{
    if (cur_removed && n_cur > 0) memset(cur_removed, 0, (size_t)n_cur);
    if (!cur_kps || !cur_desc || !cur_uright || !bounds || !cur_assign || !nmatches || n_cur < 0 || n_q < 0)
        return fail(IVF_E_INVALID, "bad argument");
    return projection_impl(CandSource::host(cur_kps, cur_desc, cur_uright, n_cur, bounds, device_id), n_q, q_u, q_v, q_ur, q_radius,
                           q_min_level, q_max_level, q_angle, q_desc, q_valid, q_blocks, check_orientation, cur_assign, cur_removed, nmatches);
}
int ivf_frame_search_by_projection(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_ur,
                                   const float* q_radius, const int32_t* q_min_level, const int32_t* q_max_level,
                                   const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid, const uint8_t* q_blocks,
                                   int check_orientation, int32_t* cur_assign, int* nmatches)
{
    if (!f || !cur_assign || !nmatches || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    CandSource S; const int rc = CandSource::resident(f, S); if (rc) return rc;
    return projection_impl(S, n_q, q_u, q_v, q_ur, q_radius, q_min_level, q_max_level, q_angle, q_desc, q_valid, q_blocks,
                           check_orientation, cur_assign, nullptr, nmatches);
}

// ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th) (ORB/src/ORBmatcher.cc:45-135)
static int map_points_impl(const CandSource& S, int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                           const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid, const uint8_t* q_blocks,
                           float nn_ratio, int32_t* cur_assign, int* nmatches)
{
    *nmatches = 0;
    if (n_q == 0 || S.n == 0) return IVF_OK;
    if (!q_u || !q_v || !q_ur || !q_radius || !q_level || !q_desc) return fail(IVF_E_INVALID, "null query array");
    // 1. + 2. candidate windows in GetFeaturesInArea order, levels [pred - 1, pred] (:72-73), their distances
    std::vector<int32_t> lo, hi; level_window(n_q, q_level, 1, 0, lo, hi);
    std::vector<int> qStart, cand, dist;
    const int rc = S.get(n_q, q_u, q_v, q_radius, lo.data(), hi.data(), q_desc, q_valid, qStart, cand, dist);
    if (rc) return rc;
    // 3. best / second best + ratio test, greedy in map-point order (:86-126)
    *nmatches = replay_map_points(S.kps, S.uright, n_q, q_ur, q_radius, q_blocks, nn_ratio, qStart, cand, dist, cur_assign);
    return IVF_OK;
}
int ivf_search_map_points(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, const float* cur_uright, int n_cur,
                          const ivf_bounds* bounds, int n_q, const float* q_u, const float* q_v, const float* q_ur,
                          const float* q_radius, const int32_t* q_level, const uint8_t* q_desc,
                          const uint8_t* q_valid, const uint8_t* q_blocks, float nn_ratio,
                          int32_t* cur_assign, int* nmatches, int device_id)
{
    if (!cur_kps || !cur_desc || !cur_uright || !bounds || !cur_assign || !nmatches || n_cur < 0 || n_q < 0)
        return fail(IVF_E_INVALID, "bad argument");
    return map_points_impl(CandSource::host(cur_kps, cur_desc, cur_uright, n_cur, bounds, device_id), n_q, q_u, q_v, q_ur, q_radius, q_level,
                           q_desc, q_valid, q_blocks, nn_ratio, cur_assign, nmatches);
}
int ivf_frame_search_map_points(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                                const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid, const uint8_t* q_blocks,
                                float nn_ratio, int32_t* cur_assign, int* nmatches)
{
    if (!f || !cur_assign || !nmatches || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    CandSource S; const int rc = CandSource::resident(f, S); if (rc) return rc;
    return map_points_impl(S, n_q, q_u, q_v, q_ur, q_radius, q_level, q_desc, q_valid, q_blocks, nn_ratio, cur_assign, nmatches);
}

// ORBmatcher::SearchForInitialization (ORB/src/ORBmatcher.cc:410-519)
int ivf_search_for_initialization(const ivf_keypoint* kps1, const uint8_t* desc1, int n1,
                                  const ivf_keypoint* kps2, const uint8_t* desc2, int n2, const ivf_bounds* bounds2,
                                  float* prev_matched_xy, int window_size, float nn_ratio, int check_orientation,
                                  int32_t* matches12, int* nmatches, int device_id)
{
    if (!kps1 || !desc1 || !kps2 || !desc2 || !bounds2 || !prev_matched_xy || !matches12 || !nmatches || n1 < 0 || n2 < 0)
        return fail(IVF_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return IVF_OK;
    // 1. + 2. windows of the octave-0 keypoints of F1 in F2's grid, GetFeaturesInArea order (:426-430), their distances (:445)
    std::vector<float> u(n1), v(n1), radius(n1, (float)window_size);
    std::vector<int32_t> level(n1); std::vector<uint8_t> valid(n1);
    for (int i1 = 0; i1 < n1; i1++) {
        u[i1] = prev_matched_xy[2 * i1]; v[i1] = prev_matched_xy[2 * i1 + 1];
        level[i1] = kps1[i1].octave; valid[i1] = level[i1] <= 0;
    }
    std::vector<int> qStart, cand, dist;
    const int rc = CandSource::host(kps2, desc2, nullptr, n2, bounds2, device_id)
                       .get(n1, u.data(), v.data(), radius.data(), level.data(), level.data(), desc1, valid.data(), qStart, cand, dist);
    if (rc) return rc;
    // 3. order-dependent replay: best / second best against the distances already claimed, stealing, histogram (:437-510)
    const int TH_LOW = 50;
    RotHist rotHist;
    std::vector<int> matchedDist(n2, INT_MAX), matches21(n2, -1);
    int nm = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        if (qStart[i1] == qStart[i1 + 1]) continue;
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (int p = qStart[i1]; p < qStart[i1 + 1]; p++) {
            const int i2 = cand[p], d = dist[p];
            if (matchedDist[i2] <= d) continue;
            if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestIdx2 = i2; }
            else if (d < bestDist2) bestDist2 = d;
        }
        if (bestDist <= TH_LOW && (float)bestDist < (float)bestDist2 * nn_ratio) {
            if (matches21[bestIdx2] >= 0) { matches12[matches21[bestIdx2]] = -1; nm--; }
            matches12[i1] = bestIdx2; matches21[bestIdx2] = i1; matchedDist[bestIdx2] = bestDist; nm++;
            if (check_orientation) rotHist.add(kps1[i1].angle - kps2[bestIdx2].angle, i1);
        }
    }
    // a match that was stolen above has been taken back already
    if (check_orientation) rotHist.reject_outliers([&](int idx1) { if (matches12[idx1] >= 0) { matches12[idx1] = -1; nm--; } });
    for (int i1 = 0; i1 < n1; i1++)
        if (matches12[i1] >= 0) { prev_matched_xy[2 * i1] = kps2[matches12[i1]].x; prev_matched_xy[2 * i1 + 1] = kps2[matches12[i1]].y; }
    *nmatches = nm;
    return IVF_OK;
}

// ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (ORB/src/ORBmatcher.cc:296-404), flat queries
static int keyframe_points_impl(const CandSource& S, int n_q, const float* q_u, const float* q_v, const float* q_radius,
                                const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid, int32_t* matched, int* nmatches)
{
    *nmatches = 0;
    if (n_q == 0 || S.n == 0) return IVF_OK;
    if (!q_u || !q_v || !q_radius || !q_level || !q_desc) return fail(IVF_E_INVALID, "null query array");
    // 1. + 2. windows (KeyFrame::GetFeaturesInArea, no level arguments) filtered by octave in [level-1, level] (:384-385), distances
    std::vector<int32_t> lo, hi; level_window(n_q, q_level, 1, 0, lo, hi);
    std::vector<int> qStart, cand, dist;
    const int rc = S.get(n_q, q_u, q_v, q_radius, lo.data(), hi.data(), q_desc, q_valid, qStart, cand, dist);
    if (rc) return rc;
    // 3. greedy replay in candidate order: occupied keypoints are skipped (:379-380)
    int nm = 0;
    for (int i = 0; i < n_q; i++) {
        int bestDist = 256, bestIdx = -1;
        for (int p = qStart[i]; p < qStart[i + 1]; p++) {
            const int idx = cand[p];
            if (matched[idx] != -1) continue;
            if (dist[p] < bestDist) { bestDist = dist[p]; bestIdx = idx; }
        }
        if (bestDist <= 50) { matched[bestIdx] = i; nm++; }
    }
    *nmatches = nm;
    return IVF_OK;
}
int ivf_search_keyframe_points(const ivf_keypoint* kf_kps, const uint8_t* kf_desc, int n_kf, const ivf_bounds* bounds,
                               int n_q, const float* q_u, const float* q_v, const float* q_radius, const int32_t* q_level,
                               const uint8_t* q_desc, const uint8_t* q_valid, int32_t* matched, int* nmatches, int device_id)
{
    if (!kf_kps || !kf_desc || !bounds || !matched || !nmatches || n_kf < 0 || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    return keyframe_points_impl(CandSource::host(kf_kps, kf_desc, nullptr, n_kf, bounds, device_id), n_q, q_u, q_v, q_radius, q_level,
                                q_desc, q_valid, matched, nmatches);
}
int ivf_frame_search_keyframe_points(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_radius,
                                     const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid, int32_t* matched, int* nmatches)
{
    if (!f || !matched || !nmatches || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    CandSource S; const int rc = CandSource::resident(f, S); if (rc) return rc;
    return keyframe_points_impl(S, n_q, q_u, q_v, q_radius, q_level, q_desc, q_valid, matched, nmatches);
}

// ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th) matching core (ORB/src/ORBmatcher.cc:893-955), flat queries
static int fuse_impl(const CandSource& S, const float* inv_level_sigma2, int n_levels, int n_q, const float* q_u, const float* q_v,
                     const float* q_ur, const float* q_radius, const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid,
                     int32_t* best_idx, int32_t* best_dist)
{
    const bool gate = inv_level_sigma2 != nullptr;               // NULL: Fuse(KF, Scw, ...) (:983-1106) has no chi-square gate
    if (gate && (!S.uright || !q_ur || n_levels < 1)) return fail(IVF_E_INVALID, "the chi-square gate needs mvuRight, ur and the sigma table");
    for (int i = 0; i < n_q; i++) { best_idx[i] = -1; if (best_dist) best_dist[i] = 256; }
    if (n_q == 0 || S.n == 0) return IVF_OK;
    if (!q_u || !q_v || !q_radius || !q_level || !q_desc) return fail(IVF_E_INVALID, "null query array");
    if (gate)
        for (int i = 0; i < S.n; i++)
            if (S.kps[i].octave < 0 || S.kps[i].octave >= n_levels) return fail(IVF_E_INVALID, "keypoint %d: octave outside the sigma table", i);
    std::vector<int32_t> lo, hi; level_window(n_q, q_level, 1, 0, lo, hi);      // octave in [level-1, level] (:913-914)
    std::vector<int> qStart, cand, dist;
    const int rc = S.get(n_q, q_u, q_v, q_radius, lo.data(), hi.data(), q_desc, q_valid, qStart, cand, dist);
    if (rc) return rc;
    for (int i = 0; i < n_q; i++) {
        const float u = q_u[i], v = q_v[i], ur = q_ur ? q_ur[i] : 0.0f;
        int bestDist = 256, bestIdx = -1;
        for (int p = qStart[i]; p < qStart[i + 1]; p++) {
            const int idx = cand[p];
            if (gate) {                                              // chi-square gates (:918-938), f32 products compared in double
                const ivf_keypoint& kp = S.kps[idx];
                if (S.uright[idx] >= 0) {
                    const float ex = u - kp.x, ey = v - kp.y, er = ur - S.uright[idx];
                    const float e2 = ex * ex + ey * ey + er * er;
                    if (e2 * inv_level_sigma2[kp.octave] > 7.8) continue;
                } else {
                    const float ex = u - kp.x, ey = v - kp.y;
                    const float e2 = ex * ex + ey * ey;
                    if (e2 * inv_level_sigma2[kp.octave] > 5.99) continue;
                }
            }
            if (dist[p] < bestDist) { bestDist = dist[p]; bestIdx = idx; }
        }
        if (best_dist) best_dist[i] = bestDist;
        if (bestDist <= 50) best_idx[i] = bestIdx;
    }
    return IVF_OK;
}
int ivf_fuse_candidates(const ivf_keypoint* kf_kps, const uint8_t* kf_desc, const float* kf_uright, int n_kf,
                        const ivf_bounds* bounds, const float* inv_level_sigma2, int n_levels,
                        int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                        const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid,
                        int32_t* best_idx, int32_t* best_dist, int device_id)
{
    if (!kf_kps || !kf_desc || !bounds || !best_idx || n_kf < 0 || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    return fuse_impl(CandSource::host(kf_kps, kf_desc, kf_uright, n_kf, bounds, device_id), inv_level_sigma2, n_levels, n_q, q_u, q_v, q_ur,
                     q_radius, q_level, q_desc, q_valid, best_idx, best_dist);
}
int ivf_frame_fuse_candidates(ivf_frame* f, const float* inv_level_sigma2, int n_levels, int n_q, const float* q_u, const float* q_v,
                              const float* q_ur, const float* q_radius, const int32_t* q_level, const uint8_t* q_desc,
                              const uint8_t* q_valid, int32_t* best_idx, int32_t* best_dist)
{
    if (!f || !best_idx || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    CandSource S; const int rc = CandSource::resident(f, S); if (rc) return rc;
    return fuse_impl(S, inv_level_sigma2, n_levels, n_q, q_u, q_v, q_ur, q_radius, q_level, q_desc, q_valid, best_idx, best_dist);
}

// ORBmatcher::SearchBySim3 (ORB/src/ORBmatcher.cc:1145-1254) on the two sets of projected map points
namespace {
int window_best(const CandSource& S, int n_q, const float* q_u, const float* q_v, const float* q_radius, const int32_t* q_level,
                const uint8_t* q_desc, const uint8_t* q_valid, int th, std::vector<int>& best)
{
    best.assign(n_q, -1);
    if (n_q == 0 || S.n == 0) return IVF_OK;
    std::vector<int32_t> lo, hi; level_window(n_q, q_level, 1, 0, lo, hi);      // octave in [level-1, level] (:1245-1246)
    std::vector<int> qStart, cand, dist;
    const int rc = S.get(n_q, q_u, q_v, q_radius, lo.data(), hi.data(), q_desc, q_valid, qStart, cand, dist);
    if (rc) return rc;
    for (int i = 0; i < n_q; i++) {
        int bestDist = INT_MAX, bestIdx = -1;
        for (int p = qStart[i]; p < qStart[i + 1]; p++)
            if (dist[p] < bestDist) { bestDist = dist[p]; bestIdx = cand[p]; }
        if (bestDist <= th) best[i] = bestIdx;
    }
    return IVF_OK;
}
int sim3_impl(const CandSource& S1, const CandSource& S2,
              const float* q12_u, const float* q12_v, const float* q12_radius, const int32_t* q12_level, const uint8_t* q12_desc,
              const uint8_t* q12_valid, const float* q21_u, const float* q21_v, const float* q21_radius, const int32_t* q21_level,
              const uint8_t* q21_desc, const uint8_t* q21_valid, int32_t* matches12, int* nfound)
{
    const int n1 = S1.n, n2 = S2.n;
    *nfound = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return IVF_OK;
    if (!q12_u || !q12_v || !q12_radius || !q12_level || !q12_desc || !q21_u || !q21_v || !q21_radius || !q21_level || !q21_desc)
        return fail(IVF_E_INVALID, "null query array");
    std::vector<int> m1, m2;                                      // vnMatch1 / vnMatch2 (:1186-1187), TH_HIGH (:1264, :1344)
    int rc = window_best(S2, n1, q12_u, q12_v, q12_radius, q12_level, q12_desc, q12_valid, 100, m1);
    if (rc) return rc;
    rc = window_best(S1, n2, q21_u, q21_v, q21_radius, q21_level, q21_desc, q21_valid, 100, m2);
    if (rc) return rc;
    int nf = 0;
    for (int i1 = 0; i1 < n1; i1++) {                             // agreement check (:1336-1349)
        const int idx2 = m1[i1];
        if (idx2 >= 0 && m2[idx2] == i1) { matches12[i1] = idx2; nf++; }
    }
    *nfound = nf;
    return IVF_OK;
}
}  // namespace

int ivf_search_by_sim3(const ivf_keypoint* kps1, const uint8_t* desc1, int n1, const ivf_bounds* bounds1,
                       const ivf_keypoint* kps2, const uint8_t* desc2, int n2, const ivf_bounds* bounds2,
                       const float* q12_u, const float* q12_v, const float* q12_radius, const int32_t* q12_level,
                       const uint8_t* q12_desc, const uint8_t* q12_valid,
                       const float* q21_u, const float* q21_v, const float* q21_radius, const int32_t* q21_level,
                       const uint8_t* q21_desc, const uint8_t* q21_valid, int32_t* matches12, int* nfound, int device_id)
{
    if (!kps1 || !desc1 || !kps2 || !desc2 || !bounds1 || !bounds2 || !matches12 || !nfound || n1 < 0 || n2 < 0)
        return fail(IVF_E_INVALID, "bad argument");
    return sim3_impl(CandSource::host(kps1, desc1, nullptr, n1, bounds1, device_id), CandSource::host(kps2, desc2, nullptr, n2, bounds2, device_id),
                     q12_u, q12_v, q12_radius, q12_level, q12_desc, q12_valid, q21_u, q21_v, q21_radius, q21_level, q21_desc, q21_valid,
                     matches12, nfound);
}
int ivf_frame_search_by_sim3(ivf_frame* f1, ivf_frame* f2,
                             const float* q12_u, const float* q12_v, const float* q12_radius, const int32_t* q12_level,
                             const uint8_t* q12_desc, const uint8_t* q12_valid,
                             const float* q21_u, const float* q21_v, const float* q21_radius, const int32_t* q21_level,
                             const uint8_t* q21_desc, const uint8_t* q21_valid, int32_t* matches12, int* nfound)
{
    if (!f1 || !f2 || !matches12 || !nfound) return fail(IVF_E_INVALID, "bad argument");
    CandSource S1, S2;
    int rc = CandSource::resident(f1, S1); if (rc) return rc;
    rc = CandSource::resident(f2, S2); if (rc) return rc;
    return sim3_impl(S1, S2, q12_u, q12_v, q12_radius, q12_level, q12_desc, q12_valid, q21_u, q21_v, q21_radius, q21_level, q21_desc,
                     q21_valid, matches12, nfound);
}

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORB/src/ORBmatcher.cc:165-294), feature vectors in CSR
int ivf_search_by_bow(const ivf_keypoint* kf_kps, const uint8_t* kf_desc, const uint8_t* kf_has_map_point, int n_kf,
                      const int32_t* kf_node, const int32_t* kf_start, const int32_t* kf_idx, int kf_nodes,
                      const ivf_keypoint* f_kps, const uint8_t* f_desc, int n_f,
                      const int32_t* f_node, const int32_t* f_start, const int32_t* f_idx, int f_nodes,
                      float nn_ratio, int check_orientation, int32_t* f_match, int* nmatches, int device_id)
{
    if (!kf_kps || !kf_desc || !kf_has_map_point || !f_kps || !f_desc || !f_match || !nmatches || n_kf < 0 || n_f < 0 ||
        kf_nodes < 0 || f_nodes < 0)
        return fail(IVF_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n_f; i++) f_match[i] = -1;
    if (kf_nodes == 0 || f_nodes == 0 || n_kf == 0 || n_f == 0) return IVF_OK;
    if (!kf_node || !kf_start || !kf_idx || !f_node || !f_start || !f_idx) return fail(IVF_E_INVALID, "null feature-vector array");
    int rc = check_feature_vector(kf_node, kf_start, kf_idx, kf_nodes, n_kf, "keyframe %s");
    if (!rc) rc = check_feature_vector(f_node, f_start, f_idx, f_nodes, n_f, "frame %s");
    if (rc) return rc;
    // 1. + 2. node merge (:187-265): per KF feature with a map point, the run of (KF, F) pairs of its node; in-node distances
    std::vector<Run> runs; std::vector<int> pairs, dist;
    rc = node_pairs(kf_desc, n_kf, kf_node, kf_start, kf_idx, kf_nodes, f_desc, n_f, f_node, f_start, f_idx, f_nodes, device_id, runs, pairs, dist,
                    [&](int i) { return kf_has_map_point[i] != 0; });
    if (rc) return rc;
    // 3. greedy replay (:200-259) and the rotation filter (:268-288)
    RotHist rotHist;
    int nm = 0;
    for (const Run& r : runs) {
        int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
        for (int k = 0; k < r.len; k++) {
            const int iF = pairs[2 * (r.first + k) + 1], d = dist[r.first + k];
            if (f_match[iF] >= 0) continue;
            if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = iF; }
            else if (d < bestDist2) bestDist2 = d;
        }
        if (bestDist1 <= 50 && (float)bestDist1 < nn_ratio * (float)bestDist2) {
            f_match[bestIdxF] = r.i1;
            if (check_orientation) rotHist.add(kf_kps[r.i1].angle - f_kps[bestIdxF].angle, bestIdxF);
            nm++;
        }
    }
    if (check_orientation) rotHist.reject_outliers([&](int j) { f_match[j] = -1; nm--; });
    *nmatches = nm;
    return IVF_OK;
}

// ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORB/src/ORBmatcher.cc:528-661), feature vectors in CSR
int ivf_search_by_bow_keyframes(const ivf_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_map_point1, int n1,
                                const int32_t* node1, const int32_t* start1, const int32_t* idx1, int nodes1,
                                const ivf_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_map_point2, int n2,
                                const int32_t* node2, const int32_t* start2, const int32_t* idx2, int nodes2,
                                float nn_ratio, int check_orientation, int32_t* matches12, int* nmatches, int device_id)
{
    if (!kps1 || !desc1 || !has_map_point1 || !kps2 || !desc2 || !has_map_point2 || !matches12 || !nmatches || n1 < 0 || n2 < 0 ||
        nodes1 < 0 || nodes2 < 0)
        return fail(IVF_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (nodes1 == 0 || nodes2 == 0 || n1 == 0 || n2 == 0) return IVF_OK;
    if (!node1 || !start1 || !idx1 || !node2 || !start2 || !idx2) return fail(IVF_E_INVALID, "null feature-vector array");
    int rc = check_feature_vector(node1, start1, idx1, nodes1, n1, "%s of keyframe 1");
    if (!rc) rc = check_feature_vector(node2, start2, idx2, nodes2, n2, "%s of keyframe 2");
    if (rc) return rc;
    // the pairs cover every KF2 feature of the node: whether it owns a map point is tested in the replay, as in the reference
    std::vector<Run> runs; std::vector<int> pairs, dist;
    rc = node_pairs(desc1, n1, node1, start1, idx1, nodes1, desc2, n2, node2, start2, idx2, nodes2, device_id, runs, pairs, dist,
                    [&](int i) { return has_map_point1[i] != 0; });
    if (rc) return rc;
    RotHist rotHist;
    std::vector<uint8_t> matched2(n2, 0);
    int nm = 0;
    for (const Run& r : runs) {
        int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
        for (int k = 0; k < r.len; k++) {
            const int i2 = pairs[2 * (r.first + k) + 1], d = dist[r.first + k];
            if (matched2[i2] || !has_map_point2[i2]) continue;
            if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdx2 = i2; }
            else if (d < bestDist2) bestDist2 = d;
        }
        if (bestDist1 < 50 && (float)bestDist1 < nn_ratio * (float)bestDist2) {          // strict '<' here (:598)
            matches12[r.i1] = bestIdx2; matched2[bestIdx2] = 1;
            if (check_orientation) rotHist.add(kps1[r.i1].angle - kps2[bestIdx2].angle, r.i1);
            nm++;
        }
    }
    if (check_orientation) rotHist.reject_outliers([&](int j) { matches12[j] = -1; nm--; });
    *nmatches = nm;
    return IVF_OK;
}

// ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist) (ORB/src/ORBmatcher.cc:1520-1652)
static int reloc_impl(const CandSource& S, int n_q, const float* q_u, const float* q_v, const float* q_radius, const int32_t* q_level,
                      const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid, int orb_dist, int check_orientation,
                      int32_t* cur_assign, int* nmatches)
{
    const ivf_keypoint* cur_kps = S.kps;
    *nmatches = 0;
    if (n_q == 0 || S.n == 0) return IVF_OK;
    if (!q_u || !q_v || !q_radius || !q_level || !q_angle || !q_desc) return fail(IVF_E_INVALID, "null query array");
    std::vector<int32_t> lo, hi; level_window(n_q, q_level, 1, 1, lo, hi);      // GetFeaturesInArea(u, v, radius, level-1, level+1) (:1574)
    std::vector<int> qStart, cand, dist;
    int rc = S.get(n_q, q_u, q_v, q_radius, lo.data(), hi.data(), q_desc, q_valid, qStart, cand, dist);
    if (rc) return rc;
    RotHist rotHist;
    int nm = 0;
    for (int i = 0; i < n_q; i++) {
        int bestDist = 256, bestIdx2 = -1;
        for (int p = qStart[i]; p < qStart[i + 1]; p++) {
            const int i2 = cand[p];
            if (cur_assign[i2] != -1) continue;
            if (dist[p] < bestDist) { bestDist = dist[p]; bestIdx2 = i2; }
        }
        if (bestDist <= orb_dist && bestIdx2 >= 0) {
            cur_assign[bestIdx2] = i; nm++;
            if (check_orientation) rotHist.add(q_angle[i] - cur_kps[bestIdx2].angle, bestIdx2);
        }
    }
    if (check_orientation) rotHist.reject_outliers([&](int j) { cur_assign[j] = -1; nm--; });
    *nmatches = nm;
    return IVF_OK;
}

int ivf_search_by_projection_reloc(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, int n_cur, const ivf_bounds* bounds,
                                   int n_q, const float* q_u, const float* q_v, const float* q_radius, const int32_t* q_level,
                                   const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid,
                                   int orb_dist, int check_orientation, int32_t* cur_assign, int* nmatches, int device_id)
{
    if (!cur_kps || !cur_desc || !bounds || !cur_assign || !nmatches || n_cur < 0 || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    return reloc_impl(CandSource::host(cur_kps, cur_desc, nullptr, n_cur, bounds, device_id), n_q, q_u, q_v, q_radius, q_level, q_angle,
                      q_desc, q_valid, orb_dist, check_orientation, cur_assign, nmatches);
}
int ivf_frame_search_by_projection_reloc(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_radius,
                                         const int32_t* q_level, const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid,
                                         int orb_dist, int check_orientation, int32_t* cur_assign, int* nmatches)
{
    if (!f || !cur_assign || !nmatches || n_q < 0) return fail(IVF_E_INVALID, "bad argument");
    CandSource S; const int rc = CandSource::resident(f, S); if (rc) return rc;
    return reloc_impl(S, n_q, q_u, q_v, q_radius, q_level, q_angle, q_desc, q_valid, orb_dist, check_orientation, cur_assign, nmatches);
}

// ORBmatcher::SearchForTriangulation (ORB/src/ORBmatcher.cc:663-829) + CheckDistEpipolarLine (:146-163)
int ivf_search_for_triangulation(const ivf_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_map_point1, const uint8_t* stereo1, int n1,
                                 const int32_t* node1, const int32_t* start1, const int32_t* idx1, int nodes1,
                                 const ivf_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_map_point2, const uint8_t* stereo2, int n2,
                                 const int32_t* node2, const int32_t* start2, const int32_t* idx2, int nodes2,
                                 const float* F12, float ex, float ey, const float* scale_factors2, const float* level_sigma2_2, int n_levels,
                                 int only_stereo, int check_orientation, int32_t* matches12, int* nmatches, int device_id)
{
    if (!kps1 || !desc1 || !has_map_point1 || !stereo1 || !kps2 || !desc2 || !has_map_point2 || !stereo2 || !F12 || !scale_factors2 ||
        !level_sigma2_2 || !matches12 || !nmatches || n1 < 0 || n2 < 0 || nodes1 < 0 || nodes2 < 0 || n_levels < 1)
        return fail(IVF_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (nodes1 == 0 || nodes2 == 0 || n1 == 0 || n2 == 0) return IVF_OK;
    if (!node1 || !start1 || !idx1 || !node2 || !start2 || !idx2) return fail(IVF_E_INVALID, "null feature-vector array");
    int rc = check_feature_vector(node1, start1, idx1, nodes1, n1, "%s of keyframe 1");
    if (!rc) rc = check_feature_vector(node2, start2, idx2, nodes2, n2, "%s of keyframe 2");
    if (rc) return rc;
    for (int i = 0; i < n2; i++) if (kps2[i].octave < 0 || kps2[i].octave >= n_levels) return fail(IVF_E_INVALID, "keypoint %d of keyframe 2: octave outside the tables", i);
    // 1. node merge: per eligible KF1 feature the run of eligible (i1, i2) pairs of its node (:697-731), their distances
    std::vector<Run> runs; std::vector<int> pairs, dist;
    rc = node_pairs(desc1, n1, node1, start1, idx1, nodes1, desc2, n2, node2, start2, idx2, nodes2, device_id, runs, pairs, dist,
                    [&](int i1) { return !(has_map_point1[i1] || (only_stereo && !stereo1[i1])); },
                    [&](int i2) { return !(has_map_point2[i2] || (only_stereo && !stereo2[i2])); });
    if (rc) return rc;
    // 2. replay with the epipole and epipolar-line gates (f32 arithmetic as written in :149-162, compared in double)
    const int TH_LOW = 50;
    RotHist rotHist;
    int nm = 0;
    for (const Run& r : runs) {
        const ivf_keypoint& kp1 = kps1[r.i1];
        int bestDist = TH_LOW, bestIdx2 = -1;
        for (int k = 0; k < r.len; k++) {
            const int i2 = pairs[2 * (r.first + k) + 1], d = dist[r.first + k];
            if (d > TH_LOW || d > bestDist) continue;
            const ivf_keypoint& kp2 = kps2[i2];
            if (!stereo1[r.i1] && !stereo2[i2]) {
                const float distex = ex - kp2.x, distey = ey - kp2.y;
                if (distex * distex + distey * distey < 100 * scale_factors2[kp2.octave]) continue;
            }
            const float a = kp1.x * F12[0] + kp1.y * F12[3] + F12[6];
            const float b = kp1.x * F12[1] + kp1.y * F12[4] + F12[7];
            const float c = kp1.x * F12[2] + kp1.y * F12[5] + F12[8];
            const float num = a * kp2.x + b * kp2.y + c;
            const float den = a * a + b * b;
            if (den == 0) continue;
            const float dsqr = num * num / den;
            if (dsqr < 3.84 * level_sigma2_2[kp2.octave]) { bestIdx2 = i2; bestDist = d; }
        }
        if (bestIdx2 >= 0) {
            matches12[r.i1] = bestIdx2; nm++;
            if (check_orientation) rotHist.add(kp1.angle - kps2[bestIdx2].angle, r.i1);
        }
    }
    if (check_orientation) rotHist.reject_outliers([&](int j) { matches12[j] = -1; nm--; });
    *nmatches = nm;
    return IVF_OK;
}

// DBoW2 vocabulary (device-resident tree) and TemplatedVocabulary::transform per descriptor
struct ivf_vocabulary {
    int device = 0, nNodes = 0, depth = 0, maxChildren = 0;
    int *dChildStart = nullptr, *dChild = nullptr; uint8_t* dDesc = nullptr;
    uint8_t* dLive = nullptr;             // [nNodes] weight > 0: what the batched matcher (ivf_track_bow.hip) needs of the weights
    int* dWord = nullptr; double* dWeight = nullptr;   // [nNodes] word id and weight: the batched mBowVec (ivf_track_db.hip)
    std::vector<int> word; std::vector<double> weight; std::vector<int> childStart;
};

int ivf_vocabulary_create(int n_nodes, const int32_t* child_start, const int32_t* child, const uint8_t* node_desc,
                          const int32_t* node_word, const double* node_weight, int depth_L, int device_id, ivf_vocabulary** out)
{
    if (!out) return fail(IVF_E_INVALID, "null argument");
    *out = nullptr;
    if (n_nodes < 2 || !child_start || !child || !node_desc || !node_word || !node_weight || depth_L < 1)
        return fail(IVF_E_INVALID, "bad argument");
    if (child_start[0] != 0) return fail(IVF_E_INVALID, "child_start[0] must be 0");
    const int nChild = child_start[n_nodes];
    if (child_start[1] == child_start[0]) return fail(IVF_E_INVALID, "the root (node 0) has no children");
    int maxC = 0;
    for (int i = 0; i < n_nodes; i++) {
        if (child_start[i + 1] < child_start[i]) return fail(IVF_E_INVALID, "child_start must not decrease (node %d)", i);
        maxC = std::max(maxC, child_start[i + 1] - child_start[i]);
    }
    if (maxC > 65535) return fail(IVF_E_INVALID, "more than 65535 children under one node");
    for (int c = 0; c < nChild; c++) if (child[c] <= 0 || child[c] >= n_nodes) return fail(IVF_E_INVALID, "child %d: node id out of range", c);
    {   // the descent kernel loops until it meets a leaf: refuse anything that is not a tree rooted at node 0
        std::vector<char> seen(n_nodes, 0); std::vector<int> stack{0}; seen[0] = 1;
        while (!stack.empty()) {
            const int i = stack.back(); stack.pop_back();
            for (int c = child_start[i]; c < child_start[i + 1]; c++) {
                if (seen[child[c]]) return fail(IVF_E_INVALID, "node %d is reachable twice: not a tree", child[c]);
                seen[child[c]] = 1; stack.push_back(child[c]);
            }
        }
    }
    int rc = have_device(device_id);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device_id));
    ivf_vocabulary* v = new ivf_vocabulary();
    v->device = device_id; v->nNodes = n_nodes; v->depth = depth_L; v->maxChildren = maxC;
    v->word.assign(node_word, node_word + n_nodes); v->weight.assign(node_weight, node_weight + n_nodes);
    v->childStart.assign(child_start, child_start + n_nodes + 1);
    if (hipMalloc(&v->dChildStart, (size_t)(n_nodes + 1) * sizeof(int)) != hipSuccess || hipMalloc(&v->dChild, (size_t)std::max(nChild, 1) * sizeof(int)) != hipSuccess ||
        hipMalloc(&v->dDesc, (size_t)n_nodes * 32) != hipSuccess || hipMalloc(&v->dLive, (size_t)n_nodes) != hipSuccess ||
        hipMalloc(&v->dWord, (size_t)n_nodes * sizeof(int)) != hipSuccess || hipMalloc(&v->dWeight, (size_t)n_nodes * sizeof(double)) != hipSuccess) {
        ivf_vocabulary_destroy(v);
        return fail(IVF_E_NO_DEVICE, "hipMalloc failed for the vocabulary");
    }
    std::vector<uint8_t> live(n_nodes);
    for (int i = 0; i < n_nodes; i++) live[i] = node_weight[i] > 0 ? 1 : 0;
    if (hipMemcpy(v->dChildStart, child_start, (size_t)(n_nodes + 1) * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->dChild, child, (size_t)nChild * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->dDesc, node_desc, (size_t)n_nodes * 32, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->dLive, live.data(), (size_t)n_nodes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->dWord, node_word, (size_t)n_nodes * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->dWeight, node_weight, (size_t)n_nodes * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        ivf_vocabulary_destroy(v);
        return fail(IVF_E_NO_DEVICE, "vocabulary upload failed");
    }
    *out = v;
    return IVF_OK;
}

void ivf_vocabulary_destroy(ivf_vocabulary* v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->dChildStart) (void)hipFree(v->dChildStart);
    if (v->dChild) (void)hipFree(v->dChild);
    if (v->dDesc) (void)hipFree(v->dDesc);
    if (v->dLive) (void)hipFree(v->dLive);
    if (v->dWord) (void)hipFree(v->dWord);
    if (v->dWeight) (void)hipFree(v->dWeight);
    delete v;
}

int ivf_bow_transform(const ivf_vocabulary* v, const uint8_t* desc, int n, int levelsup, int32_t* word_id, int32_t* node_id, double* weight)
{
    if (!v || n < 0 || (n > 0 && (!desc || !word_id || !node_id || !weight))) return fail(IVF_E_INVALID, "bad argument");
    if (n == 0) return IVF_OK;
    HIPCHK(hipSetDevice(v->device));
    uint8_t* scb = nullptr;
    const int src = thread_scratch(v->device, (size_t)n * 32 + 256 + (size_t)n * 2 * sizeof(int), &scb);
    if (src) return src;
    uint8_t* dD = scb; int* dOut = (int*)(scb + (((size_t)n * 32 + 255) & ~(size_t)255));
    HIPCHK(hipMemcpyAsync(dD, desc, (size_t)n * 32, hipMemcpyHostToDevice, nullptr));
    launch_bow_transform(v->dChildStart, v->dChild, v->dDesc, dD, n, v->depth - levelsup, dOut, dOut + n, nullptr);
    HIPCHK(hipGetLastError());
    std::vector<int> res((size_t)n * 2);
    HIPCHK(hipMemcpy(res.data(), dOut, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost));
    for (int f = 0; f < n; f++) {
        const int leaf = res[f];
        word_id[f] = v->word[leaf]; weight[f] = v->weight[leaf]; node_id[f] = res[(size_t)n + f];
    }
    return IVF_OK;
}

// BowVector / FeatureVector of one frame from the per-descriptor results (TemplatedVocabulary.h:1126-1204 with TF_IDF weights
// and L1 normalisation, the ORB vocabulary's settings; BowVector.cpp:34-46, 62-84; FeatureVector.cpp:31-45)
int ivf_bow_vectors(const int32_t* word_id, const int32_t* node_id, const double* weight, int n,
                    int32_t* bow_word, double* bow_value, int bow_cap, int* bow_n,
                    int32_t* fv_node, int32_t* fv_start, int32_t* fv_idx, int fv_cap, int* fv_n)
{
    if (n < 0 || !bow_n || !fv_n || (n > 0 && (!word_id || !node_id || !weight))) return fail(IVF_E_INVALID, "bad argument");
    std::map<int, double> bow; std::map<int, std::vector<int>> fv;
    for (int f = 0; f < n; f++) {
        if (!(weight[f] > 0)) continue;                                  // stopped word (:1157)
        bow[word_id[f]] += weight[f];                                    // addWeight
        fv[node_id[f]].push_back(f);                                     // addFeature
    }
    double norm = 0.0;
    for (auto& kv : bow) norm += fabs(kv.second);                        // L1 (BowVector.cpp:67-71)
    if (norm > 0.0) for (auto& kv : bow) kv.second /= norm;
    *bow_n = (int)bow.size(); *fv_n = (int)fv.size();
    if ((int)bow.size() > bow_cap || (int)fv.size() > fv_cap) return fail(IVF_E_CAPACITY, "%zu words / %zu nodes exceed the capacities", bow.size(), fv.size());
    int k = 0;
    for (auto& kv : bow) { if (bow_word) bow_word[k] = kv.first; if (bow_value) bow_value[k] = kv.second; k++; }
    k = 0; int pos = 0;
    if (fv_start) fv_start[0] = 0;
    for (auto& kv : fv) {
        if (fv_node) fv_node[k] = kv.first;
        for (int i : kv.second) { if (fv_idx) fv_idx[pos] = i; pos++; }
        if (fv_start) fv_start[k + 1] = pos;
        k++;
    }
    return IVF_OK;
}

// MapPoint::ComputeDistinctiveDescriptors (ORB/src/MapPoint.cc:247-312): all-pairs Hamming + row medians on the device,
// first minimum on the host
int ivf_distinctive_descriptor(const uint8_t* desc, int n, int* best_index, int* best_median, int device_id)
{
    if (!desc || !best_index || n < 1) return fail(IVF_E_INVALID, "bad argument");
    int rc = have_device(device_id);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device_id));
    uint8_t* scb = nullptr;
    rc = thread_scratch(device_id, (size_t)n * 32 + 256 + (size_t)n * sizeof(int), &scb);
    if (rc) return rc;
    uint8_t* dD = scb; int* dM = (int*)(scb + (((size_t)n * 32 + 255) & ~(size_t)255));
    HIPCHK(hipMemcpyAsync(dD, desc, (size_t)n * 32, hipMemcpyHostToDevice, nullptr));
    launch_distinct_median(dD, n, dM, nullptr);
    HIPCHK(hipGetLastError());
    std::vector<int> med(n);
    HIPCHK(hipMemcpy(med.data(), dM, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    int bm = INT_MAX, bi = 0;
    for (int i = 0; i < n; i++) if (med[i] < bm) { bm = med[i]; bi = i; }
    *best_index = bi;
    if (best_median) *best_median = bm;
    return IVF_OK;
}

// ORBmatcher::UpdateQualityScores(Frame &F) (ORB/src/ORBmatcher.cc:1108-1121): host bookkeeping, sequential by definition
int ivf_update_quality_scores(const int32_t* assign, int n, float* kp_quality, float* mp_quality, int n_map_points)
{
    if (!assign || !kp_quality || !mp_quality || n < 0 || n_map_points < 0) return fail(IVF_E_INVALID, "bad argument");
    const float kDeltaThresh = 0.01f;
    for (int i = 0; i < n; i++) {
        const int m = assign[i];
        if (m < 0) continue;
        if (m >= n_map_points) return fail(IVF_E_INVALID, "assign[%d] = %d outside the %d map points", i, m, n_map_points);
        const float mpt = mp_quality[m];
        const float upd = std::min(mpt, kp_quality[i]);
        if (fabsf(upd - mpt) > kDeltaThresh) mp_quality[m] = upd;
        kp_quality[i] = upd;
    }
    return IVF_OK;
}

}  // extern "C"

int ivf::vocabulary_view(const ivf_vocabulary* v, VocabularyView* out)
{
    if (!v || !out) return fail(IVF_E_INVALID, "null vocabulary");
    *out = VocabularyView{v->device, v->nNodes, v->depth, v->dChildStart, v->dChild, v->dDesc, v->dLive, v->dWord, v->dWeight};
    return IVF_OK;
}

// The frame half of ivf_frame_create_from_frontend (ivf_api.hip resolves the batch image): keypoints, descriptors and uRight go
// device -> device on the frame's own stream, the 64x48 grid is built on the device; nothing but the 4-byte keypoint count
// crosses PCIe (the replays' small host mirror is fetched lazily by the first search)
int ivf::frame_from_batch(int device, const BatchImage& src, const ivf_bounds& bounds, ivf_frame** out)
{
    ivf_frame* f = new ivf_frame();
    f->device = device; f->bd = bounds; f->hostKps = false; f->hostDesc = false;
    f->geom = grid_geom(bounds);
    auto bail = [&](const char* what) { ivf_frame_destroy(f); return fail(IVF_E_NO_DEVICE, "%s failed for a frame from the front end", what); };
    // sized for the batch's capacity: the (pooled) arena is acquired before the keypoint count is known
    if (frame_alloc(f, src.cap) != IVF_OK) { ivf_frame_destroy(f); return IVF_E_NO_DEVICE; }
    int n = 0;
    if (hipStreamWaitEvent(f->stream, src.done, 0) != hipSuccess ||
        hipMemcpyAsync(&n, src.count, sizeof(int), hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess) return bail("count read");
    f->n = n;
    if (n > 0) {
        if (hipMemcpyAsync(f->dKps, src.kps, (size_t)n * sizeof(ivf_keypoint), hipMemcpyDeviceToDevice, f->stream) != hipSuccess ||
            hipMemcpyAsync(f->dDesc, src.desc, (size_t)n * 32, hipMemcpyDeviceToDevice, f->stream) != hipSuccess)
            return bail("device copy");
        if (src.uright) { if (hipMemcpyAsync(f->dUright, src.uright, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, f->stream) != hipSuccess) return bail("device copy"); }
        else if (hipMemsetD32Async((hipDeviceptr_t)f->dUright, (int)0xbf800000, (size_t)n, f->stream) != hipSuccess) return bail("fill");      // -1.0f: no stereo
    }
    launch_grid_build(f->dKps, n, f->geom, f->dStart, f->dIdx, f->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(f->stream) != hipSuccess) return bail("grid build");
    *out = f;
    return IVF_OK;
}
