// ivf_grid.h -- the one device text of the frame grid (Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea,
// ORB/src/Frame.cc:415-430, :615-680), shared by the device-resident ivf_frame (ivf_match.hip, int indices: the ivf_frame_grid ABI)
// and the batched tracker (ivf_track.hip, ivf_track_local.hip; unsigned short indices: nfeatures <= 4096), with the two wave helpers the walk needs
// (ivf_kernels.hip's stereo matcher uses them too).
#pragma once
#include "ivf_device.h"

namespace ivf {

constexpr int kGC = 64, kGR = 48;                 // FRAME_GRID_COLS / ROWS (ORB/include/Frame.h:43-44)

// image bounds' origin and mfGridElementWidthInv / HeightInv (Frame.cc:208-209)
struct GridGeom { float minX, minY, invW, invH; };
inline GridGeom grid_geom(const ivf_bounds& bd)
{
    return GridGeom{bd.min_x, bd.min_y, (float)kGC / (bd.max_x - bd.min_x), (float)kGR / (bd.max_y - bd.min_y)};
}

// DescriptorDistance (ORBmatcher.cc:1700-1716): 256-bit Hamming = 8 x v_bcnt_u32_b32
__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// minimum over the wave without a trip through the LDS crossbar: row_shr 1/2/4/8 folds each row of 16 lanes into its lane 15
// (wave_row_min_u32: the four row minima), row_bcast15 / row_bcast31 fold the four rows into lane 63, which every lane then reads
__device__ __forceinline__ unsigned wave_row_min_u32(unsigned v)
{
    const int idn = -1;                           // 0xFFFFFFFF: identity of the unsigned minimum
    unsigned t;
    t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x111, 0xf, 0xf, false); v = t < v ? t : v;   // row_shr:1
    t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x112, 0xf, 0xf, false); v = t < v ? t : v;   // row_shr:2
    t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x114, 0xf, 0xf, false); v = t < v ? t : v;   // row_shr:4
    t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x118, 0xf, 0xf, false); v = t < v ? t : v;   // row_shr:8
    return v;
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    const int idn = -1;
    unsigned t;
    v = wave_row_min_u32(v);
    t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x142, 0xa, 0xf, false); v = t < v ? t : v;   // row_bcast:15 -> rows 1, 3
    t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x143, 0xc, 0xf, false); v = t < v ? t : v;   // row_bcast:31 -> rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Frame::AssignFeaturesToGrid (Frame.cc:415-430) by ONE 256-thread workgroup: the 64x48 bucket grid in CSR form, buckets in the
// reference's enumeration order (cell = ix * 48 + iy), keypoints of a bucket in insertion order (a stable counting sort: the rank
// of a keypoint inside its bucket = same-bucket keypoints in earlier 256-blocks + earlier threads of its own block).
// start [kGC * kGR + 1], idx [n]; cnt [kGC * kGR], part [256], blk [256]: workgroup scratch in LDS.
template <class IDX>
__device__ __forceinline__ void grid_build(const GridGeom G, const ivf_keypoint* __restrict__ kps, int n, int* __restrict__ start,
                                           IDX* __restrict__ idx, int* cnt, int* part, int* blk, int tid)
{
    for (int c = tid; c < kGC * kGR; c += 256) cnt[c] = 0;
    __syncthreads();
    auto cell_of = [&](int i) {
        const int px = (int)roundf((kps[i].x - G.minX) * G.invW), py = (int)roundf((kps[i].y - G.minY) * G.invH);   // PosInGrid :672-673
        return (px < 0 || px >= kGC || py < 0 || py >= kGR) ? -1 : px * kGR + py;
    };
    for (int i = tid; i < n; i += 256) { const int c = cell_of(i); if (c >= 0) atomicAdd(&cnt[c], 1); }
    __syncthreads();
    // exclusive prefix over the 3072 buckets: 12 per thread + a block scan of the partial sums
    constexpr int PER = kGC * kGR / 256;
    int local[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { local[k] = sum; sum += cnt[tid * PER + k]; }
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const int base = part[tid] - sum;
#pragma unroll
    for (int k = 0; k < PER; k++) { start[tid * PER + k] = base + local[k]; cnt[tid * PER + k] = base + local[k]; }   // cnt becomes the fill cursor
    if (tid == 255) start[kGC * kGR] = part[255];
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const int c = i < n ? cell_of(i) : -1;
        blk[tid] = c;
        __syncthreads();
        if (c >= 0) {
            int before = 0;
            for (int t = 0; t < tid; t++) before += blk[t] == c ? 1 : 0;
            idx[cnt[c] + before] = (IDX)i;
        }
        __syncthreads();
        if (c >= 0) atomicAdd(&cnt[c], 1);
        __syncthreads();
    }
}

// Frame::GetFeaturesInArea (Frame.cc:615-668) for one query, walked by ONE wave 64 candidates at a time in the reference's
// order (grid column ix outer, row iy inner, insertion order inside a bucket -- the buckets of a column are one contiguous run
// of `idx`, so the window is at most 64 runs).  f(ok, i2, dist) is called by all lanes for every step; ok = the lane holds a
// candidate that passed the octave and box filters (:636-664), dist = its Hamming distance to the query descriptor.
template <class IDX, class F>
__device__ __forceinline__ void grid_walk(const GridGeom G, const ivf_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                          const int* __restrict__ start, const IDX* __restrict__ idx, float x, float y, float r,
                                          int minL, int maxL, const uint4 qa, const uint4 qb, int lane, F&& f)
{
    const int x0 = max(0, (int)floorf((x - G.minX - r) * G.invW)), x1 = min(kGC - 1, (int)ceilf((x - G.minX + r) * G.invW));   // :620-634
    const int y0 = max(0, (int)floorf((y - G.minY - r) * G.invH)), y1 = min(kGR - 1, (int)ceilf((y - G.minY + r) * G.invH));
    if (!(x0 < kGC && x1 >= 0 && y0 < kGR && y1 >= 0)) return;
    const bool chk = (minL > 0) || (maxL >= 0);
    for (int ix = x0; ix <= x1; ix++) {
        const int s = start[ix * kGR + y0], e = start[ix * kGR + y1 + 1];
        for (int j0 = s; j0 < e; j0 += 64) {
            const int j = j0 + lane;
            bool ok = j < e;
            int i2 = 0, d = 0;
            if (ok) {
                i2 = idx[j];
                const ivf_keypoint kp = kps[i2];
                if (chk) { if (kp.octave < minL) ok = false; if (maxL >= 0 && kp.octave > maxL) ok = false; }
                if (!(fabsf(kp.x - x) < r && fabsf(kp.y - y) < r)) ok = false;
                if (ok) {
                    const uint4* cd = (const uint4*)(desc + (size_t)i2 * 32);
                    d = hamming256(cd[0], cd[1], qa, qb);
                }
            }
            f(ok, i2, d);
        }
    }
}

}  // namespace ivf
