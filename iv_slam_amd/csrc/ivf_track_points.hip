// ivf_track_points.hip -- the points a batched search hands to a solver (ivf_pose.hip, ivf_pnp.hip), on the tracker handle
// (ivf_tracker.h): for every keypoint of a frame the world position of what the search assigned to it, and a flag; and the tail of
// Tracking::TrackLocalMap (ORB/src/Tracking.cc:1636-1691) around them, on a frame's map-point indices (ivf_tracker_update_local_map).
//
//   k_points_from_pairs     xw[p][i2] = Frame::UnprojectStereo (ORB/src/Frame.cc:958-972) of keypoint assign[p][i2] of the LAST record of pair p
//                           under its last pose (ivf_tracker_run's assignment): unproject_stereo, the arithmetic k_track_prepare projected with
//   k_points_from_local     GetWorldPos() of the local map point every keypoint was assigned by ivf_tracker_search_local
//   k_points_from_keyframe  xw[p][i] = GetWorldPos() of the map point that keyframe keypoint assign[p][i] holds (ivf_tracker_search_by_bow;
//                           Tracking.cc:1173: mvpMapPoints = vpMapPointMatches)
//   k_merge_local           framePoints[f][i] = the map-point index of the local point ivf_tracker_search_local gave keypoint i (ORBmatcher.cc:124)
//   k_points_from_map       GetWorldPos() and the quality score of the map point every keypoint holds: PoseOptimization over all of them
//   k_close_local_map       mnMatchesInliers and the stereo outliers' release (Tracking.cc:1648-1677)
#include "ivf_tracker.h"

using namespace ivf;

namespace {

// A keypoint's point and flag, zeros until set(); the tail of the three kernels stores them to slot o
struct Point {
    float x[3] = {0.0f, 0.0f, 0.0f};
    uint8_t has = 0;
    __device__ __forceinline__ void set(const float* pos) { x[0] = pos[0]; x[1] = pos[1]; x[2] = pos[2]; has = 1; }
    __device__ __forceinline__ void store(float* __restrict__ xw, uint8_t* __restrict__ hasPoint, size_t o) const
    {
        xw[3 * o] = x[0]; xw[3 * o + 1] = x[1]; xw[3 * o + 2] = x[2];
        hasPoint[o] = has;
    }
};

__global__ __launch_bounds__(256) void k_points_from_pairs(TrackParams P, const uint8_t* __restrict__ records, const int2* __restrict__ pairs,
                                                          const float* __restrict__ poses, const int* __restrict__ assign,
                                                          float* __restrict__ xw, uint8_t* __restrict__ hasPoint)
{
    const int p = blockIdx.y, i2 = blockIdx.x * 256 + threadIdx.x;
    if (i2 >= P.nf) return;
    const size_t o = (size_t)p * P.nf + i2;
    Point pt;
    const int2 pr = pairs[p];
    if (rec_ok(P.nRecords, pr.x)) {
        const uint8_t* recL = records + (size_t)pr.x * P.recBytes;
        const int a = assign[o];
        if (a >= 0 && a < rec_count(recL, P.nf)) {
            const float z = rec_depth(recL, P.nf)[a];
            if (z > 0) {
                float Rl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tl[3] = {0, 0, 0};
                if (poses) load_pose(poses + (size_t)p * 24, Rl, tl);
                float out[3];
                unproject_stereo(P, Rl, tl, rec_kps(recL)[a], z, out);
                pt.set(out);
            }
        }
    }
    pt.store(xw, hasPoint, o);
}

__global__ __launch_bounds__(256) void k_points_from_local(int nf, const ivf_local_point* __restrict__ points, const int* __restrict__ offsets,
                                                          const int* __restrict__ assign, float* __restrict__ xw, uint8_t* __restrict__ hasPoint)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const size_t o = (size_t)f * nf + i;
    const int m0 = offsets[f], M = offsets[f + 1] - m0, a = assign[o];
    Point pt;
    if (m0 >= 0 && a >= 0 && a < M) pt.set(points[(size_t)m0 + a].pos);
    pt.store(xw, hasPoint, o);
}

__global__ __launch_bounds__(256) void k_points_from_keyframe(int nf, int nRecords, const int2* __restrict__ pairs, const float* __restrict__ kfXw,
                                                             const int* __restrict__ assign, float* __restrict__ xw, uint8_t* __restrict__ hasPoint)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const size_t o = (size_t)p * nf + i;
    const int kf = pairs[p].x, a = assign[o];
    Point pt;
    if (rec_ok(nRecords, kf) && a >= 0 && a < nf) pt.set(kfXw + ((size_t)kf * nf + a) * 3);
    pt.store(xw, hasPoint, o);
}

__global__ __launch_bounds__(256) void k_merge_local(int nf, const int* __restrict__ pointIds, const int* __restrict__ offsets, const int* __restrict__ assign,
                                                    int* __restrict__ framePoints)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const size_t o = (size_t)f * nf + i;
    const int m0 = offsets[f], M = offsets[f + 1] - m0, a = assign[o];
    if (m0 >= 0 && a >= 0 && a < M) framePoints[o] = pointIds[(size_t)m0 + a];
}

__global__ __launch_bounds__(256) void k_points_from_map(int nf, const ivf_local_point* __restrict__ mapPoints, int nPoints, const float* __restrict__ pointQuality,
                                                        const int* __restrict__ framePoints, float* __restrict__ xw, uint8_t* __restrict__ hasPoint,
                                                        float* __restrict__ quality)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const size_t o = (size_t)f * nf + i;
    const int m = framePoints[o];
    Point pt;
    float q = 1.0f;
    if ((unsigned)m < (unsigned)nPoints) {
        pt.set(mapPoints[m].pos);
        if (pointQuality) q = pointQuality[m];
    }
    pt.store(xw, hasPoint, o);
    if (quality) quality[o] = q;
}

// one workgroup per frame: the count is a sum of integers, the same in every run
__global__ __launch_bounds__(256) void k_close_local_map(int nf, const ivf_local_point* __restrict__ mapPoints, int nPoints, const uint8_t* __restrict__ outlier,
                                                        int onlyTracking, int stereo, int* __restrict__ framePoints, int* __restrict__ ninliers)
{
    __shared__ int s_n;
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int n = 0;
    for (int i = tid; i < nf; i += 256) {
        const size_t o = (size_t)f * nf + i;
        const int m = framePoints[o];
        if ((unsigned)m >= (unsigned)nPoints) continue;
        if (!outlier[o]) n += (onlyTracking || (mapPoints[m].flags & 2)) ? 1 : 0;                  // :1660-1666
        else if (stereo) framePoints[o] = -1;                                                      // :1673-1674
    }
    if (n) atomicAdd(&s_n, n);
    __syncthreads();
    if (tid == 0) ninliers[f] = s_n;
}

}  // namespace

extern "C" {

int ivf_tracker_points_from_pairs(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                                  const float* d_poses_pairs, const int32_t* d_assign, float* d_xw, uint8_t* d_has_point, void* hip_stream)
{
    if (!t || !d_records || !d_pairs || !d_assign || !d_xw || !d_has_point) return fail(IVF_E_INVALID, "null argument");
    if (((size_t)d_records & 15) != 0) return fail(IVF_E_INVALID, "the record block must be 16-byte aligned");
    if (n_pairs == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, true, record_bytes, n_records, n_pairs, st);
    if (rc != IVF_OK) return rc;
    TrackParams P = t->P;
    P.nRecords = n_records;
    hipLaunchKernelGGL(k_points_from_pairs, dim3((P.nf + 255) / 256, n_pairs), dim3(256), 0, st, P, d_records, (const int2*)d_pairs, d_poses_pairs, d_assign,
                       d_xw, d_has_point);
    return tracker_end(t, st);
}

int ivf_tracker_points_from_local(ivf_tracker* t, const ivf_local_point* d_points, const int32_t* d_point_offsets, const int32_t* d_assign, int n_frames,
                                  float* d_xw, uint8_t* d_has_point, void* hip_stream)
{
    if (!t || !d_points || !d_point_offsets || !d_assign || !d_xw || !d_has_point) return fail(IVF_E_INVALID, "null argument");
    if (((size_t)d_points & 15) != 0) return fail(IVF_E_INVALID, "the point array must be 16-byte aligned");
    if (n_frames == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, false, 0, 0, n_frames, st);
    if (rc != IVF_OK) return rc;
    hipLaunchKernelGGL(k_points_from_local, dim3((t->P.nf + 255) / 256, n_frames), dim3(256), 0, st, t->P.nf, d_points, d_point_offsets, d_assign, d_xw, d_has_point);
    return tracker_end(t, st);
}

int ivf_tracker_points_from_keyframe(ivf_tracker* t, const int32_t* d_pairs, int n_pairs, int n_records, const float* d_kf_xw,
                                     const int32_t* d_assign, float* d_xw, uint8_t* d_has_point, void* hip_stream)
{
    if (!t || !d_pairs || !d_kf_xw || !d_assign || !d_xw || !d_has_point) return fail(IVF_E_INVALID, "null argument");
    if (n_records < 1) return fail(IVF_E_INVALID, "n_records must be >= 1");
    if (n_pairs == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, false, 0, 0, n_pairs, st);
    if (rc != IVF_OK) return rc;
    hipLaunchKernelGGL(k_points_from_keyframe, dim3((t->P.nf + 255) / 256, n_pairs), dim3(256), 0, st, t->P.nf, n_records, (const int2*)d_pairs, d_kf_xw,
                       d_assign, d_xw, d_has_point);
    return tracker_end(t, st);
}

int ivf_tracker_merge_local(ivf_tracker* t, const int32_t* d_point_ids, const int32_t* d_point_offsets, const int32_t* d_assign, int n_frames,
                            int32_t* d_frame_points, void* hip_stream)
{
    if (!t || !d_point_ids || !d_point_offsets || !d_assign || !d_frame_points) return fail(IVF_E_INVALID, "null argument");
    if (n_frames == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, false, 0, 0, n_frames, st);
    if (rc != IVF_OK) return rc;
    hipLaunchKernelGGL(k_merge_local, dim3((t->P.nf + 255) / 256, n_frames), dim3(256), 0, st, t->P.nf, d_point_ids, d_point_offsets, d_assign, d_frame_points);
    return tracker_end(t, st);
}

int ivf_tracker_points_from_map(ivf_tracker* t, const ivf_local_point* d_map_points, int n_points, const float* d_point_quality,
                                const int32_t* d_frame_points, int n_frames, float* d_xw, uint8_t* d_has_point, float* d_quality, void* hip_stream)
{
    if (!t || !d_frame_points || !d_xw || !d_has_point || (n_points > 0 && !d_map_points)) return fail(IVF_E_INVALID, "null argument");
    if (n_points < 0) return fail(IVF_E_INVALID, "n_points must be >= 0");
    if (((size_t)d_map_points & 15) != 0) return fail(IVF_E_INVALID, "the point array must be 16-byte aligned");
    if (n_frames == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, false, 0, 0, n_frames, st);
    if (rc != IVF_OK) return rc;
    hipLaunchKernelGGL(k_points_from_map, dim3((t->P.nf + 255) / 256, n_frames), dim3(256), 0, st, t->P.nf, d_map_points, n_points, d_point_quality,
                       d_frame_points, d_xw, d_has_point, d_quality);
    return tracker_end(t, st);
}

int ivf_tracker_close_local_map(ivf_tracker* t, const ivf_local_point* d_map_points, int n_points, const uint8_t* d_outlier, int n_frames,
                                int only_tracking, int stereo, int32_t* d_frame_points, int32_t* d_ninliers, void* hip_stream)
{
    if (!t || !d_outlier || !d_frame_points || !d_ninliers || (n_points > 0 && !d_map_points)) return fail(IVF_E_INVALID, "null argument");
    if (n_points < 0) return fail(IVF_E_INVALID, "n_points must be >= 0");
    if (((size_t)d_map_points & 15) != 0) return fail(IVF_E_INVALID, "the point array must be 16-byte aligned");
    if (n_frames == 0) return IVF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = tracker_begin(t, false, 0, 0, n_frames, st);
    if (rc != IVF_OK) return rc;
    hipLaunchKernelGGL(k_close_local_map, dim3(n_frames), dim3(256), 0, st, t->P.nf, d_map_points, n_points, d_outlier, only_tracking, stereo,
                       d_frame_points, d_ninliers);
    return tracker_end(t, st);
}

}  // extern "C"
