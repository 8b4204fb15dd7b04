/*
 * ivfront.h -- flat C-ABI of the MI355X-native IV-SLAM visual front end (libivfront.so).
 *
 * The reference (ut-amrl/IV_SLAM) has no plugin/FFI layer for this path: its boundary is two C++
 * classes, ORB_SLAM2::ORBextractor (ORB/include/ORBextractor.h:51-126) and ORB_SLAM2::ORBmatcher
 * (ORB/include/ORBmatcher.h:37-108), plus Frame::ComputeStereoMatches (ORB/src/Frame.cc:758-932)
 * which reads ORBextractor::mvImagePyramid directly.  This header is the C-ABI a maintainer binds
 * BEHIND those class surfaces (see include/ivfront_orbslam.hpp and INTEGRATION.md); every entry
 * point names the reference interface it replaces.  ORB/ = introspective_ORB_SLAM/.
 *
 * Conventions: plain pointers and sizes only; caller-allocated outputs; every function returns an
 * int status (IVF_OK or a negative IVF_E_*), never throws; ivf_last_error() gives a thread-local
 * message.  One handle = one non-re-entrant instance (like one ORBextractor); different handles
 * may be used concurrently from different threads (ORB/src/Frame.cc:116-124 runs L/R on 2 threads).
 * All compute runs in hand-written HIP kernels on gfx950; there is NO CPU fallback: without a
 * usable GPU every compute entry point fails with IVF_E_NO_DEVICE.
 */
#ifndef IVFRONT_H
#define IVFRONT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVF_OK             0
#define IVF_E_INVALID     -1   /* bad argument */
#define IVF_E_CAPACITY    -2   /* caller buffer too small */
#define IVF_E_GEOMETRY    -3   /* cell grid leaves the image where the reference would throw / read OOB (with introspection: only without a cost map) */
#define IVF_E_NO_DEVICE   -4   /* no usable HIP device / HIP runtime error */
#define IVF_E_STATE       -5   /* call order violated (e.g. stereo match before extract) */

#define IVF_MAX_LEVELS 16

/* cv::KeyPoint subset produced by ORBextractor::operator() (ORB/src/ORBextractor.cc:1155-1156,1286-1294) */
typedef struct ivf_keypoint {
    float x, y;        /* pt, level-0 coordinates (level coords * mvScaleFactor[octave]) */
    float size;        /* (int)(31 * mvScaleFactor[octave]) */
    float angle;       /* degrees, [0,360) */
    float response;    /* FAST score, times the quality factor when introspection is active */
    int32_t octave;
} ivf_keypoint;

/* ORBextractor constructor arguments (ORB/include/ORBextractor.h:57-58, ORB/src/ORBextractor.cc:411-415) */
typedef struct ivf_extractor_params {
    int32_t nfeatures;
    float   scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    int32_t enable_introspection;   /* bool enableIntrospection */
} ivf_extractor_params;

typedef struct ivf_extractor ivf_extractor;   /* one ORB_SLAM2::ORBextractor */
typedef struct ivf_frontend  ivf_frontend;    /* batched, device-resident stereo front end */

/* ---- library ---- */
int         ivf_version(void);
const char* ivf_last_error(void);
int         ivf_device_count(void);                 /* number of visible HIP devices (0 if none) */
long long   ivf_debug_launch_count(void);           /* measurement aid: kernel launches this process has issued through the library */
/* Build provenance: the first 16 hex digits of sha256 over iv_slam_amd/csrc/{*.hip sorted, *.h sorted} and include/{* sorted},
 * taken when the library was linked (iv_slam_amd/csrc/Makefile).  iv_slam_amd/_lib.py recomputes it from the sources next to
 * the library and refuses to load a library built from anything else: a stale .so cannot produce a test result or a bench line.
 * r05: the hash also covers the build's variant flags, returned by ivf_build_flags() -- "" for the product, "-DIVF_EXPERIMENT" for the
 * experiment build (make EXPERIMENT=1 -> libivfront_exp.so: the kernel-variant selectors of the experiments in DESIGN.md exist only
 * there), any EXTRA=-D... of a one-off build: a differently compiled library cannot pass as the measured one. */
const char* ivf_build_id(void);
const char* ivf_build_flags(void);
/* Diagnostic: number of per-thread scratch slots (device + pinned host buffers of the per-call entry points) the process has
 * ever created.  Slots are leased by a thread and handed back when it exits, so the count follows the peak number of
 * CONCURRENT caller threads, not the number of threads ever started (ORB/src/Frame.cc:116-124 starts two per frame). */
int         ivf_debug_scratch_slots(void);

/* ---- ORBextractor ---- */
/* ORBextractor::ORBextractor (ORB/src/ORBextractor.cc:411-476); constructed in Tracking (ORB/src/Tracking.cc:174-191) */
int  ivf_extractor_create(const ivf_extractor_params* params, int device_id, ivf_extractor** out);
/* ~ORBextractor / Tracking::Release (ORB/src/Tracking.cc:2617-2626) */
void ivf_extractor_destroy(ivf_extractor* e);
/* GetLevels / GetScaleFactor (ORB/include/ORBextractor.h:69-73) */
int  ivf_extractor_get_levels(const ivf_extractor* e);
float ivf_extractor_get_scale_factor(const ivf_extractor* e);
/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (ORB/include/ORBextractor.h:75-89); each array has nlevels entries; any pointer may be NULL */
int  ivf_extractor_get_scale_tables(const ivf_extractor* e, float* scale, float* inv_scale,
                                    float* sigma2, float* inv_sigma2);
/* OpenCV-version switches for the three primitives whose arithmetic differs between OpenCV releases (the reference
 * accepts 2.4.3 ... 4.x, ORB/CMakeLists.txt:37-46, and pins none).  0 = OpenCV >= 3.4.2 / 4.x, the default everywhere.
 *   blur        1: cv::GaussianBlur 8U coefficients cvRound(k*256) = [18,34,49,55,49,34,18] (<= 3.4.1; saturating) (:1277)
 *   retain_best 1: KeyPointsFilter::retainBest calls nth_element(begin, begin + n, end) instead of begin + n - 1 (2.4 / 3.x) (:1146,:1164)
 *   atan2       1: cv::fastAtan2 = x*y/(x^2 + 0.28 y^2) in double (<= 2.4.3) instead of the degree-7 polynomial (:104)
 * Takes effect from the next extraction / run on the handle. */
int  ivf_extractor_set_opencv_variant(ivf_extractor* e, int blur, int retain_best, int atan2);
int  ivf_frontend_set_opencv_variant(ivf_frontend* fe, int blur, int retain_best, int atan2);
/* mnFeaturesPerLevel (ORB/src/ORBextractor.cc:438-452) and umax (:458-475), for tests */
int  ivf_extractor_get_feature_tables(const ivf_extractor* e, int32_t* features_per_level, int32_t* umax16);
/* ORBextractor::operator()(image, mask, keypoints, descriptors) (ORB/src/ORBextractor.cc:1224-1296).
 * image: 8-bit grey, host memory.  cost: the `mask` argument = u8 cost map of the same size, or NULL
 * (used only when the handle was created with enable_introspection, as in :1231-1238).
 * kps[cap], desc[cap*32] caller-allocated; *n_out = number written.  Empty image -> IVF_OK, *n_out = 0. */
int  ivf_extract(ivf_extractor* e, const uint8_t* image, int width, int height, int stride,
                 const uint8_t* cost, int cost_stride,
                 ivf_keypoint* kps, uint8_t* desc, int cap, int* n_out);
/* mvImagePyramid[level] / mvQualityImagePyramid[level] (ORB/include/ORBextractor.h:91-92): copies the
 * un-padded level of the LAST ivf_extract into dst (rows of dst_stride bytes); dst may be NULL to query size. */
int  ivf_extractor_pyramid_level(const ivf_extractor* e, int level, uint8_t* dst, int dst_stride, int* width, int* height);
int  ivf_extractor_quality_level(const ivf_extractor* e, int level, uint8_t* dst, int dst_stride, int* width, int* height);
/* The 7x7 sigma-2 blurred copy of mvImagePyramid[level] that the descriptors of the LAST ivf_extract were sampled from
 * (the local `workingMat` of ORB/src/ORBextractor.cc:1276-1277; the reference does not keep it).  Diagnostic / parity
 * tests only; like the reference, levels without keypoints are not blurred (IVF_E_STATE for those). */
int  ivf_extractor_blur_level(const ivf_extractor* e, int level, uint8_t* dst, int dst_stride, int* width, int* height);
/* keypoints per level of the last call (allKeypoints[level].size(), ORB/src/ORBextractor.cc:1253-1254) */
int  ivf_extractor_level_counts(const ivf_extractor* e, int32_t* counts);

/* ---- Frame::ComputeStereoMatches (ORB/src/Frame.cc:758-932) ----
 * Uses the pyramids held by the two extractor handles from their last ivf_extract (as the reference
 * reads mpORBextractorLeft/Right->mvImagePyramid, :765,855,867,872).  bf = mbf, b = mb.
 * u_right[nL], depth[nL] receive mvuRight / mvDepth (-1 = no match). */
int  ivf_stereo_match(const ivf_extractor* left, const ivf_extractor* right,
                      const ivf_keypoint* kps_left, int n_left, const uint8_t* desc_left,
                      const ivf_keypoint* kps_right, int n_right, const uint8_t* desc_right,
                      float bf, float b, float* u_right, float* depth);

/* ---- ORBmatcher ---- */
/* ORBmatcher::DescriptorDistance (ORB/src/ORBmatcher.cc:1700-1716); host helper, 32-byte rows */
int  ivf_hamming(const uint8_t* a, const uint8_t* b);
/* dist[i] = DescriptorDistance(desc_a[pairs[2i]], desc_b[pairs[2i+1]]) on the device */
int  ivf_hamming_pairs(const uint8_t* desc_a, int n_a, const uint8_t* desc_b, int n_b,
                       const int32_t* pairs, int n_pairs, int32_t* dist, int device_id);

typedef struct ivf_bounds { float min_x, min_y, max_x, max_y; } ivf_bounds;   /* Frame::mnMinX.. (ORB/src/Frame.cc:724-756) */
/* Frame::GetFeaturesInArea on Frame::mGrid (ORB/src/Frame.cc:415-430, 615-680): host helper that
 * returns indices in the reference's cell-major order; *n_out may exceed cap (IVF_E_CAPACITY). */
int  ivf_features_in_area(const ivf_keypoint* kps, int n, const ivf_bounds* bounds,
                          float x, float y, float r, int min_level, int max_level,
                          int32_t* out, int cap, int* n_out);
/* ---- Frame::UndistortKeyPoints / Frame::ComputeImageBounds (ORB/src/Frame.cc:696-726, :728-756) ----
 * Both are cv::undistortPoints(src, dst, mK, mDistCoef, cv::Mat(), mK) (:714, :740) as OpenCV 4.x's plain C++ path computes it
 * (DESIGN.md A-14): IEEE double throughout, EXACTLY five fixed-point iterations (TermCriteria(MAX_ITER, 5, 0.01): the count only,
 * converged or not), float result.  mK and mDistCoef are CV_32F (ORB/src/Tracking.cc:106-123), hence float here.
 * dist = k1,k2,p1,p2[,k3[,k4,k5,k6[,s1,s2,s3,s4]]]; n_dist 0, 4, 5, 8 or 12 as ivf_init_undistort_rectify_map accepts (tilt terms
 * unsupported), anything else IVF_E_INVALID.  Like the reference, only k1 switches the undistortion on: with n_dist == 0 or
 * dist[0] == 0 the keypoints are copied and the bounds are (0, 0, width, height), whatever the other coefficients say (:698-702, :730). */
typedef struct ivf_camera { float fx, fy, cx, cy; float dist[12]; int32_t n_dist; } ivf_camera;
/* Frame::ComputeImageBounds (Frame.cc:728-756): the four image corners (0,0), (width,0), (0,height), (width,height) undistorted;
 * min_x = min(p0.x, p2.x), max_x = max(p1.x, p3.x), min_y = min(p0.y, p1.y), max_y = max(p2.y, p3.y).  Host only: needs no device. */
int  ivf_image_bounds(const ivf_camera* cam, int width, int height, ivf_bounds* out);
/* Frame::UndistortKeyPoints (Frame.cc:696-726) for one frame, host buffers, computed on the device: out[i] = kps[i] with pt
 * undistorted; size, angle, response, octave are copied (:721-724).  out may alias kps; n == 0 is fine. */
int  ivf_undistort_keypoints(const ivf_camera* cam, const ivf_keypoint* kps, int n, ivf_keypoint* out, int device_id);
/* Frame::UndistortKeyPoints (Frame.cc:696-726) for n_frames frames in device memory: d_kps / d_out [n_frames][cap], d_count
 * [n_frames] as the front end lays them out; slots at or past a frame's count are not written; d_out may be d_kps.  One kernel
 * launch on hip_stream (hipStream_t, NULL = default stream), asynchronous; a camera that does not undistort copies the keypoints below each count. */
int  ivf_undistort_keypoints_device(const ivf_camera* cam, const ivf_keypoint* d_kps, const int32_t* d_count, int n_frames, int cap,
                                    ivf_keypoint* d_out, void* hip_stream);

/* ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (ORB/src/ORBmatcher.cc:1372-1518)
 * on flat, already-projected queries (one per last-frame map point that passed :1399-1421):
 *   q_u,q_v  projection (:1416-1417); q_ur = u - mbf*invzc (:1453); q_radius = th*mvScaleFactors[oct] (:1427);
 *   q_min_level,q_max_level = GetFeaturesInArea level args chosen at :1429-1434; q_angle = LastFrame.mvKeysUn[i].angle;
 *   q_desc = pMP->GetDescriptor() (32 B each); q_valid (nullable) 0 = skip; q_blocks (nullable, default 1) =
 *   pMP->Observations()>0.  cur_assign[n_cur] in/out: -1 free, -2 occupied by a blocking map point,
 *   >=0 index of the query matched (CurrentFrame.mvpMapPoints).  Window Hamming distances are computed on
 *   the device; the order-dependent greedy assignment (:1447-1472) and rotation histogram (:1475-1511) are
 *   replayed in the reference's order. */
int  ivf_search_by_projection(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, const float* cur_uright, int n_cur,
                              const ivf_bounds* bounds,
                              int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                              const int32_t* q_min_level, const int32_t* q_max_level,
                              const float* q_angle, const uint8_t* q_desc,
                              const uint8_t* q_valid, const uint8_t* q_blocks,
                              int check_orientation, int32_t* cur_assign, int* nmatches, int device_id);

/* Same search; additionally cur_removed[n_cur] (nullable) = 1 where a keypoint was matched in this call and then dropped by
 * the rotation-consistency filter: the reference sets such an entry of mvpMapPoints to NULL (:1504) even if it held a map
 * point without observations before the call, which cur_assign == -1 alone cannot tell from "never touched". */
int  ivf_search_by_projection_ex(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, const float* cur_uright, int n_cur,
                                 const ivf_bounds* bounds,
                                 int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                                 const int32_t* q_min_level, const int32_t* q_max_level,
                                 const float* q_angle, const uint8_t* q_desc,
                                 const uint8_t* q_valid, const uint8_t* q_blocks,
                                 int check_orientation, int32_t* cur_assign, uint8_t* cur_removed, int* nmatches, int device_id);

/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th) (ORB/src/ORBmatcher.cc:45-135; called
 * from Tracking::SearchLocalPoints, ORB/src/Tracking.cc:2124-2130) on flat queries, one per map point with
 * mbTrackInView && !isBad():  q_u,q_v = mTrackProjX/Y; q_ur = mTrackProjXR; q_radius = r * mvScaleFactors[level] with
 * r = RadiusByViewingCos(mTrackViewCos) (2.5 if viewCos > 0.998 else 4.0), times th when th != 1 (:63-70);
 * q_level = mnTrackScaleLevel (window levels [level-1, level]); nn_ratio = mfNNratio.  Best / second best with the
 * ratio test only when both are in the same octave (:117-121).  cur_assign / q_valid / q_blocks as above. */
int  ivf_search_map_points(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, const float* cur_uright, int n_cur,
                           const ivf_bounds* bounds, int n_q, const float* q_u, const float* q_v, const float* q_ur,
                           const float* q_radius, const int32_t* q_level, const uint8_t* q_desc,
                           const uint8_t* q_valid, const uint8_t* q_blocks, float nn_ratio,
                           int32_t* cur_assign, int* nmatches, int device_id);

/* ORBmatcher::UpdateQualityScores(Frame &F) (ORB/src/ORBmatcher.cc:1108-1121; active only with
 * --ivslam_propagate_keyptqual, ORB/src/ORBmatcher.cc:130,1513,1647).  assign[i] = map-point index of keypoint i or -1
 * (F.mvpMapPoints); kp_quality = F.mvKeyQualScore (in/out); mp_quality = MapPoint quality scores (in/out).  Host-side
 * bookkeeping: sequential by definition (later keypoints see earlier updates). */
int  ivf_update_quality_scores(const int32_t* assign, int n, float* kp_quality, float* mp_quality, int n_map_points);

/* ---- testing hook ----
 * Runs the device's cv::KeyPointsFilter::retainBest core (the wave-cooperative replay of libstdc++ std::nth_element
 * used by the keypoint selection kernels) on caller-supplied non-negative responses: order_out[i] = index of the
 * element that ends at position i after nth_element(begin, begin+n_points-1, end, response-greater).  1 <= n <= 65536.
 * Up to 4096 elements the lists live in LDS, as in the kernels' common tiers.  Above, they live in the calling thread's device
 * scratch and both global-memory forms run on copies of the same keys: the wave-cooperative replay (order_out) and the
 * one-thread sequential replay; IVF_E_STATE if their orders differ anywhere. */
int  ivf_test_retain_best(const float* responses, int n, int n_points, int32_t* order_out, int device_id);

/* ---- batched device-resident stereo front end (throughput path; one per GPU) ----
 * Equivalent to, for each pair: left/right ORBextractor::operator() (ORB/src/Frame.cc:115-125),
 * mvKeyQualScore (ORB/src/Frame.cc:130-143) and Frame::ComputeStereoMatches (:758-932), for up to
 * max_pairs pairs per call with all inputs/outputs resident in HBM. */
typedef struct ivf_frontend_config {
    ivf_extractor_params left, right;   /* Tracking builds the right extractor with introspection off (ORB/src/Tracking.cc:182-183) */
    int32_t width, height;              /* fixed image size */
    int32_t max_pairs;                  /* batch capacity */
    float   bf, b;                      /* Frame::mbf, Frame::mb */
    int32_t device_id;
} ivf_frontend_config;

/* Threads and streams (r05 / r06): a handle may be used from any thread, one call at a time; different handles may be used from different threads
 * at once.  But every front end of a process on ONE device runs its batches on the same three internal streams (a per-device pool, created once,
 * never destroyed -- six more streams for a second front end cost the first one a quarter of its throughput on this runtime): two front ends on
 * one device are executed IN TURN, not side by side, and they are coupled through those streams:
 *   - ivf_frontend_sync(A) also waits for what B has enqueued so far;
 *   - work a caller puts on ivf_frontend_batch_stream(A) (a collective, the tracker step) sits in front of B's next batches too -- a slow peer
 *     in A's all-gather stalls an unrelated front end, e.g. the second camera of a rig.  Keep such work short, or run it on a stream of your own
 *     behind ivf_frontend_pack_gather_block_of(..., your_stream) (see IVF_STREAM_OF_BATCH below);
 *   - ivf_frontend_destroy(A) waits for A's own batches only (their completion events); finish what you enqueued behind them on a lent
 *     stream before destroying the handle.
 * Front ends on different devices share nothing. */
int  ivf_frontend_create(const ivf_frontend_config* cfg, ivf_frontend** out);
void ivf_frontend_destroy(ivf_frontend* fe);
/* Enqueue one batch; asynchronous.  The batch is ordered after everything already enqueued on `hip_stream`
 * (a hipStream_t, NULL = default stream; it produced the inputs) and runs on one of the front end's three internal
 * streams, so consecutive batches overlap; `hip_stream` itself only waits until the inputs have been ingested
 * (the caller may overwrite them in stream order right after this call).  Results of a run stay valid until two
 * further runs have been enqueued.  Use ivf_frontend_sync / ivf_frontend_fetch / ivf_frontend_pack_gather_block to consume.
 * d_left/d_right: device pointers to n_pairs grey images, image i at base + i*image_stride, rows of row_stride bytes.
 * d_cost: device pointer to n_pairs u8 cost maps (same layout) or NULL. */
int  ivf_frontend_run(ivf_frontend* fe, const uint8_t* d_left, const uint8_t* d_right, const uint8_t* d_cost,
                      size_t image_stride, int row_stride, int n_pairs, void* hip_stream);
/* The same with the grey conversion in front of the extractor fused into the ingest (r06): Tracking::GrabImageStereo converts a 3-channel image with
 * cvtColor(mImGray, mImGray, CV_RGB2GRAY or CV_BGR2GRAY) by mbRGB = Camera.RGB (ORB/src/Tracking.cc:272-295; the right image likewise, :296-311).
 * A side is IVF_COLOR_GRAY (8UC1 as in ivf_frontend_run), IVF_COLOR_BGR (8UC3, bytes B,G,R: what cv::imread gives; CV_BGR2GRAY) or IVF_COLOR_RGB
 * (bytes R,G,B; CV_RGB2GRAY), each side with its own strides (bytes).  cv::cvtColor on 8-bit data is fixed point; the coefficients are those of
 * OpenCV 4.x -- (9798 R + 19235 G + 3735 B + 2^14) >> 15 -- like every other OpenCV primitive of this library; OR IVF_COLOR_CV3 into a code for
 * OpenCV <= 3.x's (4899 R + 9617 G + 1868 B + 2^13) >> 14.  A PCIe-fed pipeline with the introspection FCN ships the left COLOUR image once (the FCN
 * reads the same buffer, ivf_fcn_forward_device) instead of the colour image and a grey copy of it.  d_cost / its strides as in ivf_frontend_run.
 * stereo_kitti.cc:494-495 swaps R and B of the FCN's input IN PLACE; without rectification that is the very buffer GrabImageStereo converts afterwards
 * (SURVEY Appendix D-9): a host that reproduces the reference there hands over the swapped buffer, i.e. the other byte-order code. */
#define IVF_COLOR_GRAY 0
#define IVF_COLOR_BGR  1
#define IVF_COLOR_RGB  2
#define IVF_COLOR_CV3  4
int  ivf_frontend_run_color(ivf_frontend* fe, const uint8_t* d_left, int left_code, size_t left_image_stride, int left_row_stride,
                            const uint8_t* d_right, int right_code, size_t right_image_stride, int right_row_stride,
                            const uint8_t* d_cost, size_t cost_image_stride, int cost_row_stride, int n_pairs, void* hip_stream);
/* Cost maps without a copy (r06).  ivf_frontend_run ingests the cost maps like the images: a copy into the pitched level-0 plane of the batch context
 * (the reference has no such step: extractor and FCN share one cv::Mat, stereo_kitti.cc:508-521 -> Tracking.cc).  A producer on the device -- the FCN --
 * can write there directly: ivf_frontend_cost_plane returns the plane of the context the NEXT ivf_frontend_run / _run_color of this handle will use
 * (pair i's map at d_plane + i * image_stride, rows of row_stride bytes, only the first `width` bytes of a row may be written) and makes hip_stream wait
 * until that context's previous batch is done with it; pass exactly this pointer and these strides as d_cost / cost strides to ivf_frontend_run_color
 * and the ingest of the cost maps is skipped.  ivf_fcn_forward_device_strided writes such a plane. */
int  ivf_frontend_cost_plane(ivf_frontend* fe, uint8_t** d_plane, size_t* image_stride, int* row_stride, void* hip_stream);
/* Block until every ivf_frontend_run on this handle has finished (and, the internal streams being shared per device, whatever other front ends of
 * the process have enqueued on that device so far); reports device-side consistency errors. */
int  ivf_frontend_sync(ivf_frontend* fe);
/* Device-resident results of the last run (valid until the next run).  side 0 = left, 1 = right.
 * d_kps: [max_pairs][cap] ivf_keypoint, d_desc: [max_pairs][cap][32], d_count: [max_pairs] int32, cap = nfeatures;
 * d_uright/d_depth/d_quality: [max_pairs][cap] float (left only).  Any out pointer may be NULL. */
int  ivf_frontend_device_results(const ivf_frontend* fe, int side, const ivf_keypoint** d_kps, const uint8_t** d_desc,
                                 const int32_t** d_count, const float** d_uright, const float** d_depth,
                                 const float** d_quality, int* cap);
/* Copy one pair's results to host (synchronises).  uright/depth/quality are left-only and may be NULL. */
int  ivf_frontend_fetch(ivf_frontend* fe, int pair, int side, ivf_keypoint* kps, uint8_t* desc, int cap, int* n_out,
                        float* uright, float* depth, float* quality);
/* Same for the run `age` runs back (0 = the last one ... 2 = the oldest one still held): results of a run stay valid until
 * two further runs have been enqueued, so a caller that keeps three batches in flight reads each of them this way. */
int  ivf_frontend_fetch_of(ivf_frontend* fe, int age, int pair, int side, ivf_keypoint* kps, uint8_t* desc, int cap, int* n_out,
                           float* uright, float* depth, float* quality);
/* Frame::UndistortKeyPoints inside the batch (the stereo constructor's call, ORB/src/Frame.cc:145, :696-726).  With a camera set,
 * every run from the next one on also produces mvKeysUn of the LEFT frames in its batch context, by one more kernel launch behind the
 * batch (no host synchronisation, no allocation per run; three contexts in flight like every other result).  Only the left keypoints
 * are undistorted: ComputeStereoMatches, the quality lookup and the descriptors keep using the distorted mvKeys (Frame.cc:130-146,
 * :758-932), so ivf_frontend_device_results / _fetch / _fetch_of return exactly what they return without a camera.  What changes:
 * ivf_frontend_undistorted / _fetch_undistorted below, the keypoint field of the gather records (ivf_frontend_pack_gather_block[_of])
 * and the grid of ivf_frame_create_from_frontend (side 0).  cam == NULL, or a camera that does not undistort (n_dist == 0 or
 * dist[0] == 0, Frame.cc:698-702), restores the behaviour of a handle that never had a camera.  The buffers are allocated by the
 * first call that sets an undistorting camera. */
int  ivf_frontend_set_camera(ivf_frontend* fe, const ivf_camera* cam);
/* mvKeysUn of the run `age` runs back (Frame.cc:696-726), device-resident and addressed like d_kps of ivf_frontend_device_results(side 0):
 * the LEFT frame of pair p at *d_kps_un + 2 * p * cap (the slots of the right frames in between are never written), counts = the left
 * counts d_count[2 * p].  Valid like the other results of that run.  IVF_E_STATE when that run had no undistorting camera: mvKeysUn == mvKeys then (ivf_frontend_device_results). */
int  ivf_frontend_undistorted(const ivf_frontend* fe, int age, const ivf_keypoint** d_kps_un);
/* mvKeysUn of one pair's left frame to the host (synchronises), Frame.cc:696-726; a run without an undistorting camera returns
 * mvKeys, as the reference does (:698-702). */
int  ivf_frontend_fetch_undistorted(ivf_frontend* fe, int age, int pair, ivf_keypoint* kps_un, int cap, int* n_out);
/* Elapsed milliseconds of the dominant kernel (FAST score + NMS) in the last run, from HIP events
 * recorded on the run's stream around that launch (bench.py's roofline leg); <0 if unavailable. */
float ivf_frontend_last_fast_ms(ivf_frontend* fe);
/* Same measurement summed over the last `last_n` runs (<= 64 are kept; last_n < 1 = all kept):
 * *sum_ms = total milliseconds, *n_out = number of launches summed.  Synchronises on those events. */
int   ivf_frontend_fast_ms_stats(ivf_frontend* fe, int last_n, double* sum_ms, int* n_out);
/* Pack this rank's results of the last run for a descriptor all-gather: writes into d_block (device)
 * n_pairs fixed-size records {int32 n; int32 pad[3]; ivf_keypoint kps[cap]; uint8 desc[cap][32]; float uright[cap];
 * float depth[cap]} (the LEFT frame of each pair: mvKeys, mDescriptors, mvuRight, mvDepth -- what a rank needs to run the
 * tracker's cross-frame search against a frame extracted elsewhere, ivf_tracker_run below) and returns the record size in
 * *record_bytes (= ivf_track_record_bytes(cap)).
 * With a camera set for that run (ivf_frontend_set_camera) the keypoint field holds mvKeysUn instead of mvKeys (Frame.cc:696-726).
 * The record layout and size do not change: the tracker step reads nothing but mvKeysUn, mvuRight, mvDepth and the descriptors from
 * a record (ORB/src/ORBmatcher.cc:1372-1518, :45-135; Frame::UnprojectStereo, Frame.cc:958-972), and mvuRight / mvDepth are those
 * of the distorted keypoints, as in the reference. */
int  ivf_frontend_pack_gather_block(ivf_frontend* fe, uint8_t* d_block, size_t block_bytes, size_t* record_bytes,
                                    void* hip_stream);
/* Same for the run `age` runs back (0 = the last one ... 2 = the oldest one still held).  Note that `hip_stream` waits
 * for that run to finish: pack on a stream of its own (bench.py does), not on the stream that feeds the next batch. */
int  ivf_frontend_pack_gather_block_of(ivf_frontend* fe, int age, uint8_t* d_block, size_t block_bytes, size_t* record_bytes,
                                       void* hip_stream);
/* hip_stream value for the two functions above: pack on the internal stream the batch itself ran on (in order behind it,
 * no cross-stream wait); ivf_frontend_batch_stream returns that stream (a hipStream_t) so that the consumer of the block
 * -- bench.py's all-gather -- can be enqueued behind the pack.
 * Ordering consequence (r04): the three internal streams are also LENT -- the 7x7 blur of the batch in context k runs on the internal
 * stream of context k + 1 (beside its own selection chain; IVF_NO_SIDE_BLUR=1 keeps it at home).  Work a caller puts on
 * batch_stream of batch n (a collective, the tracker step) therefore sits in front of the blur of batch n + 2 on that stream, and the
 * descriptors of batch n + 2 wait for that blur: a slow peer in the collective of batch n delays the extraction of batch n + 2 -- not
 * of batch n + 1.  Keep such work short (bench.py: pack + all-gather + tracker step, ~0.3 ms) or run it on a stream of your own behind
 * ivf_frontend_pack_gather_block_of(..., your_stream). */
#define IVF_STREAM_OF_BATCH ((void*)(intptr_t)-1)
void* ivf_frontend_batch_stream(ivf_frontend* fe, int age);

/* ---- batched, device-resident tracker step: the consumer of the all-gather -----------------------------------------------
 * For every (last, cur) pair of gather records, in ONE launch sequence and without leaving HBM: the matcher part of
 * Tracking::TrackWithMotionModel (ORB/src/Tracking.cc:1303-1330) =
 *   UpdateLastFrame's stereo points (Tracking.cc:1256-1300; Frame::UnprojectStereo, ORB/src/Frame.cc:958-972)
 *   -> ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono = false) (ORB/src/ORBmatcher.cc:1372-1518): projection,
 *      GetFeaturesInArea windows (ORB/src/Frame.cc:615-668), greedy assignment in last-keypoint order with the stereo check,
 *      rotation histogram + ComputeThreeMaxima (:1654-1695)
 *   -> the retry with th_retry when fewer than retry_below matches were found (Tracking.cc:1320-1330).
 * The keypoints of a record are mvKeysUn: for rectified stereo mvKeysUn == mvKeys (Frame.cc:698-702); for a lens-distorted camera
 * set it on the front end (ivf_frontend_set_camera: the records then carry the undistorted keypoints, Frame.cc:696-726) or undistort
 * hand-built records with ivf_undistort_keypoints_device, and take `bounds` from ivf_image_bounds (Frame.cc:728-756; min_x / min_y
 * may be negative). */
typedef struct ivf_track_config {
    int32_t nfeatures;                       /* capacity of a gather record (<= 4096) */
    int32_t nlevels;
    float   scale_factors[IVF_MAX_LEVELS];   /* mvScaleFactors (ivf_extractor_get_scale_tables) */
    float   fx, fy, cx, cy, bf, b;           /* Frame::fx, fy, cx, cy, mbf, mb */
    ivf_bounds bounds;                       /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    float   th;                              /* window factor: 7 for stereo, 15 otherwise (Tracking.cc:1313-1317), times the caller's multipliers */
    float   th_retry;                        /* 2 * th in the reference (Tracking.cc:1327) */
    int32_t retry_below;                     /* 20 (Tracking.cc:1320); 0 = never retry */
    int32_t check_orientation;               /* mbCheckOrientation of the matcher (true at Tracking.cc:1305) */
    float   th_depth;                        /* mThDepth: > 0 selects UpdateLastFrame's rule -- every stereo point closer than this and at
                                              * least the 100 closest, as new points WITHOUT observations (localization mode); <= 0: every
                                              * stereo point carries a point and points_block applies */
    int32_t points_block;                    /* default of pMP->Observations() > 0 (:1447-1449) when no flags are passed */
    int32_t max_pairs;                       /* (last, cur) pairs per call */
    int32_t device_id;
} ivf_track_config;
typedef struct ivf_tracker ivf_tracker;
size_t ivf_track_record_bytes(int nfeatures);
int  ivf_tracker_create(const ivf_track_config* cfg, ivf_tracker** out);
void ivf_tracker_destroy(ivf_tracker* t);
/* d_records: n_records gather records, record_bytes apart, 16-byte aligned (a packed block, or the all-gathered buffer);
 * d_pairs [n_pairs][2] int32 on the device = (last record, cur record) indices -- an index outside [0, n_records) gives that
 * pair d_nmatches = -1 and d_assign = -1 instead of a read outside the block;
 * d_poses [n_pairs][2][12] = for every PAIR {LastFrame.mTcw, CurrentFrame.mTcw} row-major 3x4 -- the optimised pose of the last
 * frame and the motion-model prior mVelocity * mLastFrame.mTcw of the current one (Tracking.cc:1311), so a frame that is "cur" in
 * one pair and "last" in the next carries a different pose in each, as in the reference -- or NULL = identity everywhere
 * (zero-motion prior);
 * d_point_flags [n_records][nfeatures] (nullable), per keypoint of a record when it is the LAST frame of a pair: bit 0 = the
 * keypoint carries a map point (0: it carries none, whatever its depth), bit 1 = that point has observations (it blocks the
 * current keypoint it takes, :1447-1449).  With flags th_depth is ignored; without them UpdateLastFrame's rule (th_depth > 0)
 * or "every stereo point" (th_depth <= 0) decides and points_block gives bit 1.
 * d_point_quality / d_key_quality [n_pairs][nfeatures] (both or neither; in/out): ORBmatcher::UpdateQualityScores(CurrentFrame)
 * (ORB/src/ORBmatcher.cc:1108-1121) as SearchByProjection runs it before returning under --ivslam_propagate_keyptqual
 * (:1513-1515), on the device: d_point_quality[p][i] = MapPoint::GetQualityScore() of the point last keypoint i carries,
 * d_key_quality[p][i2] = CurrentFrame.mvKeyQualScore[i2]; q = min of the two, the point's score is rewritten when it moves by
 * more than 0.01, the keypoint's always.  A retried pair is updated twice, like the two calls of Tracking.cc:1319-1328.
 * Outputs: d_assign [n_pairs][nfeatures] = for every keypoint of the current frame the index of the last-frame keypoint whose
 * point it received (CurrentFrame.mvpMapPoints) or -1; d_nmatches [n_pairs] = the return value.  Asynchronous on hip_stream.
 * The handle owns the scratch of ONE run: a run enqueued on a different stream than the previous one waits for it (an event);
 * use one tracker per stream to let runs overlap. */
int  ivf_tracker_run(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                     const float* d_poses, const uint8_t* d_point_flags, float* d_point_quality, float* d_key_quality,
                     int32_t* d_assign, int32_t* d_nmatches, void* hip_stream);

/* One local map point as Tracking::SearchLocalPoints (ORB/src/Tracking.cc:2088-2132) sees it.  80 bytes, 16-byte aligned arrays. */
typedef struct ivf_local_point {
    float   pos[3];                  /* MapPoint::GetWorldPos() */
    float   normal[3];               /* MapPoint::GetNormal() */
    float   min_distance;            /* mfMinDistance: the range test uses 0.8f * it (GetMinDistanceInvariance, MapPoint.cc:378-382) */
    float   max_distance;            /* mfMaxDistance: the range test uses 1.2f * it (:384-388), PredictScale the value itself (:412); > 0 */
    uint8_t desc[32];                /* GetDescriptor() */
    int32_t flags;                   /* bit 0: skip (isBad(), or mnLastFrameSeen == this frame: already matched, Tracking.cc:2114-2115);
                                      * bit 1: Observations() > 0 (a keypoint this point takes is skipped by later points, ORBmatcher.cc:87-89) */
    int32_t pad[3];
} ivf_local_point;
/* Batched Tracking::SearchLocalPoints, from the projection on: for frame slot f = record d_frames[f] with pose d_poses[f]
 * ([n_frames][12], row-major 3x4 Tcw after TrackWithMotionModel's optimisation; NULL = identity) and its local map points
 * d_points[d_point_offsets[f] .. d_point_offsets[f+1]) (at most max_points_per_frame are used): Frame::isInFrustum(pMP,
 * cos_limit = 0.5) (Frame.cc:557-613) incl. MapPoint::PredictScale (MapPoint.cc:407-422), then
 * ORBmatcher(nn_ratio).SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:45-135).  A record index outside [0, n_records)
 * or a decreasing / negative offset gives that frame d_nmatches = -1 and d_assign = -1.
 * d_occupied [n_frames][nfeatures] (nullable): 1 = the keypoint already holds a map point with observations (skipped, :87-89).
 * d_point_quality (indexed like d_points) / d_key_quality [n_frames][nfeatures] (both or neither; in/out): UpdateQualityScores(F)
 * (:128-132, :1108-1121) on the device for the keypoints that receive a point in THIS call; keypoints that held one before went
 * through the same update when they got it, and a second pass over them changes nothing (min(q_mp, q_kp) == q_kp by then).
 * Outputs: d_assign [n_frames][nfeatures] = index (within the frame's point range) of the map point each keypoint received in
 * THIS call or -1; d_nmatches [n_frames] = the return value (assignments made, replaced ones included).  n_frames <= max_pairs.
 * Asynchronous on hip_stream; shares the handle's scratch (and its one-call-at-a-time rule) with ivf_tracker_run.  A max_points_per_frame
 * beyond nfeatures enlarges that scratch; when the device refuses (IVF_E_NO_DEVICE) the handle stays usable with the scratch it had. */
int  ivf_tracker_search_local(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames,
                              int n_frames, const float* d_poses, const ivf_local_point* d_points, const int32_t* d_point_offsets,
                              int max_points_per_frame, const uint8_t* d_occupied, float th, float nn_ratio, float cos_limit,
                              float* d_point_quality, float* d_key_quality, int32_t* d_assign, int32_t* d_nmatches, void* hip_stream);

/* Batched Optimizer::PoseOptimization (ORB/src/Optimizer.cc:251-503), the call between the two searches: for frame slot f = record
 * d_frames[f], one 6-dof pose vertex and one unary edge per keypoint that holds a map point -- EdgeSE3ProjectXYZOnlyPose where
 * mvuRight < 0, EdgeStereoSE3ProjectXYZOnlyPose otherwise -- with information mvInvLevelSigma2[octave] (1.0f / (sf * sf) of
 * cfg.scale_factors, as the ORBextractor constructor derives it) and a Huber kernel of width deltaMono / deltaStereo TIMES THE MAP
 * POINT'S QUALITY SCORE (:315-320, :342, :380), optimised by g2o's Levenberg-Marquardt on the dense 6x6 system in n_rounds rounds of
 * at most 10 iterations; after every round the edges are re-classified against 5.991 / 7.815 (:423-490), the kernels are dropped after
 * round min(2, n_rounds - 2), and a frame with fewer than 10 edges stops after its first round (:492).  One HIP kernel, one workgroup
 * per frame, double arithmetic where the reference uses it; the sums over edges are taken in a fixed order (bit-identical re-runs).
 * d_xw [n_frames][nfeatures][3] = pMP->GetWorldPos() of the point keypoint i holds; d_has_point [n_frames][nfeatures] = mvpMapPoints[i]
 * != NULL (keypoints past the record's count are ignored); d_quality [n_frames][nfeatures] or NULL (= 1.0f) = the qual_score of
 * :315-320; n_rounds = FLAGS_optimizer_pose_opt_iter_count (default 4), 1..4.  The scores are expected in [0, 1].  They are not
 * clamped: a negative one gives its edge a negative weight once chi2 exceeds delta^2, H + lambda I stops being positive, solves fail
 * as g2o's would, and the call returns whatever pose and flags the reference's arithmetic gives on that input (in the tested case the
 * input pose and 0 inliers).  Non-finite arithmetic (a NaN, a point at z = 0 in the camera frame) cannot hang the call, every loop
 * has a compile-time bound, but its result is unspecified beyond that: the one tested case, a z = 0.0f point at the identity pose,
 * returns the pose unchanged with no outlier flagged.
 * d_poses [n_frames][12] in: pFrame->mTcw (row-major 3x4), out: the pose SetPose receives; d_outlier [n_frames][nfeatures] = mvbOutlier
 * (0 where there is no point); d_ninliers [n_frames] = the return value (0 with fewer than 3 correspondences: pose unchanged; -1 for a
 * record index outside [0, n_records): pose unchanged); d_chi2 [n_frames][nfeatures] (nullable) = mvChi2 as logging == true records it
 * in round n_rounds - 1, 0 where there is no point or that round did not run.  n_frames <= max_pairs.
 * Asynchronous on hip_stream; obeys the handle's one-call-at-a-time rule like the two searches. */
int  ivf_tracker_optimize_pose(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames, int n_frames,
                               const float* d_xw, const uint8_t* d_has_point, const float* d_quality, int n_rounds, float* d_poses,
                               uint8_t* d_outlier, int32_t* d_ninliers, float* d_chi2, void* hip_stream);
/* The inputs of ivf_tracker_optimize_pose from what the two searches wrote, without leaving the device.
 * from_pairs: after ivf_tracker_run on the same d_pairs / d_poses_pairs ([n_pairs][2][12] or NULL = identity): d_xw[p][i2] =
 * Frame::UnprojectStereo(d_assign[p][i2]) of the LAST record of pair p under its last pose (ORB/src/Frame.cc:958-972, the float / gemm
 * arithmetic ivf_tracker_run projects with), d_has_point[p][i2] = 1; 0 (and xw = 0) where d_assign is -1, the last keypoint has no
 * depth or the last record index is outside the block.  The frames to optimise are the pairs' cur records.
 * from_local: after ivf_tracker_search_local: d_xw[f][i] = d_points[d_point_offsets[f] + d_assign[f][i]].pos. */
int  ivf_tracker_points_from_pairs(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                                   const float* d_poses_pairs, const int32_t* d_assign, float* d_xw, uint8_t* d_has_point, void* hip_stream);
int  ivf_tracker_points_from_local(ivf_tracker* t, const ivf_local_point* d_points, const int32_t* d_point_offsets, const int32_t* d_assign,
                                   int n_frames, float* d_xw, uint8_t* d_has_point, void* hip_stream);

/* ---- introspection FCN forward (IF/networks/models_light/models_light.py:18-28; called at
 * ORB/Examples/Stereo/stereo_kitti.cc:231-247 (load) and :493-514 (pre-process, forward, u8 truncation)) ----
 * weights_blob: the model's state_dict f32 tensors in state_dict order, num_batches_tracked skipped
 * (tools/export_fcn_weights.py; 2,189,666 floats).  Input = BGR u8 image (what cv::imread returns), in_width x
 * in_height; output = cost map out_width x out_height (the reference sets out_size = image size because the
 * extractor builds the cost pyramid from the mask's own dimensions, ORB/src/ORBextractor.cc:1330-1331). */
typedef struct ivf_fcn ivf_fcn;
int  ivf_fcn_create(const float* weights_blob, size_t n_floats, int in_width, int in_height, int out_width, int out_height,
                    int max_batch, int device_id, ivf_fcn** out);
void ivf_fcn_destroy(ivf_fcn* f);
/* one image, host buffers: bgr rows of `stride` bytes; cost_u8 = (uint8)(cost*255) (truncation, :511), rows of
 * cost_stride bytes; cost_f32 (nullable) = the f32 map [out_height*out_width].  Either output may be NULL. */
int  ivf_fcn_forward(ivf_fcn* f, const uint8_t* bgr, int width, int height, int stride,
                     uint8_t* cost_u8, int cost_stride, float* cost_f32);
/* batch, device buffers: d_bgr = n interleaved BGR images (image i at base + i*image_stride, rows of row_stride
 * bytes); d_cost_u8 [n][out_h][out_w] and/or d_cost_f32 [n][out_h][out_w]; asynchronous on hip_stream. */
int  ivf_fcn_forward_device(ivf_fcn* f, const uint8_t* d_bgr, size_t image_stride, int row_stride, int n,
                            uint8_t* d_cost_u8, float* d_cost_f32, void* hip_stream);
/* the same with the u8 maps written through the caller's strides (r06): map i at d_cost_u8 + i * cost_image_stride, rows of cost_row_stride bytes
 * (>= out_width), e.g. the front end's own cost plane (ivf_frontend_cost_plane above) */
int  ivf_fcn_forward_device_strided(ivf_fcn* f, const uint8_t* d_bgr, size_t image_stride, int row_stride, int n,
                                    uint8_t* d_cost_u8, size_t cost_image_stride, int cost_row_stride, void* hip_stream);
/* Device-side flags of the handle (r05).  The convolutions run as split-f16 MFMA products (x = hi + lo in f16), exact to 22 bits
 * while |x| < 65504.  Weights are pre-scaled per output channel and every hidden tensor is bounded by ReLU6 (mobilenet.py:44-62); the
 * linear-bottleneck outputs are not, so the kernels that store them raise a flag when one reaches 65504 (libtorch's f32 convs,
 * stereo_kitti.cc:508, have no such limit: the reference would simply go on).  ivf_fcn_forward checks the flag itself and returns
 * IVF_E_STATE instead of a cost map; after ivf_fcn_forward_device call ivf_fcn_status(f, hip_stream): it waits for the stream, returns
 * IVF_E_STATE if any forward of this handle since the last check raised the flag, and clears it.  Non-finite weights are refused by
 * ivf_fcn_create (IVF_E_INVALID).  The kernels raise the flag in a word of the DEVICE and the last kernel of a forward moves it into the
 * handle: when two handles run forwards CONCURRENTLY on one device (different streams) handle A's overflow can be collected by handle B's
 * forward -- B then reports IVF_E_STATE and A reports IVF_OK for a wrong cost map.  The flag is never lost for the DEVICE, but it can be lost for
 * the handle that raised it: callers that overlap forwards of several handles on one device must treat IVF_E_STATE from ANY of them as
 * invalidating the forwards of ALL of them since their last checks (bench.py and the reference's one-network-per-process use a single handle). */
int  ivf_fcn_status(ivf_fcn* f, void* hip_stream);
/* The other stereo driver's call contract (Examples/Stereo/stereo_airsim.cc:386-411), which resizes in u8 around the network:
 * bgr (src_width x src_height) -> cv::resize INTER_LINEAR to the handle's in size (:389-390) -> forward (the module's interpolation to
 * 512x512 is the identity when in = 512x512) -> u8 map (cost*255 truncated, :409) at the handle's out size -> cv::resize INTER_LINEAR to
 * dst_width x dst_height (:410-411).  The rounding to u8 between the resizes and the network is the driver's: no combination of the calls
 * above reproduces it.  The handle owns the scratch (max_batch u8 inputs at the in size, max_batch u8 maps at the out size, allocated by the
 * first such call) and keeps the resize tables of the last (src, dst) geometry.  Input = BGR as for ivf_fcn_forward: the R/B swap of the
 * network's input happens inside (a resize treats the channels alike, so swap-then-resize equals resize-then-swap).  The driver's swap is
 * IN PLACE on imLeft (:386-387), which TrackStereo receives afterwards: that side effect is the caller's.
 * Host buffers: rows of `stride` / `cost_stride` bytes; checks the f16-range flag like ivf_fcn_forward (IVF_E_STATE, output not written). */
int  ivf_fcn_forward_resized(ivf_fcn* f, const uint8_t* bgr, int src_width, int src_height, int stride,
                             uint8_t* cost_u8, int dst_width, int dst_height, int cost_stride);
/* stereo_airsim.cc:386-411 for n <= max_batch device images (image i at d_bgr + i * image_stride, rows of row_stride bytes); map i at
 * d_cost_u8 + i * cost_image_stride, rows of cost_row_stride bytes -- e.g. ivf_frontend_cost_plane's plane.  Asynchronous on hip_stream;
 * check ivf_fcn_status afterwards like after ivf_fcn_forward_device. */
int  ivf_fcn_forward_device_resized(ivf_fcn* f, const uint8_t* d_bgr, int src_width, int src_height, size_t image_stride, int row_stride, int n,
                                    uint8_t* d_cost_u8, int dst_width, int dst_height, size_t cost_image_stride, int cost_row_stride,
                                    void* hip_stream);

/* ---- next rows of SURVEY section 8(f) ----
 * ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORB/src/ORBmatcher.cc:410-519):
 * kps1, desc1, kps2, desc2 = mvKeysUn and mDescriptors of the two frames, bounds2 = F2's (mnMinX, mnMinY, mnMaxX, mnMaxY);
 * prev_matched_xy [n1][2] in/out (vbPrevMatched), matches12 [n1] out (vnMatches12), *nmatches = return value.
 * nn_ratio / check_orientation = mfNNratio / mbCheckOrientation of the matcher. */
int  ivf_search_for_initialization(const ivf_keypoint* kps1, const uint8_t* desc1, int n1,
                                   const ivf_keypoint* kps2, const uint8_t* desc2, int n2, const ivf_bounds* bounds2,
                                   float* prev_matched_xy, int window_size, float nn_ratio, int check_orientation,
                                   int32_t* matches12, int* nmatches, int device_id);
/* ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (ORB/src/ORBmatcher.cc:296-404) on projected
 * candidates: the caller runs :318-365 (Sim3 transform, depth / IsInImage / distance-invariance / viewing-angle tests,
 * PredictScale) and passes per surviving point u, v, radius = th * mvScaleFactors[level], level = nPredictedLevel and
 * the map point descriptor.  matched [n_kf] in/out: -1 = vpMatched[idx] is NULL, -2 = occupied on entry, on return
 * >= 0 = index of the query now matched there.  *nmatches = return value. */
int  ivf_search_keyframe_points(const ivf_keypoint* kf_kps, const uint8_t* kf_desc, int n_kf, const ivf_bounds* bounds,
                                int n_q, const float* q_u, const float* q_v, const float* q_radius, const int32_t* q_level,
                                const uint8_t* q_desc, const uint8_t* q_valid, int32_t* matched, int* nmatches, int device_id);
/* ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th) (ORB/src/ORBmatcher.cc:831-982): the matching core :893-955 on projected
 * map points (u, v, ur = u - bf*invz, radius, level as above); kf_uright = mvuRight, inv_level_sigma2 = mvInvLevelSigma2.
 * best_idx[i] = the keypoint to fuse query i with (-1: none within TH_LOW), best_dist[i] (nullable) its distance.  The
 * Replace / AddObservation bookkeeping (:958-977) stays with the caller, in query order.
 * inv_level_sigma2 == NULL selects the core of Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:983-1106), which
 * has no reprojection gate (kf_uright and q_ur may then be NULL as well). */
int  ivf_fuse_candidates(const ivf_keypoint* kf_kps, const uint8_t* kf_desc, const float* kf_uright, int n_kf,
                         const ivf_bounds* bounds, const float* inv_level_sigma2, int n_levels,
                         int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                         const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid,
                         int32_t* best_idx, int32_t* best_dist, int device_id);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORB/src/ORBmatcher.cc:1145-1254).  The caller
 * projects KF1's map points that are still unmatched into KF2 (:1193-1230) -> per keypoint slot i1 of KF1: q12_valid,
 * u, v, radius = th * mvScaleFactors[level], level = nPredictedLevel, the map point descriptor; and KF2's into KF1
 * (:1273-1310) -> q21_*.  matches12[i1] = keypoint index in KF2 when both directions agree (:1336-1349), else -1;
 * *nfound = return value.  (vpMatches12[i1] = vpMapPoints2[matches12[i1]] is the caller's last step.) */
int  ivf_search_by_sim3(const ivf_keypoint* kps1, const uint8_t* desc1, int n1, const ivf_bounds* bounds1,
                        const ivf_keypoint* kps2, const uint8_t* desc2, int n2, const ivf_bounds* bounds2,
                        const float* q12_u, const float* q12_v, const float* q12_radius, const int32_t* q12_level,
                        const uint8_t* q12_desc, const uint8_t* q12_valid,
                        const float* q21_u, const float* q21_v, const float* q21_radius, const int32_t* q21_level,
                        const uint8_t* q21_desc, const uint8_t* q21_valid, int32_t* matches12, int* nfound, int device_id);
/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame &F, vpMapPointMatches) (ORB/src/ORBmatcher.cc:165-294; used by
 * Tracking::TrackReferenceKeyFrame and Relocalization).  DBoW2::FeatureVector of each side in CSR form: *_node[k] the
 * node ids in std::map (ascending) order, *_idx[*_start[k] .. *_start[k+1]) the feature indices of node k.
 * kf_has_map_point[i] = vpMapPointsKF[i] && !isBad().  kf_kps = pKF->mvKeysUn, f_kps = F.mvKeys (angles only).
 * f_match[iF] = index i of the keyframe keypoint whose map point F's keypoint iF receives (vpMapPointMatches[iF] =
 * vpMapPointsKF[i]) or -1; *nmatches = return value. */
int  ivf_search_by_bow(const ivf_keypoint* kf_kps, const uint8_t* kf_desc, const uint8_t* kf_has_map_point, int n_kf,
                       const int32_t* kf_node, const int32_t* kf_start, const int32_t* kf_idx, int kf_nodes,
                       const ivf_keypoint* f_kps, const uint8_t* f_desc, int n_f,
                       const int32_t* f_node, const int32_t* f_start, const int32_t* f_idx, int f_nodes,
                       float nn_ratio, int check_orientation, int32_t* f_match, int* nmatches, int device_id);
/* ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (ORB/src/ORBmatcher.cc:528-661, loop closing):
 * same CSR feature vectors; has_map_point* = vpMapPoints*[i] && !isBad().  matches12[idx1] = idx2 (vpMatches12[idx1] =
 * vpMapPoints2[idx2]) or -1; acceptance is bestDist1 < TH_LOW (strict) here; *nmatches = return value. */
int  ivf_search_by_bow_keyframes(const ivf_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_map_point1, int n1,
                                 const int32_t* node1, const int32_t* start1, const int32_t* idx1, int nodes1,
                                 const ivf_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_map_point2, int n2,
                                 const int32_t* node2, const int32_t* start2, const int32_t* idx2, int nodes2,
                                 float nn_ratio, int check_orientation, int32_t* matches12, int* nmatches, int device_id);
/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORB/src/ORBmatcher.cc:663-829, local
 * mapping's CreateNewMapPoints) including CheckDistEpipolarLine (:146-163).  has_map_point* = GetMapPoint(i) != NULL,
 * stereo* = mvuRight[i] >= 0; F12 row-major 3x3 f32; (ex, ey) = epipole of camera 1 in image 2 (:670-676);
 * scale_factors2 / level_sigma2_2 = pKF2->mvScaleFactors / mvLevelSigma2.  matches12[idx1] = idx2 or -1 (vMatchedPairs =
 * the pairs with matches12 >= 0 in ascending idx1, :815-823); *nmatches = return value. */
int  ivf_search_for_triangulation(const ivf_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_map_point1, const uint8_t* stereo1, int n1,
                                  const int32_t* node1, const int32_t* start1, const int32_t* idx1, int nodes1,
                                  const ivf_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_map_point2, const uint8_t* stereo2, int n2,
                                  const int32_t* node2, const int32_t* start2, const int32_t* idx2, int nodes2,
                                  const float* F12, float ex, float ey, const float* scale_factors2, const float* level_sigma2_2, int n_levels,
                                  int only_stereo, int check_orientation, int32_t* matches12, int* nmatches, int device_id);
/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist)
 * (ORB/src/ORBmatcher.cc:1520-1652, Tracking::Relocalization) on the keyframe's projected map points (caller: :1543-1569):
 * per map point u, v, radius = th * mvScaleFactors[level], level = nPredictedLevel, q_angle = pKF->mvKeysUn[i].angle and
 * its descriptor.  cur_assign [n_cur] in/out: -1 = mvpMapPoints[i2] is NULL, -2 = occupied on entry, >= 0 = query index
 * matched there; orb_dist = ORBdist; *nmatches = return value.  (UpdateQualityScores at :1641: ivf_update_quality_scores.) */
int  ivf_search_by_projection_reloc(const ivf_keypoint* cur_kps, const uint8_t* cur_desc, int n_cur, const ivf_bounds* bounds,
                                    int n_q, const float* q_u, const float* q_v, const float* q_radius, const int32_t* q_level,
                                    const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid,
                                    int orb_dist, int check_orientation, int32_t* cur_assign, int* nmatches, int device_id);
/* ---- DBoW2 vocabulary: Frame::ComputeBoW / KeyFrame::ComputeBoW (ORB/src/Frame.cc:683-694, KeyFrame.cc:66-77) =
 * mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1259).
 * The tree is handed over once as flat arrays (node 0 = root; children of node i = child[child_start[i] ..
 * child_start[i+1]); node_desc [n_nodes][32]; node_word / node_weight = Node::word_id / Node::weight, read at leaves;
 * depth_L = m_L) and stays on the device. */
typedef struct ivf_vocabulary ivf_vocabulary;
int  ivf_vocabulary_create(int n_nodes, const int32_t* child_start, const int32_t* child, const uint8_t* node_desc,
                           const int32_t* node_word, const double* node_weight, int depth_L, int device_id, ivf_vocabulary** out);
void ivf_vocabulary_destroy(ivf_vocabulary* v);
/* per descriptor: word id, weight and the node at level L - levelsup (:1217-1259) */
int  ivf_bow_transform(const ivf_vocabulary* v, const uint8_t* desc, int n, int levelsup,
                       int32_t* word_id, int32_t* node_id, double* weight);
/* mBowVec (TF-IDF, L1-normalised; word ids ascending) and mFeatVec (CSR, node ids ascending: the form ivf_search_by_bow*
 * and ivf_search_for_triangulation take) from those results; *_cap = capacities (n is always enough), *_n = sizes. */
int  ivf_bow_vectors(const int32_t* word_id, const int32_t* node_id, const double* weight, int n,
                     int32_t* bow_word, double* bow_value, int bow_cap, int* bow_n,
                     int32_t* fv_node, int32_t* fv_start, int32_t* fv_idx, int fv_cap, int* fv_n);
/* Tracking::TrackReferenceKeyFrame's matcher part (ORB/src/Tracking.cc:1159-1176) for n_pairs (reference keyframe, current frame) pairs
 * of gather records, on the device from end to end: the fallback of a frame that ivf_tracker_run could not track (no velocity, or fewer
 * than 20 matches after the retry, Tracking.cc:556-577).  Frame::ComputeBoW (Tracking.cc:1168) is reduced to what the search reads:
 * mFeatVec of both records of every pair, i.e. the node at level L - levelsup of every keypoint (TemplatedVocabulary.h:1217-1259; a
 * keypoint whose word has weight 0 enters no node, :1157), node ids ascending, features ascending inside a node; mBowVec is not
 * computed.  Then ORBmatcher(nn_ratio, check_orientation).SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches)
 * (ORB/src/ORBmatcher.cc:165-294; the reference calls it with 0.7, true) and, when the quality arrays are given,
 * UpdateQualityScores(mCurrentFrame) (Tracking.cc:1174-1176).  Results are those of ivf_bow_transform + ivf_bow_vectors +
 * ivf_search_by_bow on the same data, bit for bit.
 * d_pairs [n_pairs][2] = (keyframe record, current record); d_select [n_pairs] (nullable): 0 leaves the pair out (d_assign = -1,
 * d_nmatches = -2) -- a mask a device-side comparison of ivf_tracker_run's d_nmatches produces without a sync; a record index outside
 * [0, n_records) gives -1 / -1.  d_point_flags [n_records][nfeatures] (nullable), bit 0 = the keypoint holds a live map point
 * (vpMapPointsKF[i] && !isBad(), :197-203); NULL: every keyframe keypoint with a stereo depth holds one (ivf_tracker_run's default
 * with th_depth <= 0).  Given flags decide alone: a keyframe's map points need no stereo depth, their positions come from
 * ivf_tracker_points_from_keyframe's d_kf_xw.  d_point_quality [n_pairs][nfeatures] (indexed by keyframe keypoint) and d_key_quality
 * [n_pairs][nfeatures] (by frame keypoint): both or neither, in/out.
 * d_assign [n_pairs][nfeatures]: the keyframe keypoint whose map point frame keypoint i receives, or -1; d_nmatches [n_pairs] = the
 * return value (the caller applies the < 15 rule of Tracking.cc:1172).  IVF_E_INVALID: a vocabulary on another device than the
 * tracker, levelsup < 0, n_pairs > max_pairs.  Asynchronous on hip_stream; the feature vectors live in scratch the handle allocated at
 * ivf_tracker_create, so the call obeys the handle's one-call-at-a-time rule like the other searches. */
int  ivf_tracker_search_by_bow(ivf_tracker* t, const ivf_vocabulary* voc, int levelsup,
                               const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                               const int32_t* d_select, const uint8_t* d_point_flags, float nn_ratio, int check_orientation,
                               float* d_point_quality, float* d_key_quality, int32_t* d_assign, int32_t* d_nmatches, void* hip_stream);
/* The third feeder of ivf_tracker_optimize_pose, after ivf_tracker_search_by_bow on the same d_pairs (Tracking.cc:1173: mvpMapPoints =
 * vpMapPointMatches): d_xw[p][i] = d_kf_xw[keyframe record of pair p][d_assign[p][i]], d_has_point[p][i] = 1; 0 (and xw = 0) where
 * d_assign is -1 or the keyframe record index is outside [0, n_records).  d_kf_xw [n_records][nfeatures][3] = GetWorldPos() of the map
 * point each keypoint of each record holds.  The frames to optimise are the pairs' current records.  Asynchronous on hip_stream. */
int  ivf_tracker_points_from_keyframe(ivf_tracker* t, const int32_t* d_pairs, int n_pairs, int n_records, const float* d_kf_xw,
                                      const int32_t* d_assign, float* d_xw, uint8_t* d_has_point, void* hip_stream);
/* Tracking::Relocalization after its first pose (ORB/src/Tracking.cc:2351-2404), for n_pairs (keyframe, lost frame) pairs of gather
 * records without leaving the device: ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
 * (ORB/src/ORBmatcher.cc:1520-1652; the reference calls it with (10, 100) at Tracking.cc:2375 and (3, 64) at :2391).  For every
 * keypoint i of the keyframe record, in order: skipped when it holds no point, a bad one or a found one (:1541-1543); x3Dc = Rcw * xw +
 * tcw, u = fx * xc * invzc + cx with invzc = 1.0 / zc narrowed to float and NO test on the sign of zc (:1547-1554: a point behind the
 * camera whose projection lands inside the image is searched for); the four bounds (:1556-1559); dist3D = |xw - Ow| inside
 * [0.8f * min_distance, 1.2f * max_distance] (:1562-1570); MapPoint::PredictScale (MapPoint.cc:407-422); the window of radius
 * th * scale[level] on levels [level - 1, level + 1] (:1575-1577; level - 1 == -1 is GetFeaturesInArea's own rule, Frame.cc:615-668);
 * the FIRST minimum of the descriptor distance among the keypoints that hold no point (:1587-1602), accepted when <= orb_dist (:1604);
 * with check_orientation the 30-bin histogram of keyframe angle - frame angle and ComputeThreeMaxima (:1609-1645): keypoints of the other
 * bins are freed again after the walk; UpdateQualityScores(CurrentFrame) (:1647-1649) when the quality arrays are given.  Results equal
 * ivf_search_by_projection_reloc on the same data, bit for bit.
 * d_pairs [n_pairs][2] = (keyframe record, current record) and d_select [n_pairs] (nullable) as in ivf_tracker_search_by_bow, except
 * that a pair left out keeps its d_assign: d_select 0 gives d_nmatches = -2, a record index outside [0, n_records) gives -1.
 * d_poses [n_pairs][12] = CurrentFrame.mTcw (row-major 3x4), NULL = identity.  d_kf_points [n_records][nfeatures] (16-byte aligned) =
 * the map point each keypoint of each record holds: pos, min_distance, max_distance and desc (GetDescriptor()) are read, flags bit 0 =
 * no point / isBad(), normal is ignored; the angle is the keyframe record's own keypoint's.  pos must agree with the d_kf_xw that
 * ivf_tracker_points_from_keyframe reads, which turns d_assign into the solvers' d_xw / d_has_point after this call as after
 * ivf_tracker_search_by_bow.  d_found [n_pairs][nfeatures] by keyframe keypoint = sAlreadyFound; NULL = the keyframe keypoints present
 * in d_assign on entry (the rebuild of Tracking.cc:2386-2389).  d_assign [n_pairs][nfeatures], in/out: for each keypoint of the current
 * frame the keyframe keypoint whose point it holds, or -1; entries >= 0 on entry are occupied (:1590) and never change.  d_nmatches
 * [n_pairs] = the return value (nadditional).  d_point_quality (by keyframe keypoint) / d_key_quality (by frame keypoint), both
 * [n_pairs][nfeatures], both or neither, in/out: the update runs over every keypoint that holds a point on return; as in the reference,
 * where sAlreadyFound always contains what the frame holds, a point must not end on two keypoints (d_found covers d_assign's entries).
 * IVF_E_INVALID: orb_dist outside [0, 255] (at 256 the reference indexes with -1), th <= 0, n_pairs > max_pairs, a null required
 * pointer.  Every loop has a compile-time bound: a NaN pose cannot hang the call.  Asynchronous on hip_stream; uses the scratch of
 * ivf_tracker_search_local (grown to nfeatures queries per pair at the first call) and obeys the handle's one-call-at-a-time rule. */
int  ivf_tracker_search_reloc(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                              const int32_t* d_select, const float* d_poses, const ivf_local_point* d_kf_points, const uint8_t* d_found, float th,
                              int orb_dist, int check_orientation, float* d_point_quality, float* d_key_quality, int32_t* d_assign,
                              int32_t* d_nmatches, void* hip_stream);
/* The set bookkeeping around that search, on d_assign [n_frames][nfeatures] in place: d_assign[f][i] = -1 where
 * (d_mask[f][i] != 0) != keep_when_set (d_mask [n_frames][nfeatures], NULL = nothing is dropped); then, if d_found is given,
 * d_found[f][k] = 1 for every k still in d_assign[f], 0 elsewhere.  keep_when_set = 1 on ivf_tracker_solve_pnp's d_inlier with d_found =
 * sFound is Tracking.cc:2351-2361; keep_when_set = 0 on ivf_tracker_optimize_pose's d_outlier is :2368-2370 and :2398-2400.
 * n_frames <= max_pairs.  Asynchronous on hip_stream. */
int  ivf_tracker_filter_assign(ivf_tracker* t, int32_t* d_assign, int n_frames, const uint8_t* d_mask, int keep_when_set, uint8_t* d_found,
                               void* hip_stream);
/* The draws of the two RANSAC solvers below, ivf_tracker_solve_pnp (K = 4 points per sample) and ivf_tracker_solve_sim3 (K = 3).
 * d_draws [n][max_iterations][K], n = n_frames / n_pairs, max_iterations in [1, 300]: the values rand() returned for the K samples of
 * iteration it = mnIterations before its increment, each in [0, RAND_MAX = 2^31 - 1]; bit 31 is ignored.  The call applies the
 * reference's sampling to them: vAvailableIndices = mvAllIndices (0 .. N - 1), then K times randi = DUtils::Random::RandomInt(0, size - 1)
 * = (int)((double)r / 2^31 * size) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50), sample vAvailableIndices[randi], overwrite that position
 * with the back and drop the back.  The sampling is therefore the caller's: reproducible (iv_slam_amd.track.ransac_draws), or glibc's
 * stream to follow the reference exactly. */
/* Batched PnPsolver (ORB/src/PnPsolver.cc), the step of Tracking::Relocalization (ORB/src/Tracking.cc:2272-2421) between
 * SearchByBoW(pKF, mCurrentFrame, ...) and PoseOptimization: EPnP inside a RANSAC loop, in double as the reference runs it, for frame
 * slot f = record d_frames[f].  The correspondences are those the constructor collects (PnPsolver.cc:71-114): mvKeysUn[i] and
 * mvLevelSigma2[octave] (scale factor squared, in float) of every keypoint i below the record's count with d_has_point[f][i] != 0, and
 * d_xw[f][i] (both arrays as ivf_tracker_points_from_keyframe writes and ivf_tracker_optimize_pose takes them), in keypoint order.
 * probability, min_inliers, epsilon, th2 are SetRansacParameters' (Tracking.cc:2317: 0.99, 10, 0.5, 5.991; minSet is 4): :137-156
 * give mRansacMinInliers and mRansacMaxIts = clamp(ceil(log(1 - p) / log(1 - eps^3)), 1, max_iterations), 1 when mRansacMinInliers == N.
 * A call runs iterate() to completion: because the loop condition of :186 is an OR, the iterate(5, ...) of Tracking.cc:2339 runs until
 * mnIterations reaches mRansacMaxIts unless Refine succeeds earlier, and so does this call (where mRansacMaxIts < 5 the reference's
 * first call goes on to 5 iterations; this one stops at mRansacMaxIts).  The hypotheses are independent, so all of them are computed at
 * once (one wave each) and the bookkeeping of :213-259 is replayed in iteration order: the first iteration whose Refine (:264-309, on
 * mvbBestInliers, accepted with MORE than mRansacMinInliers inliers) succeeds returns mRefinedTcw and mvbRefinedInliers; with none, the
 * best hypothesis and its inliers when it has at least mRansacMinInliers; else no pose.  CheckInliers (:312-343) keeps the reference's
 * float / double mix.  cvSVD, cvInvert and cvSolve(CV_SVD) are a cyclic Jacobi SVD with a fixed pair order and sweep cap: a 4-point
 * hypothesis leaves a four-dimensional null space whose basis rounding chooses, so the poses of single hypotheses are not comparable
 * between implementations (what they compute around that basis is: ivf_test_pnp_hypotheses below); Refine's pose is.
 * d_draws [n_frames][max_iterations][4]: the draws contract above with K = 4, the sampling of :192-205.
 * Outputs: d_poses [n_frames][12] (row-major 3x4, the f64 mRi / mti narrowed to float, :221-227 / :298-304) is written only where a
 * pose is returned; d_inlier [n_frames][nfeatures] = vbInliers by keypoint; d_ninliers [n_frames] = nInliers, 0 = cv::Mat() (also for
 * N < mRansacMinInliers, :177-181), -1 = record index outside [0, n_records): nothing else of that frame is written;
 * d_iterations [n_frames] (nullable) = mnIterations on return; d_hyp_poses [n_frames][max_iterations][12] and d_hyp_ninliers
 * [n_frames][max_iterations] (nullable) = pose (narrowed to float) and mnInliersi of every iteration below mRansacMaxIts, the others
 * untouched.  IVF_E_INVALID: a null required pointer, max_iterations outside [1, 300], probability outside (0, 1), epsilon outside
 * [0, 1], n_frames > max_pairs.  Every loop has a compile-time bound: NaN input cannot hang the call.  Two runs are bit-identical.
 * Asynchronous on hip_stream, no host synchronisation; the scratch is allocated at the first call for max_pairs frames and obeys the
 * handle's one-call-at-a-time rule. */
int  ivf_tracker_solve_pnp(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames, int n_frames,
                           const float* d_xw, const uint8_t* d_has_point, const uint32_t* d_draws, int max_iterations, double probability,
                           int min_inliers, float epsilon, float th2, float* d_poses, uint8_t* d_inlier, int32_t* d_ninliers,
                           int32_t* d_iterations, float* d_hyp_poses, int32_t* d_hyp_ninliers, void* hip_stream);
/* Testing hook: the hypotheses of ivf_tracker_solve_pnp with their intermediate values.  The inputs are those of that call; its first
 * two launches run (the correspondences with mRansacMaxIts, then one wave per hypothesis), the bookkeeping of :213-259 and Refine do
 * not.  d_hyp_poses and d_hyp_ninliers (both required here) receive what that call writes into them, to the bit.  d_taps
 * [n_frames][max_iterations][IVF_PNP_TAP_DOUBLES] receives one record of doubles per iteration below mRansacMaxIts, the others and the
 * frames with a bad record index are untouched: [0, 4) the sample, as indices into the frame's correspondences in the order drawn
 * (PnPsolver.cc:192-205); [4, 16) cws[4][3] (choose_control_points); [16, 64) the four vectors ut + 12 * (11 - i), i = 0 .. 3, of MtM
 * (:501-503); [64, 76) the singular values of MtM, descending; then per candidate c = 0, 1, 2 (find_betas_approx_1, _2, _3) at
 * 76 + 21 c: the betas before gauss_newton (4) and after it (4), R (9, row-major), t (3) and the reprojection error; [139] the
 * candidate chosen (:522-524).  IVF_E_INVALID as for ivf_tracker_solve_pnp, and for a null d_taps, d_hyp_poses or d_hyp_ninliers.
 * Asynchronous on hip_stream; the handle's one-call-at-a-time rule holds. */
#define IVF_PNP_TAP_DOUBLES 140
int  ivf_test_pnp_hypotheses(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_frames, int n_frames,
                             const float* d_xw, const uint8_t* d_has_point, const uint32_t* d_draws, int max_iterations, double probability,
                             int min_inliers, float epsilon, float th2, double* d_taps, float* d_hyp_poses, int32_t* d_hyp_ninliers,
                             void* hip_stream);
/* Batched Sim3Solver (ORB/src/Sim3Solver.cc), the step of LoopClosing::ComputeSim3 (ORB/src/LoopClosing.cc:279-306) between
 * SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]) and SearchBySim3: Horn's closed form on three 3D-3D correspondences inside a
 * RANSAC loop, for pair p = (KF1 = current keyframe record d_pairs[p][0], KF2 = candidate record d_pairs[p][1]).  d_select as in
 * ivf_tracker_search_by_bow; d_poses [n_records][12] = Tcw of every record (row-major 3x4) as ivf_tracker_create_map_points takes it;
 * d_kf_xw [n_records][nfeatures][3] = GetWorldPos() as ivf_tracker_points_from_keyframe takes it; d_point_flags
 * [n_records][nfeatures], bit 0 = the keypoint holds a live map point; d_match12 [n_pairs][nfeatures] = vpMatched12 as indices: the
 * KF2 keypoint whose point KF1 keypoint i1 is matched to, or -1 (the array ivf_tracker_search_by_bow_keyframes writes).
 * The constructor (Sim3Solver.cc:40-115): for i1 ascending below KF1's count a correspondence is collected when d_match12[p][i1] = i2
 * >= 0, i2 is below KF2's count and both keypoints hold a live point (:67-76); GetIndexInKeyFrame (:78-82) is taken to be i1 / i2, the
 * keypoint that holds the point.  mvX3Dc = Rcw * Xw + tcw per side (:97-101); mvnMaxError = 9.210 * mvLevelSigma2[octave] computed in
 * double and TRUNCATED to an integer, a vector<size_t> (:87-91): 9 at level 0, not 9.21; FromCameraToImage (:408-426) divides by z
 * without a test of its sign.  SetRansacParameters (:117-141) with (probability, min_inliers, max_iterations; LoopClosing.cc:280 passes
 * 0.99, 20, 300): epsilon = (float)min_inliers / N, mRansacMaxIts = clamp(ceil(log(1 - p) / log(1 - epsilon^3)), 1, max_iterations),
 * 1 when min_inliers == N.  iterate (:143-210): N < min_inliers returns nothing (:149-153; so does N < 3, where the reference has no
 * sample to draw); per iteration three DUtils::Random::RandomInt draws with the swap-with-back removal (:166-180), ComputeSim3
 * (:229-340), CheckInliers (:343-367: both reprojections, err = dist.dot(dist) compared as float against the integer bound); the best
 * is replaced on mnInliersi >= mnBestInliers (:186) and the call succeeds on mnInliersi > min_inliers, strictly (:195).  Only a success
 * returns a transform: the best failed hypothesis is not returned (:209).
 * One call runs from the state on entry to the first success or to mRansacMaxIts: the loop condition of :161 is an AND, and
 * LoopClosing.cc:291-346 goes on calling iterate(5, ...) on a solver whose OptimizeSim3 failed, so d_state [n_pairs][2] =
 * {mnIterations, mnBestInliers} is in/out (NULL: {0, 0}, nothing written back); a second call with the state the first one left
 * continues where the reference's next iterate would, with the draws of those iterations.  d_iterations lets a caller rebuild the
 * round-robin order over candidates: the winner is the smallest ceil(iterations / 5), then candidate order.
 * d_draws [n_pairs][max_iterations][3]: the draws contract above (before ivf_tracker_solve_pnp) with K = 3, the sampling of :166-180.
 * Arithmetic: cv::Mat CV_32F products, dot, norm and reduce accumulate in double and narrow once; M and N are float
 * matrices (:246-268); cv::eigen is a cyclic two-sided Jacobi in f64 with a fixed pair order and sweep cap, the vector of the largest
 * eigenvalue narrowed to float (its sign is arbitrary: q and -q give one R); atan2, norm and cv::Rodrigues (:281-287) in double,
 * narrowed once; ms12i = (float)(nom / den) (:297-311), 1.0f with fix_scale (:314); mT21i as :333-339 form it.  A degenerate sample
 * whose imaginary part vanishes gives NaN (:283), hence no inlier.
 * Outputs: d_sim3 [n_pairs][16] = mR12i (9, row-major), mt12i (3), ms12i, 3 zeros, written only on success; d_inlier
 * [n_pairs][nfeatures] = vbInliers by i1, cleared for every written pair; d_ninliers [n_pairs] = nInliers, 0 = cv::Mat(), -1 = a record
 * index outside [0, n_records), -2 = not selected: nothing else of such a pair is written; d_iterations [n_pairs] (nullable) =
 * mnIterations on return; d_hyp_sim3 [n_pairs][max_iterations][16] and d_hyp_ninliers [n_pairs][max_iterations] (nullable) = the
 * transform and mnInliersi of every iteration from mnIterations on entry to mRansacMaxIts (the hypotheses are independent and computed at
 * once, also those behind the success), the others untouched.  IVF_E_INVALID: a null required pointer,
 * max_iterations outside [1, 300], probability outside (0, 1), min_inliers < 0, n_pairs > max_pairs.  Every loop has a compile-time
 * bound: NaN input cannot hang the call.  Two runs are bit-identical.  Asynchronous on hip_stream, no host synchronisation; the
 * scratch is allocated at the first call for max_pairs pairs and obeys the handle's one-call-at-a-time rule. */
int  ivf_tracker_solve_sim3(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                            const int32_t* d_select, const float* d_poses, const float* d_kf_xw, const uint8_t* d_point_flags,
                            const int32_t* d_match12, const uint32_t* d_draws, int max_iterations, double probability, int min_inliers,
                            int fix_scale, int32_t* d_state, float* d_sim3, uint8_t* d_inlier, int32_t* d_ninliers, int32_t* d_iterations,
                            float* d_hyp_sim3, int32_t* d_hyp_ninliers, void* hip_stream);
/* The two searches around that solver in LoopClosing::ComputeSim3 (ORB/src/LoopClosing.cc:236-405), on the device: with them the chain
 * runs from a candidate pair of gather records to the full correspondence set of OptimizeSim3 without the host reading anything.  Both
 * take pair p = (KF1 = d_pairs[p][0], KF2 = d_pairs[p][1]) and d_select as ivf_tracker_search_by_bow does, except that a pair left out
 * is left alone: d_select 0 gives -2 in the count output, a record index outside [0, n_records) gives -1, and nothing else of such a pair
 * is written.  Asynchronous on hip_stream, one call of the handle at a time, no host synchronisation -- except in the first
 * ivf_tracker_search_by_sim3 of a handle, which enlarges the grid scratch and waits on the host for the handle's previous call first; every loop is bounded by nfeatures,
 * by the grid or by the node count, so a NaN pose or a NaN similarity cannot hang a launch; two runs are bit-identical.
 *
 * ivf_tracker_search_by_bow_keyframes: ORBmatcher(nn_ratio, check_orientation).SearchByBoW(pKF1, pKF2, vpMatches12)
 * (ORB/src/ORBmatcher.cc:528-661; LoopClosing.cc:270 calls it with 0.75, true).  The feature vectors of both records are computed in
 * the call as ivf_tracker_search_by_bow computes them (same descent, same sort, same scratch), and the search is that call's kernel body
 * with the differences of this overload: a KF2 candidate must itself hold a live point (:580-586); the occupancy is vbMatched2, by KF2
 * keypoint; the acceptance is bestDist1 < TH_LOW, strictly (:604); the histogram takes angle1 - angle2 (:613); a match the rotation
 * filter removes is cleared in vpMatches12 only (:654).  d_point_flags [n_records][nfeatures] (nullable), bit 0 = the keypoint holds a
 * live map point, read for both sides; NULL: every keypoint with a stereo depth holds one, on both sides.
 * d_match12 [n_pairs][nfeatures], by KF1 keypoint: the KF2 keypoint whose point it is matched to, or -1 -- the array
 * ivf_tracker_solve_sim3 reads; d_nmatches [n_pairs] = the return value.  Results equal ivf_bow_transform + ivf_bow_vectors +
 * ivf_search_by_bow_keyframes on the same data, bit for bit.  IVF_E_INVALID as ivf_tracker_search_by_bow. */
int  ivf_tracker_search_by_bow_keyframes(ivf_tracker* t, const ivf_vocabulary* voc, int levelsup,
                                         const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                                         const int32_t* d_select, const uint8_t* d_point_flags, float nn_ratio, int check_orientation,
                                         int32_t* d_match12, int32_t* d_nmatches, void* hip_stream);
/* ivf_tracker_search_by_sim3: ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORB/src/ORBmatcher.cc:1145-1369)
 * INCLUDING both projection loops, behind the inlier filter of LoopClosing.cc:318-323.  d_select: the caller derives it on the device
 * from ivf_tracker_solve_sim3's d_ninliers > 0 (d_sim3 is unwritten for a failed pair).  d_poses [n_records][12] as
 * ivf_tracker_solve_sim3 takes it; d_kf_points [n_records][nfeatures] (16-byte aligned) as ivf_tracker_search_reloc takes it: pos,
 * min_distance, max_distance and desc are read, flags bit 0 = no point / isBad(); d_sim3 [n_pairs][16] as ivf_tracker_solve_sim3 writes
 * it; d_match12 [n_pairs][nfeatures]; d_inlier [n_pairs][nfeatures] (nullable; NULL: every match is kept); th: the reference passes 7.5.
 * Per pair: vpMatches12[i1] = d_match12[p][i1] where d_inlier is set, else none; vbAlreadyMatched1 / 2 (:1175-1185) with
 * GetIndexInKeyFrame taken to be the keypoint index itself (as ivf_tracker_solve_sim3 does), an index outside KF2's count marks nothing
 * there.  Direction 1 -> 2 (:1191-1268), for every KF1 keypoint in this order: skipped without a point, with a bad one or an already
 * matched one; p3Dc1 = R1w * xw + t1w, p3Dc2 = sR21 * p3Dc1 + t21; skipped on z < 0.0 (a zero depth goes on: its infinite or NaN
 * projection fails the next test); invz = 1.0 / z in double, narrowed once; u = fx * (x * invz) + cx, v likewise, with the HANDLE's
 * intrinsics in both directions (the reference uses KF1's for both); KeyFrame::IsInImage (KeyFrame.cc:647-650): >= min and < max,
 * strictly; dist3D = cv::norm(p3Dc2), the camera-frame norm, inside [0.8f * min_distance, 1.2f * max_distance]; MapPoint::PredictScale;
 * radius = th * scale[level]; the window of KeyFrame::GetFeaturesInArea (KeyFrame.cc:606-645) on octaves [level - 1, level]; the FIRST
 * minimum of the descriptor distance, with no occupancy test, accepted at <= TH_HIGH (100).  Direction 2 -> 1 (:1271-1348) is the mirror
 * image with sR12, t12 and vbAlreadyMatched2.  Then the agreement check (:1350-1366).
 * Arithmetic: matrix * vector products accumulate in double and narrow once, R * x + t in one accumulation;
 * sR12[k] = (float)((double)s12 * R12[k]); sR21[k] = (float)((1.0 / (double)s12) * R12^T[k]); t21 = -(sR21 * t12); the norm accumulates in
 * double, then sqrt, then narrows; nothing is fused.  OpenCV's own rounding of scalar * Mat is not pinned by the reference.
 * Outputs: d_matches [n_pairs][nfeatures] = vpMatches12 on return as KF2 keypoint indices by KF1 keypoint: the filtered input entries
 * plus the agreed new ones, -1 elsewhere and past KF1's count; it may not alias d_match12.  d_nfound [n_pairs] = the return value.
 * d_match1 / d_match2 [n_pairs][nfeatures] (nullable) = vnMatch1 / vnMatch2.  IVF_E_INVALID: a null required pointer, th <= 0, d_matches
 * == d_match12, n_pairs > max_pairs.  Uses the handle's grid scratch with two grids per pair (grown at the first call: the new buffers
 * are allocated before the old ones are freed, so a failure, IVF_E_NO_DEVICE, leaves the handle usable) and a query scratch of its own of
 * 2 * nfeatures queries per pair, allocated at the first call. */
int  ivf_tracker_search_by_sim3(ivf_tracker* t, const uint8_t* d_records, size_t record_bytes, int n_records, const int32_t* d_pairs, int n_pairs,
                                const int32_t* d_select, const float* d_poses, const ivf_local_point* d_kf_points, const float* d_sim3,
                                const int32_t* d_match12, const uint8_t* d_inlier, float th, int32_t* d_matches, int32_t* d_nfound,
                                int32_t* d_match1, int32_t* d_match2, void* hip_stream);
/* The first two lines of Tracking::Relocalization (ORB/src/Tracking.cc:2274-2285), on the device: with them the chain runs from a lost
 * frame's gather record to its restart pose without the host reading anything.
 *
 * ivf_tracker_bow_vectors: Frame::ComputeBoW's mBowVec (ORB/src/Frame.cc:683-694) for frame slot f = record d_frames[f], i.e.
 * TemplatedVocabulary::transform (TemplatedVocabulary.h:1126-1204) with the ORB vocabulary's TF_IDF weights and L1_NORM.  Every keypoint
 * below the record's count descends the tree (:1217-1259, the descent ivf_bow_transform and ivf_tracker_search_by_bow run); a leaf of
 * weight <= 0 contributes nothing (:1157); a word that k keypoints reach holds the result of k successive `+= weight` from 0.0
 * (BowVector.cpp:34-46: the map's operator[] then addWeight), added in keypoint order; the L1 norm is the sum of fabs(value) in ascending
 * word order and every value is divided by it when it is > 0.0 (BowVector.cpp:62-84).  All of it in f64, nothing fused or
 * reassociated: word ids and value bits equal ivf_bow_transform + ivf_bow_vectors on the same descriptors.
 * d_bow_word / d_bow_value [n_frames][nfeatures]: the words ascending and their values, -1 / 0.0 beyond the count; d_bow_n [n_frames]:
 * the number of words, -1 for a record index outside [0, n_records): nothing else of that slot is written.  n_frames is not bound by
 * max_pairs (the call needs no scratch of the handle).  IVF_E_INVALID: a null required pointer, n_frames < 0, a vocabulary on another
 * device than the tracker.  Every loop is bounded by nfeatures or by the depth of the tree.  Asynchronous on hip_stream; obeys the
 * handle's one-call-at-a-time rule. */
int  ivf_tracker_bow_vectors(ivf_tracker* t, const ivf_vocabulary* voc, const uint8_t* d_records, size_t record_bytes, int n_records,
                             const int32_t* d_frames, int n_frames, int32_t* d_bow_word, double* d_bow_value, int32_t* d_bow_n,
                             void* hip_stream);
/* ivf_tracker_reloc_candidates: KeyFrameDatabase::DetectRelocalizationCandidates (ORB/src/KeyFrameDatabase.cc:199-309) with
 * mpVoc->score = L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), for n_frames lost frames against one database of
 * n_keyframes keyframes.  The database is flat device arrays the caller keeps between calls, keyframe index = order of
 * KeyFrameDatabase::add: d_kf_bow_word / d_kf_bow_value [n_keyframes][nfeatures] and d_kf_bow_n [n_keyframes] as
 * ivf_tracker_bow_vectors wrote them when the keyframe was inserted; d_kf_live [n_keyframes] (nullable), 0 = erased: in no inverted
 * list, so it shares no word, is never scored and is skipped as a neighbour; d_kf_neigh [n_keyframes][10] =
 * GetBestCovisibilityKeyFrames(10) as keyframe indices in order, -1 after the last; d_kf_reloc_score [n_keyframes] (nullable, NULL =
 * 0.0f), read-only: the mRelocScore each keyframe holds BEFORE this call, the same for every frame of the batch -- the reference reads it
 * (:276-277) for a neighbour that shares a word with the frame but was not scored, and that is all such a neighbour contributes;
 * d_kf_record [n_keyframes]: the gather record of each keyframe in the block the later searches read, -1 = none.  The frames:
 * d_bow_word / d_bow_value / d_bow_n as ivf_tracker_bow_vectors wrote them and d_frame_record [n_frames].  Per frame:
 *   mnRelocWords of keyframe k = the number of words both vectors hold (:207-222), 0 = the keyframe is absent;
 *   minCommonWords = (int)(maxCommonWords * 0.8f), the product in float (:235); keyframes with mnRelocWords > minCommonWords are scored
 *   (:246): the f64 sum of fabs(vi - wi) - fabs(vi) - fabs(wi), vi the frame's value, over the common words in ascending word order
 *   (ScoringObject.cpp:34-59), then -score / 2.0 narrowed to float (:249);
 *   per scored keyframe accScore = its score, then for its neighbours in order -- skipping -1 (or any index outside the database),
 *   erased keyframes and those that share no word (:273) -- accScore += s in float, s = the neighbour's score of this query if it was
 *   scored, else its d_kf_reloc_score; pBestKF moves to the neighbour on s > bestScore, strictly (:276-281);
 *   bestAccScore starts at 0 (:259, :285); entries with accScore > 0.75f * bestAccScore, strictly, are retained (:290-297);
 *   the distinct pBestKF of the retained entries come out in the order of lScoreAndMatch (:294-305), which is the order of first
 *   encounter walking the frame's words ascending and each word's inverted list in insertion order (:207-221), i.e. scored keyframes
 *   ordered by (smallest shared word, keyframe index), each pBestKF at its first retained occurrence.
 * Outputs: d_cand [n_frames][max_candidates] keyframe indices, -1 beyond the count; d_ncand [n_frames] the true count, even above
 * max_candidates (then the first max_candidates are written); d_pairs [n_frames * max_candidates][2] and d_select
 * [n_frames * max_candidates]: slot f * max_candidates + j = (d_kf_record[candidate j], d_frame_record[f]) and 1 for a written
 * candidate whose keyframe has a record (>= 0), else (-1, -1) and 0 -- what ivf_tracker_search_by_bow, ivf_tracker_search_reloc and
 * (through the pairs' frame column) ivf_tracker_solve_pnp take, n_pairs = n_frames * max_candidates <= max_pairs being the caller's to
 * respect; d_scores [n_frames][n_keyframes] (nullable): the float score of every scored keyframe, the NaN with bits 0x7fc00000
 * elsewhere -- what the caller folds into its mRelocScore state (:250); d_common [n_frames][n_keyframes] (nullable): mnRelocWords.
 * n_keyframes == 0 or a frame with d_bow_n <= 0 gives d_ncand = 0.  IVF_E_INVALID: a null required pointer, max_candidates < 1,
 * n_keyframes < 0, n_frames < 0, a vocabulary on another device than the tracker.  Every loop is bounded by nfeatures, n_keyframes or
 * 10; garbage input (unsorted words, a count above nfeatures, a neighbour outside the database) may give a meaningless answer but no
 * read outside the arrays.  Two runs are bit-identical.  Asynchronous on hip_stream, no host synchronisation; the scratch
 * (40 bytes per frame and keyframe) sits on the handle, grows on demand (the one place where the call waits, for the handle's previous
 * call, before it frees the smaller buffers; a refused growth, IVF_E_NO_DEVICE, leaves the handle usable with the scratch it had) and
 * obeys the one-call-at-a-time rule. */
int  ivf_tracker_reloc_candidates(ivf_tracker* t, const ivf_vocabulary* voc, const int32_t* d_kf_bow_word, const double* d_kf_bow_value,
                                  const int32_t* d_kf_bow_n, const uint8_t* d_kf_live, const int32_t* d_kf_neigh,
                                  const float* d_kf_reloc_score, const int32_t* d_kf_record, int n_keyframes, const int32_t* d_bow_word,
                                  const double* d_bow_value, const int32_t* d_bow_n, const int32_t* d_frame_record, int n_frames,
                                  int max_candidates, int32_t* d_cand, int32_t* d_ncand, int32_t* d_pairs, int32_t* d_select,
                                  float* d_scores, int32_t* d_common, void* hip_stream);
/* LoopClosing::DetectLoop (ORB/src/LoopClosing.cc:108-234) for n_queries new keyframes, on the device: with the two calls below a batch
 * goes from gather records (ivf_tracker_bow_vectors) to mvpEnoughConsistentCandidates as the pair table
 * ivf_tracker_search_by_bow_keyframes takes, without the host reading anything.  The database is ivf_tracker_reloc_candidates' (the
 * current keyframes are rows of it already); new are the connected sets of every keyframe as a CSR -- d_conn_start [n_keyframes + 1],
 * d_conn [n_conn] database indices = GetVectorCovisibleKeyFrames / GetConnectedKeyFrames, in any order -- and the queries:
 * d_query_kf [n_queries], the database index of each current keyframe, and d_query_visible [n_queries]: keyframe k is in the inverted
 * file of query q iff k < d_query_visible[q], it is live and k != d_query_kf[q].  That is mpKeyFrameDB->add(mpCurrentKF) after each
 * DetectLoop (:121, :151, :220): consecutive keyframes appended in order, each with visible = its own index, give the reference's
 * sequential result from one snapshot.  An entry of d_conn outside [0, n_keyframes) is skipped; a row whose offsets are negative,
 * decreasing or past n_conn is empty.
 *
 * ivf_tracker_loop_candidates: minScore (:129-143) and KeyFrameDatabase::DetectLoopCandidates (ORB/src/KeyFrameDatabase.cc:76-197).
 * d_query_select [n_queries] (nullable): 0 = the early return of :119 (mnId < mLastLoopKFid + 10): d_ncand = -2 and nothing else of
 * the query is written; a d_query_kf outside the database gives d_ncand = -1 likewise.  Per query:
 *   minScore = 1.0f, lowered with `<` by the score of every connected keyframe that is live (isBad, :135), whether or not it is visible;
 *   the score is L1Scoring::score as in ivf_tracker_reloc_candidates (f64 terms in ascending word order, -score / 2.0, narrowed to
 *   float), so a connected keyframe that shares no word gives -0.0f and d_min_score keeps the bits of the row's first minimum;
 *   mnLoopWords of keyframe k = the words both vectors hold for a k in the inverted file and not in the connected row (:93-102), else 0:
 *   a connected keyframe never enters lKFsSharingWords, never raises maxCommonWords and is never accumulated as a neighbour;
 *   minCommonWords = (int)(maxCommonWords * 0.8f) (:120); keyframes with mnLoopWords > minCommonWords are scored (:129-135) and enter
 *   lScoreAndMatch iff si >= minScore (:136);
 *   per entry accScore = its score, then for its d_kf_neigh in order accScore += mLoopScore of every neighbour that was scored in THIS
 *   query, whether or not its own score reached minScore (:159); a neighbour that was not (0 < mnLoopWords <= minCommonWords included)
 *   adds nothing -- there is no stale score as in relocalization; pBestKF moves on a strictly greater score (:162);
 *   bestAccScore starts at minScore (:145); entries with accScore > 0.75f * bestAccScore, strictly, are retained (:176-184) and their
 *   distinct pBestKF come out in list order = (smallest shared word, keyframe index) of the entry (:182-193).
 * Outputs: d_min_score [n_queries]; d_cand [n_queries][max_candidates], -1 beyond the count; d_ncand [n_queries] the true count, even
 * above max_candidates; d_scores / d_common [n_queries][n_keyframes] (nullable) as ivf_tracker_reloc_candidates writes them.
 * IVF_E_INVALID: a null required pointer, a negative count, max_candidates < 1.  No read outside the arrays whatever they hold; two runs
 * are bit-identical; asynchronous on hip_stream; the scratch is ivf_tracker_reloc_candidates' (40 bytes per query and keyframe, grown
 * on demand, a refused growth leaves the handle usable); obeys the one-call-at-a-time rule. */
int  ivf_tracker_loop_candidates(ivf_tracker* t, const int32_t* d_kf_bow_word, const double* d_kf_bow_value, const int32_t* d_kf_bow_n,
                                 const uint8_t* d_kf_live, const int32_t* d_kf_neigh, int n_keyframes, const int32_t* d_conn_start,
                                 const int32_t* d_conn, int n_conn, const int32_t* d_query_kf, const int32_t* d_query_visible,
                                 const int32_t* d_query_select, int n_queries, int max_candidates, float* d_min_score, int32_t* d_cand,
                                 int32_t* d_ncand, float* d_scores, int32_t* d_common, void* hip_stream);
/* ivf_tracker_loop_consistency: the covisibility-consistency groups (ORB/src/LoopClosing.cc:148-230) for the queries of the call IN
 * ORDER, from d_cand / d_ncand of ivf_tracker_loop_candidates.  mvConsistentGroups is device memory of the caller, read and written:
 * d_group_member [group_cap][member_cap] keyframe indices ascending, -1 padded; d_group_size and d_group_count [group_cap] (the
 * consistency counter); d_n_groups [1]; rows at and beyond n_groups are cleared (-1, 0, 0) whenever the state is rewritten.  Per query:
 *   d_ncand < 0 (not selected, or no such keyframe): skipped, the state is untouched;
 *   d_ncand == 0: n_groups = 0 (:152);
 *   else the group of candidate i is its connected row plus itself (:169-170); it is consistent with previous group iG iff they share a
 *   keyframe (:176-187).  The new state, in candidate order: for each i the previous groups iG, ascending, for which i is the FIRST
 *   consistent candidate (vbConsistentGroup, :193-198), each as (group of i, count[iG] + 1); then, if i is consistent with no previous
 *   group, (group of i, 0) (:208-212).  Candidate i is enough-consistent iff count[iG] + 1 >= th for some iG it is consistent with
 *   (:199; th = mnCovisibilityConsistencyTh, 3 in the reference), whether or not iG was flagged before.
 * Outputs: d_enough [n_queries][max_candidates] = mvpEnoughConsistentCandidates as keyframe indices in candidate order, -1 padded;
 * d_nenough [n_queries]; d_pairs [n_queries][max_candidates][2] = (d_kf_record[query keyframe], d_kf_record[candidate]), the
 * (KF1, KF2) order of ivf_tracker_search_by_bow_keyframes, and d_select = 1 where both records are >= 0, else (-1, -1) and 0;
 * d_status [n_queries].  Overflow -- a group of more than member_cap keyframes, more than group_cap new entries, or d_ncand >
 * max_candidates (a truncated list) -- is a condition: the state stays as it was before that query, and d_status of it and of every
 * later query of the call is 1 with d_nenough = 0 and every select 0; 0 = exact.  A query with d_nenough > 0 is where the reference
 * goes on to ComputeSim3; the later queries of the call are computed as if that loop was rejected, which is what the reference does when
 * ComputeSim3 returns false.  IVF_E_INVALID: a null required pointer, a negative count, max_candidates / group_cap / member_cap < 1.
 * One workgroup walks the queries; every loop is bounded by a connected row, n_keyframes / 32, max_candidates, group_cap or member_cap.
 * The scratch (max_candidates * ((n_keyframes + 31) / 32 + 4 + group_cap) + 1 + 3 * group_cap words of 4 bytes) sits on the handle and grows
 * on demand. */
int  ivf_tracker_loop_consistency(ivf_tracker* t, const int32_t* d_kf_record, int n_keyframes, const int32_t* d_conn_start,
                                  const int32_t* d_conn, int n_conn, const int32_t* d_query_kf, int n_queries, const int32_t* d_cand,
                                  const int32_t* d_ncand, int max_candidates, int th, int32_t* d_group_member, int32_t* d_group_size,
                                  int32_t* d_group_count, int32_t* d_n_groups, int group_cap, int member_cap, int32_t* d_enough,
                                  int32_t* d_nenough, int32_t* d_pairs, int32_t* d_select, int32_t* d_status, void* hip_stream);

/* ---- Tracking::UpdateLocalMap and the tail of TrackLocalMap from a device-resident map ---------------------------------------------
 * The map as flat device arrays the caller keeps between calls, in the style of the keyframe database above: keyframe index = position
 * in the caller's tables, map-point index = position in `points`, -1 = none.  Every index read from one of these tables is checked
 * against its range before it is used: an out-of-range entry is skipped as if it were -1, a CSR row whose offsets are negative,
 * decreasing or past the table's length is an empty row.  No kernel reads outside the arrays, whatever the tables hold. */
typedef struct ivf_map_view {
    const ivf_local_point* points;   /* [n_points] the record the searches read; flags bit 0 = isBad(), bit 1 = Observations() > 0 */
    const int32_t* obs_offsets;      /* [n_points + 1] CSR into obs_kf */
    const int32_t* obs_kf;           /* [n_obs] MapPoint::GetObservations() as keyframe indices */
    const int32_t* kf_point_offsets; /* [n_keyframes + 1] CSR into kf_points; a row holds at most nfeatures entries (the keyframe's
                                      * keypoints), a longer one is read up to nfeatures */
    const int32_t* kf_points;        /* [n_kf_points] KeyFrame::GetMapPointMatches() as map-point indices or -1, in keypoint order */
    const uint8_t* kf_live;          /* [n_keyframes] 0 = isBad(); NULL = all live */
    const int32_t* kf_neigh;         /* [n_keyframes][10] GetBestCovisibilityKeyFrames(10), -1 padded (ivf_tracker_reloc_candidates' table) */
    const int32_t* kf_child_offsets; /* [n_keyframes + 1] CSR into kf_children */
    const int32_t* kf_children;      /* [n_children] GetChilds() in the order the caller's std::set iterates */
    const int32_t* kf_parent;        /* [n_keyframes] GetParent() or -1 */
    const int32_t* kf_order;         /* [n_keyframes] the keyframe indices in the order the host's std::map<KeyFrame*, int> iterates
                                      * them (by pointer value, which only the host knows): a permutation; NULL = identity.  The table is
                                      * walked by position: an out-of-range entry is skipped, a keyframe it does not name is never voted in */
    int32_t n_points, n_keyframes, n_obs, n_kf_points, n_children;
} ivf_map_view;
/* ivf_tracker_update_local_map: Tracking::UpdateLocalMap (ORB/src/Tracking.cc:2134-2270) = UpdateLocalKeyFrames then UpdateLocalPoints,
 * for n_frames frames against one map, between the first ivf_tracker_optimize_pose and ivf_tracker_search_local.  No records are read.
 * d_frame_points [n_frames][nfeatures] (in/out) = mCurrentFrame.mvpMapPoints as map-point indices or -1; entries past the frame's
 * keypoint count are -1 by contract.  Per frame:
 *   the vote (:2170-2185): every held point that is not bad adds one to every keyframe of its observations; a bad held point becomes -1
 *   in d_frame_points;
 *   no vote at all (:2187): the reference returns and UpdateLocalPoints runs on the previous mvpLocalKeyFrames.  d_local_kf
 *   [n_frames][max_local_keyframes] and d_n_local_kf [n_frames] are in/out like that member: the row is kept as it came in, its count is
 *   clamped to [0, max_local_keyframes] and written back, its entries are range-checked when the points are collected, d_ref_kf[f] is
 *   left alone;
 *   otherwise the voted, live keyframes in kf_order (:2197-2212); d_ref_kf[f] = pKFmax, the first in that order with a strictly larger
 *   count, written only when there is one (:2266-2269);
 *   the expansion (:2216-2264) over the K voted entries only (the end iterator is taken before the loop): leave when the list holds more
 *   than 80; append the first of the ten neighbours that is live and not yet included; append the first child, in the given order, that
 *   is live and not yet included; if there is a parent that is not yet included, append it WITHOUT a liveness test and leave the whole
 *   expansion (the break of :2261 ends the outer loop);
 *   d_n_local_kf[f] = the true length of the list; the row holds its first max_local_keyframes entries and -1 beyond the count;
 *   the points (:2143-2166): the keyframes of the row in order, each keyframe's matches in keypoint order, -1 and bad points skipped,
 *   every point once, at its first appearance.
 * Outputs in the layout ivf_tracker_search_local takes: d_points [n_frames][max_points_per_frame], copies of the map's records with
 * flags bit 0 additionally set on a point the frame already holds (mnLastFrameSeen == mnId, :2099-2100, :2114); d_point_ids, laid out
 * the same way, the map-point index of each; d_point_offsets [n_frames + 1] = f * max_points_per_frame; padding past the count has
 * flags = 1, id -1 and zeros elsewhere, so the search skips it; d_n_local_points [n_frames] = the true count, the first
 * max_points_per_frame in order being kept; d_occupied [n_frames][nfeatures] = 1 where the keypoint holds a point with
 * Observations() > 0 (ivf_tracker_search_local's d_occupied).
 * Not done here: IncreaseVisible / IncreaseFound / mnLastFrameSeen on the map.  They are map state shared by the frames of a batch;
 * the caller folds them in from d_frame_points and the search's outputs if it keeps them.
 * IVF_E_INVALID: a null pointer (kf_live and kf_order excepted), a negative table length, n_frames outside [0, max_pairs], a cap < 1,
 * arrays read as 16-byte pieces that are not 16-byte aligned; IVF_E_CAPACITY: n_frames * max_points_per_frame or max_local_keyframes *
 * nfeatures beyond 2^31 - 1 (or a hash set beyond 2^30 slots).  Two launches and one memset; integer atomics only, two runs are byte-identical.  The scratch sits on
 * the handle and grows on demand like ivf_tracker_reloc_candidates': a vote row of n_keyframes ints per frame when n_keyframes exceeds
 * what LDS holds (8192), and per frame a hash set of 8 bytes x the power of two >= 2 * min(max_local_keyframes * nfeatures, n_points).
 * Asynchronous on hip_stream; obeys the handle's one-call-at-a-time rule. */
int  ivf_tracker_update_local_map(ivf_tracker* t, const ivf_map_view* map, int32_t* d_frame_points, int n_frames, int max_local_keyframes,
                                  int max_points_per_frame, int32_t* d_local_kf, int32_t* d_n_local_kf, int32_t* d_ref_kf,
                                  ivf_local_point* d_points, int32_t* d_point_ids, int32_t* d_point_offsets, int32_t* d_n_local_points,
                                  uint8_t* d_occupied, void* hip_stream);
/* What ivf_tracker_update_local_map switches on and allocates, for tests and measurements: the largest n_keyframes whose vote rows
 * live in LDS, and the bytes of the hash sets of one call (cleared by its memset), 0 for arguments the call would refuse. */
int    ivf_tracker_local_map_lds_keyframes(void);
size_t ivf_tracker_local_map_set_bytes(int nfeatures, int n_points, int n_frames, int max_local_keyframes);
/* The tail of Tracking::TrackLocalMap (ORB/src/Tracking.cc:1636-1691) without a host read; n_frames <= max_pairs, asynchronous, the
 * handle's one-call-at-a-time rule; IVF_E_INVALID for a null required pointer or n_points < 0.
 * merge_local: d_frame_points[f][i] = d_point_ids[d_point_offsets[f] + d_assign[f][i]] where ivf_tracker_search_local's d_assign is
 * inside the frame's range (ORBmatcher.cc:124: the keypoint receives the point, replacing what it held); other entries are kept.
 * points_from_map: the input of ivf_tracker_optimize_pose over ALL held points: d_xw / d_has_point as ivf_tracker_points_from_local
 * writes them, from d_points[d_frame_points[f][i]].pos of the map; d_quality [n_frames][nfeatures] (nullable) = d_point_quality
 * [n_points] of the held point, 1.0f where d_point_quality is NULL or the keypoint holds none.
 * close_local_map (:1648-1677): d_ninliers[f] = the keypoints that hold a point and are not in d_outlier (ivf_tracker_optimize_pose's),
 * with only_tracking == 0 only those whose point has Observations() > 0 (flags bit 1); with stereo != 0 an outlier keypoint's entry
 * of d_frame_points becomes -1 (:1673-1674).  The 30 / 50 decision (:1684-1691) stays with the caller, who knows mnLastRelocFrameId. */
int  ivf_tracker_merge_local(ivf_tracker* t, const int32_t* d_point_ids, const int32_t* d_point_offsets, const int32_t* d_assign, int n_frames,
                             int32_t* d_frame_points, void* hip_stream);
int  ivf_tracker_points_from_map(ivf_tracker* t, const ivf_local_point* d_map_points, int n_points, const float* d_point_quality,
                                 const int32_t* d_frame_points, int n_frames, float* d_xw, uint8_t* d_has_point, float* d_quality,
                                 void* hip_stream);
int  ivf_tracker_close_local_map(ivf_tracker* t, const ivf_local_point* d_map_points, int n_points, const uint8_t* d_outlier, int n_frames,
                                 int only_tracking, int stereo, int32_t* d_frame_points, int32_t* d_ninliers, void* hip_stream);
/* ---- LocalMapping::CreateNewMapPoints (ORB/src/LocalMapping.cc:273-525), stereo / RGB-D branch, for n_kf current keyframes at once ----
 * Keyframe slot k = record d_kf[k] with up to max_neigh neighbours d_neigh[k][r] = GetBestCovisibilityKeyFrames(10) in that order, -1
 * padded.  Per neighbour, in rank order: the baseline gate (:311-319), ComputeF12 (:609-626), the epipole (ORB/src/ORBmatcher.cc:670-676),
 * KeyFrame::ComputeBoW reduced to mFeatVec (as ivf_tracker_search_by_bow computes it, at level L - levelsup),
 * ORBmatcher(0.6, false).SearchForTriangulation(..., false) (ORBmatcher.cc:663-829), and per match :352-497: the parallax decision, the
 * linear triangulation or Frame::UnprojectStereo, z1 <= 0, z2 <= 0, the reprojection gates (5.991 / 7.8 times mvLevelSigma2), dist == 0
 * and the scale-consistency gate with ratioFactor = 1.5f * scale_factors[1]; then the new point: MapPoint(x3D, current keyframe),
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth for its two observations (ORB/src/MapPoint.cc:247-376) and
 * SetQualityScore(min(mvKeyQualScore[idx1], mvKeyQualScore[idx2])) (:512-517).  No host read; asynchronous on hip_stream.
 * Inputs (device): d_records / record_bytes / n_records as every tracker call takes them (keypoints, descriptors, uRight and the depth
 * behind it, as ivf_tracker_points_from_pairs reads them); d_poses [n_records][12] = Tcw of every record, row-major 3x4; d_has_point
 * [n_records][nfeatures] = GetMapPoint(i) != NULL on entry, read only; d_key_quality [n_records][nfeatures] (nullable: the quality is 1)
 * = mvKeyQualScore; d_F12 [n_kf][max_neigh][9] (nullable) replaces the computed fundamental matrix: a host that holds the reference's
 * own F12 passes it; d_kf_order [n_records] (nullable = identity) = the record indices in the order the host's
 * std::map<KeyFrame*, size_t> iterates the keyframes (ivf_map_view.kf_order's meaning; a record it does not name comes behind the named
 * ones, in index order): with two observations both medians of ComputeDistinctiveDescriptors are 0 and the strict `<` keeps the
 * descriptor of the keyframe that comes first.
 * Within a keyframe the ranks are serial: a keypoint that received a point from neighbour r is skipped by the search of the ranks behind
 * it (AddMapPoint, then ORBmatcher.cc:708), one whose match failed a gate stays free.  The call works on a copy of the keyframe's row of
 * d_has_point.  SLOTS ARE INDEPENDENT: every slot sees d_has_point as on entry, also for a record that is a neighbour in one slot and
 * current in another; ordering keyframes against each other is the caller's job (separate calls).  Every idx1 searches independently
 * (vbMatched2 is tested and never set): several may take the same idx2, each gets its own point; a later equal distance replaces the
 * earlier one (`dist>bestDist`, :744).  CheckNewKeyFrames()' early return does not exist here: a batch runs all ranks.
 * Arithmetic: cv::Mat products, dot and norm as everywhere in the tracker (double accumulation, one narrowing);
 * F12 = K1^-T [t12]x R12 K2^-1 in closed form in f64 from the float poses and the handle's intrinsics, narrowed once -- NOT the
 * reference's float cv::Mat chain, from which it differs by a few ulps (d_F12 feeds the reference's own values); cos(2 atan2(b/2, z)) as
 * (z^2 - h^2) / (z^2 + h^2) in f64; the triangulation's singular vector from a cyclic one-sided Jacobi in f64 (fixed pair order, the
 * sweep limit of ivf_tracker_solve_pnp), narrowed to float -- more accurate than cv::SVD on CV_32F, so a match within that difference
 * of a gate may decide differently than the reference.
 * Outputs, dense by keypoint of the current keyframe (an idx1 creates at most one point per call): d_new_point [n_kf][nfeatures]
 * (16-byte aligned; flags = 2; zeros where no point was made), d_new_neigh (the neighbour's rank or -1), d_new_idx2 (or -1),
 * d_new_order (the point's rank in creation order -- neighbour rank, then idx1 ascending -- the order mlpRecentAddedMapPoints and the
 * map receive it in, or -1; of the points that share an idx2 the neighbour finally holds the last), d_new_quality (0 where none),
 * d_n_new [n_kf] = nnew.  Nullable diagnostics [n_kf][max_neigh][nfeatures]: d_matches = vMatchedIndices by idx1, -1 elsewhere;
 * d_stage = IVF_CREATE_* of every matched idx1 (IVF_CREATE_BASELINE on every keypoint of a neighbour skipped for its baseline).
 * A d_kf index outside [0, n_records) gives d_n_new = -1; a neighbour index outside it (-1) skips the neighbour.  IVF_E_CAPACITY:
 * n_kf * max_neigh > max_pairs; IVF_E_INVALID: a null required pointer, max_neigh < 1, levelsup < 0, a vocabulary on another device.
 * Obeys the handle's one-call-at-a-time rule; shares the feature-vector scratch of ivf_tracker_search_by_bow. */
#define IVF_CREATE_NONE           0   /* no match */
#define IVF_CREATE_BASELINE       1   /* neighbour skipped: baseline < mb */
#define IVF_CREATE_LOW_PARALLAX   2   /* no stereo and very low parallax (:414-415) */
#define IVF_CREATE_W_ZERO         3   /* :399 */
#define IVF_CREATE_Z1             4
#define IVF_CREATE_Z2             5
#define IVF_CREATE_CHI2_1_MONO    6
#define IVF_CREATE_CHI2_1_STEREO  7
#define IVF_CREATE_CHI2_2_MONO    8
#define IVF_CREATE_CHI2_2_STEREO  9
#define IVF_CREATE_DIST_ZERO      10
#define IVF_CREATE_RATIO_LOW      11
#define IVF_CREATE_RATIO_HIGH     12
#define IVF_CREATE_BY_SVD         13  /* created: linear triangulation */
#define IVF_CREATE_BY_STEREO1     14  /* created: UnprojectStereo of the current keyframe */
#define IVF_CREATE_BY_STEREO2     15  /* created: UnprojectStereo of the neighbour */
int  ivf_tracker_create_map_points(ivf_tracker* t, const ivf_vocabulary* voc, int levelsup, const uint8_t* d_records, size_t record_bytes,
                                   int n_records, const int32_t* d_kf, int n_kf, const int32_t* d_neigh, int max_neigh, const float* d_poses,
                                   const uint8_t* d_has_point, const float* d_key_quality, const float* d_F12, const int32_t* d_kf_order,
                                   ivf_local_point* d_new_point, int32_t* d_new_neigh, int32_t* d_new_idx2, int32_t* d_new_order,
                                   float* d_new_quality, int32_t* d_n_new, int32_t* d_matches, uint8_t* d_stage, void* hip_stream);
/* MapPoint::ComputeDistinctiveDescriptors (ORB/src/MapPoint.cc:247-312): desc = the n observed descriptors (rows of
 * vDescriptors, in mObservations order); *best_index = the row to copy into mDescriptor, *best_median (nullable) its median. */
int  ivf_distinctive_descriptor(const uint8_t* desc, int n, int* best_index, int* best_median, int device_id);

/* ---- device-resident frame -----------------------------------------------------------------------
 * Frame::AssignFeaturesToGrid (ORB/src/Frame.cc:415-430) once per frame on the device: keypoints (mvKeysUn), descriptors
 * and the 64x48 bucket grid (buckets in the reference's ix-major order, keypoints of a bucket in insertion order) stay
 * in HBM; searches against the frame then run GetFeaturesInArea (:615-668) and DescriptorDistance for every query on
 * the device and only replay the order-dependent assignment on the host. */
typedef struct ivf_frame ivf_frame;
int  ivf_frame_create(const ivf_keypoint* kps, const uint8_t* desc, const float* uright, int n, const ivf_bounds* bounds,
                      int device_id, ivf_frame** out);
void ivf_frame_destroy(ivf_frame* f);
/* number of keypoints of the frame (Frame::N) -- NOT the number that fell inside the grid */
int  ivf_frame_count(const ivf_frame* f);
/* the grid as built on the device: cell_start [64*48+1] (cell = ix*48 + iy), cell_index [n] */
int  ivf_frame_grid(const ivf_frame* f, int32_t* cell_start, int32_t* cell_index);
/* ivf_search_by_projection against the resident frame (same query arrays, same results) */
int  ivf_frame_search_by_projection(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_ur,
                                    const float* q_radius, const int32_t* q_min_level, const int32_t* q_max_level,
                                    const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid, const uint8_t* q_blocks,
                                    int check_orientation, int32_t* cur_assign, int* nmatches);
/* ivf_search_map_points (SearchByProjection(F, mapPoints), Tracking::SearchLocalPoints) against the resident frame */
int  ivf_frame_search_map_points(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_ur, const float* q_radius,
                                 const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid, const uint8_t* q_blocks,
                                 float nn_ratio, int32_t* cur_assign, int* nmatches);

/* A resident frame made straight from a batch of the front end (run `age` back, pair, side 0 = left / 1 = right): keypoints,
 * descriptors and uRight are copied device -> device and the grid is built on the device; only the keypoint count is read
 * back.  The greedy replays' host mirror (angle, octave, uRight: 28 B per keypoint) is fetched by the first search.
 * With a camera set for that run (ivf_frontend_set_camera) the left frame's keypoints and grid are those of mvKeysUn
 * (Frame::AssignFeaturesToGrid reads mvKeysUn, ORB/src/Frame.cc:424); pass the bounds of ivf_image_bounds. */
int  ivf_frame_create_from_frontend(ivf_frontend* fe, int age, int pair, int side, const ivf_bounds* bounds, ivf_frame** out);
/* The remaining window searches against a resident frame: same semantics as ivf_search_keyframe_points, ivf_fuse_candidates
 * (the frame's own uRight is the keyframe's mvuRight), ivf_search_by_sim3 (two resident keyframes) and
 * ivf_search_by_projection_reloc, with windows AND Hamming distances computed on the device (k_grid_window). */
int  ivf_frame_search_keyframe_points(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_radius,
                                      const int32_t* q_level, const uint8_t* q_desc, const uint8_t* q_valid, int32_t* matched, int* nmatches);
int  ivf_frame_fuse_candidates(ivf_frame* f, const float* inv_level_sigma2, int n_levels, int n_q, const float* q_u, const float* q_v,
                               const float* q_ur, const float* q_radius, const int32_t* q_level, const uint8_t* q_desc,
                               const uint8_t* q_valid, int32_t* best_idx, int32_t* best_dist);
int  ivf_frame_search_by_sim3(ivf_frame* f1, ivf_frame* f2,
                              const float* q12_u, const float* q12_v, const float* q12_radius, const int32_t* q12_level,
                              const uint8_t* q12_desc, const uint8_t* q12_valid,
                              const float* q21_u, const float* q21_v, const float* q21_radius, const int32_t* q21_level,
                              const uint8_t* q21_desc, const uint8_t* q21_valid, int32_t* matches12, int* nfound);
int  ivf_frame_search_by_projection_reloc(ivf_frame* f, int n_q, const float* q_u, const float* q_v, const float* q_radius,
                                          const int32_t* q_level, const float* q_angle, const uint8_t* q_desc, const uint8_t* q_valid,
                                          int orb_dist, int check_orientation, int32_t* cur_assign, int* nmatches);

/* ---- rectification in front of the extractor -------------------------------------------------
 * cv::initUndistortRectifyMap(K, D, R, P(0:3,0:3), size, CV_32F, map1, map2) as the driver calls it
 * (introspective_ORB_SLAM/Examples/Stereo/stereo_kitti.cc:285-343): host-side, double arithmetic, OpenCV 4.x plain C++
 * path.  K, R (NULL = identity), P: 3x3 row-major; dist = k1,k2,p1,p2[,k3[,k4,k5,k6[,s1..s4]]]
 * (n_dist 0, 4, 5, 8 or 12; tilt terms unsupported); map1/map2: [height][width] f32 (source x / source y). */
int  ivf_init_undistort_rectify_map(const double* K, const double* dist, int n_dist, const double* R, const double* P,
                                    int width, int height, float* map1, float* map2);
/* cv::remap(src, dst, map1, map2, cv::INTER_LINEAR) for 8-bit images, 1 or 3 interleaved channels, BORDER_CONSTANT 0
 * (stereo_kitti.cc:462-468 left/right image, :519-521 predicted cost image).  The maps are converted once
 * to the fixed-point form cv::remap derives per call and stay on the device; (width, height) = destination = map size. */
typedef struct ivf_remap ivf_remap;
int  ivf_remap_create(const float* map1, const float* map2, int width, int height, int src_width, int src_height,
                      int channels, int device_id, ivf_remap** out);
void ivf_remap_destroy(ivf_remap* r);
/* host buffers (drop-in for one cv::remap call; synchronous) */
int  ivf_remap_apply(ivf_remap* r, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride);
/* device buffers, n_images images image_stride bytes apart, on `hip_stream` (hipStream_t, NULL = default stream); asynchronous */
int  ivf_remap_apply_device(ivf_remap* r, const uint8_t* d_src, int src_stride, size_t src_image_stride, uint8_t* d_dst,
                      int dst_stride, size_t dst_image_stride, int n_images, void* hip_stream);
/* test aid: the fixed-point maps as cv::convertMaps would give them: xy [height][width][2] int16, alpha [height][width] (fy<<5|fx) */
int  ivf_remap_get_fixed_maps(const ivf_remap* r, int16_t* xy, uint16_t* alpha);

/* cv::resize(src, dst, cv::Size(dst_width, dst_height)) with the default INTER_LINEAR, 8-bit images of 1 or 3 interleaved channels
 * (Examples/Stereo/stereo_airsim.cc:389-390: the RGB image to the network's 512x512 input; :410-411: the u8 cost map back to the image
 * size).  OpenCV's fixed-point arithmetic, bit-exact: 11-bit coefficients, any down- or up-scale per axis.  The
 * coefficient tables are built once per handle and stay on the device.  channels 1 or 3; sources of at most 65536 pixels per axis. */
typedef struct ivf_resize ivf_resize;
int  ivf_resize_create(int src_width, int src_height, int dst_width, int dst_height, int channels, int device_id, ivf_resize** out);
void ivf_resize_destroy(ivf_resize* r);
/* host buffers (drop-in for one cv::resize call, stereo_airsim.cc:389-390 / :410-411; synchronous) */
int  ivf_resize_apply(ivf_resize* r, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride);
/* device buffers (stereo_airsim.cc:389-390 / :410-411 for n_images images): image i at d_src + i * src_image_stride, rows of src_stride
 * bytes, likewise the destination; on `hip_stream` (hipStream_t, NULL = default stream); asynchronous */
int  ivf_resize_apply_device(ivf_resize* r, const uint8_t* d_src, int src_stride, size_t src_image_stride,
                             uint8_t* d_dst, int dst_stride, size_t dst_image_stride, int n_images, void* hip_stream);
/* test aid, host only, needs no device: one axis of ssize -> dsize as cv::resize builds it (stereo_airsim.cc:389-390 / :410-411), the
 * table behind both the handles above and the extractor's pyramid: per destination index d the two source indices the pass reads,
 * idx0 = clip(s) and idx1 = clip(s + 1) with s = cvFloor(f), f = (float)((d + 0.5) * (1. / ((double)dsize / ssize)) - 0.5), and the
 * 11-bit coefficients w0 = saturate_cast<short>((1 - (f - s)) * 2048), w1 = saturate_cast<short>((f - s) * 2048).  That is the row
 * rule; the column rule is the same table with w0 = 2048, w1 = 0 where idx0 == idx1 (cv::resize clamps the column and sets fx = 0). */
int  ivf_resize_axis_table(int ssize, int dsize, int32_t* idx0, int32_t* idx1, int16_t* w0, int16_t* w1);

/* measurement aid (bench.py): HIP events bracket the network's most expensive launch (fused depthwise 3x3 + 1x1
 * projection 960 -> 160 of block 15, k_fcn_dwpw<5,4>) on the stream each forward runs on.  probe_stats returns the summed
 * duration of the last `last_n` probed forwards (0 = all kept, at most 64) and the batch size of the oldest of them. */
int  ivf_fcn_probe_enable(ivf_fcn* f);
/* r05: two probes -- 0 (default) = block 15 (k_fcn_irbd4<true>: launched twice per forward, blocks 15 and 16), 1 = block 17
 * (k_fcn_irbd4h: the largest single launch); probe_info / probe_stats report the selected one. */
int  ivf_fcn_probe_select(ivf_fcn* f, int which);
int  ivf_fcn_probe_stats(ivf_fcn* f, int last_n, double* sum_ms, int* n_out, int* batch);
/* which kernel the probe bracketed, as dispatched (e.g. "ivffcn::k_fcn_dwpw<5, 4> 960->160"), and its algorithmic HBM bytes
 * per image (hidden tensor read once + residual read + output written).  IVF_E_STATE before the first probed forward. */
int  ivf_fcn_probe_info(const ivf_fcn* f, char* name, int name_cap, double* algorithmic_bytes_per_image);

#ifdef __cplusplus
}
#endif
#endif /* IVFRONT_H */
