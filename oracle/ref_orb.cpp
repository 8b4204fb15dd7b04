/*
 * ref_orb.cpp -- C ABI over the reference's own ORB_SLAM2::ORBextractor (TEST INFRASTRUCTURE ONLY).
 *
 * oracle/Makefile (target `ref`) compiles the reference's src/ORBextractor.cc, unmodified, against the stand-in OpenCV headers
 * of oracle/cvshim/ and links it with this file into oracle/_ref/libivf_ref_orb.so.  The extractor's logic is then the
 * reference's; the OpenCV primitives under it are the oracle's (oracle/cvshim delegates to orc_*).  Neither that library nor
 * any line of the reference is committed.  tests/ref_lib.py is the loader.
 *
 * Layouts are the oracle's (oracle/ivf_oracle.h): keypoints as orc_keypoint, descriptors as n x 32 bytes, tables as in
 * orc_extractor_tables.  Return codes: 0 ok, -1 bad argument, -2 more keypoints than `cap`, -4 the shim asserted (an
 * out-of-range view or at<>, an unsupported argument): ref_orb_last_error() then holds the message.
 */
#include <opencv2/core.hpp>
#include <string>
#include <vector>

#include "ORBextractor.h"
#include "ivf_oracle.h"

#ifndef REF_ORB_BUILD_ID
#error "REF_ORB_BUILD_ID must be defined by oracle/Makefile"
#endif

namespace {

/* derived only to read the protected tables */
class Extractor : public ORB_SLAM2::ORBextractor {
public:
    Extractor(int n, float sf, int nl, int ini, int mn, bool intro) : ORB_SLAM2::ORBextractor(n, sf, nl, ini, mn, intro) {}
    const std::vector<int>& featuresPerLevel() const { return mnFeaturesPerLevel; }
    const std::vector<int>& uMax() const { return umax; }
};

struct Handle {
    Extractor* ext;
    int nlevels;
    std::vector<int> level_count;
    std::vector<unsigned char> plane;     /* contiguous copy handed out by the level accessors */
    bool had_cost;
};

thread_local std::string g_error;

int level_copy(Handle* h, const std::vector<cv::Mat>& pyr, int level, int pad, const uint8_t** data, int* w, int* hh)
{
    if (!h || level < 0 || level >= h->nlevels || pyr[level].empty()) return -1;
    try {
        const cv::Mat& m = pyr[level];
        const int W = m.cols + 2 * pad, H = m.rows + 2 * pad;
        h->plane.resize((size_t)W * H);
        /* the level is a view 19 pixels inside its bordered plane (ComputePyramid), so up to 19 pixels round it are storage */
        for (int y = 0; y < H; y++) {
            const unsigned char* row = m.data + ((ptrdiff_t)y - pad) * (ptrdiff_t)m.step1() - pad;
            std::copy(row, row + W, h->plane.begin() + (size_t)y * W);
        }
        *data = h->plane.data(); *w = W; *hh = H;
        return 0;
    } catch (const std::exception& e) { g_error = e.what(); return -4; }
}

}  // namespace

extern "C" {

/* "<ours>:<reference>": sha256[:16] over this file + the shim headers + ivf_oracle.h, and over the reference's two extractor files */
const char* ref_orb_build_id(void) { return REF_ORB_BUILD_ID; }
const char* ref_orb_last_error(void) { return g_error.c_str(); }

void* ref_orb_create(const orc_params* p)
{
    if (!p || p->nlevels < 1 || p->nlevels > ORC_MAX_LEVELS) return nullptr;
    try {
        Handle* h = new Handle();
        h->ext = new Extractor(p->nfeatures, p->scale_factor, p->nlevels, p->ini_th_fast, p->min_th_fast, p->enable_introspection != 0);
        h->nlevels = p->nlevels;
        h->level_count.assign((size_t)p->nlevels, 0);
        h->had_cost = false;
        return h;
    } catch (const std::exception& e) { g_error = e.what(); return nullptr; }
}

void ref_orb_destroy(void* hv)
{
    Handle* h = (Handle*)hv;
    if (!h) return;
    delete h->ext;
    delete h;
}

void ref_orb_tables(void* hv, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2, int* features_per_level, int* umax16)
{
    Handle* h = (Handle*)hv;
    const std::vector<float> sc = h->ext->GetScaleFactors(), inv = h->ext->GetInverseScaleFactors();
    const std::vector<float> s2 = h->ext->GetScaleSigmaSquares(), is2 = h->ext->GetInverseScaleSigmaSquares();
    for (int l = 0; l < h->nlevels; l++) {
        if (scale) scale[l] = sc[l];
        if (inv_scale) inv_scale[l] = inv[l];
        if (sigma2) sigma2[l] = s2[l];
        if (inv_sigma2) inv_sigma2[l] = is2[l];
        if (features_per_level) features_per_level[l] = h->ext->featuresPerLevel()[l];
    }
    if (umax16) for (size_t v = 0; v < 16; v++) umax16[v] = v < h->ext->uMax().size() ? h->ext->uMax()[v] : 0;
}

int ref_orb_extract(void* hv, const uint8_t* img, int w, int hgt, int stride, const uint8_t* cost, int cost_stride,
                    orc_keypoint* kps, uint8_t* desc, int cap, int* n_out)
{
    Handle* h = (Handle*)hv;
    if (!h || !n_out) return -1;
    *n_out = 0;
    std::fill(h->level_count.begin(), h->level_count.end(), 0);
    try {
        cv::Mat image, mask, descriptors;
        if (img && w > 0 && hgt > 0) image = cv::Mat(hgt, w, CV_8UC1, (void*)img, (size_t)stride);
        if (cost && w > 0 && hgt > 0) mask = cv::Mat(hgt, w, CV_8UC1, (void*)cost, (size_t)cost_stride);
        h->had_cost = !mask.empty();
        std::vector<cv::KeyPoint> keypoints;
        (*h->ext)(image, mask, keypoints, descriptors);
        const int n = (int)keypoints.size();
        if (n > cap) return -2;
        if (n > 0 && (descriptors.rows != n || descriptors.cols != 32)) { g_error = "descriptor matrix is not n x 32"; return -4; }
        for (int i = 0; i < n; i++) {
            const cv::KeyPoint& k = keypoints[i];
            if (k.octave < 0 || k.octave >= h->nlevels) { g_error = "keypoint octave out of range"; return -4; }
            orc_keypoint o = {k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave};
            kps[i] = o;
            std::copy(descriptors.ptr(i), descriptors.ptr(i) + 32, desc + (size_t)i * 32);
            h->level_count[(size_t)k.octave]++;
        }
        *n_out = n;
        return 0;
    } catch (const std::exception& e) { g_error = e.what(); return -4; }
}

/* mvImagePyramid[level] / mvQualityImagePyramid[level] after the last extract, as a contiguous copy valid until the next call on
 * this handle.  pad = 0 gives the level itself; 0 < pad <= 19 includes that many pixels of the border ComputePyramid put round it. */
int ref_orb_pyramid_level(void* hv, int level, int pad, const uint8_t** data, int* w, int* h)
{
    Handle* hd = (Handle*)hv;
    if (!hd || pad < 0 || pad > 19) return -1;
    return level_copy(hd, hd->ext->mvImagePyramid, level, pad, data, w, h);
}
int ref_orb_quality_level(void* hv, int level, int pad, const uint8_t** data, int* w, int* h)
{
    Handle* hd = (Handle*)hv;
    if (!hd || pad < 0 || pad > 19 || !hd->had_cost) return -1;
    return level_copy(hd, hd->ext->mvQualityImagePyramid, level, pad, data, w, h);
}
int ref_orb_level_count(void* hv, int level)
{
    Handle* h = (Handle*)hv;
    return (!h || level < 0 || level >= h->nlevels) ? -1 : h->level_count[(size_t)level];
}

}  // extern "C"
