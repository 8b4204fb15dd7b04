// TEST-ONLY driver: RUNS the adapter's ivf::UndistortKeyPoints and ivf::ComputeImageBounds (include/ivfront_orbslam.hpp; the bodies of
// Frame::UndistortKeyPoints / Frame::ComputeImageBounds, ORB/src/Frame.cc:696-756) against the mock cv types of tests/cv_mock, the way
// a Frame constructor calls them: mK 3x3 CV_32F, mDistCoef n x 1 CV_32F (ORB/src/Tracking.cc:106-123), mvKeys -> mvKeysUn.
// Scenario file: int32 {cols, rows, n_dist, n_keys}; float {fx, fy, cx, cy}; float dist[n_dist]; n_keys x {float x, y, size, angle,
// response; int32 octave}.  Result file: n_keys keypoints in the same form, then float {mnMinX, mnMinY, mnMaxX, mnMaxY}.
// tests/test_gpu_undistort_adapter.py compares it byte for byte with the ctypes path.
#include "ivfront_orbslam.hpp"
#include <cstdio>

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: undistort_driver scenario.bin result.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> out;
    auto put = [&](const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    try {
        int32_t hdr[4];
        float k[4];
        if (fread(hdr, 4, 4, f) != 4 || fread(k, 4, 4, f) != 4) throw std::runtime_error("short header");
        const int cols = hdr[0], rows = hdr[1], nDist = hdr[2], nKeys = hdr[3];
        cv::Mat mK(3, 3, CV_32F);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) mK.at<float>(i, j) = i == j ? 1.0f : 0.0f;     // cv::Mat::eye
        mK.at<float>(0, 0) = k[0]; mK.at<float>(1, 1) = k[1]; mK.at<float>(0, 2) = k[2]; mK.at<float>(1, 2) = k[3];
        cv::Mat mDistCoef(nDist, 1, CV_32F);
        for (int i = 0; i < nDist; i++) if (fread(&mDistCoef.at<float>(i, 0), 4, 1, f) != 1) throw std::runtime_error("short distortion vector");
        std::vector<cv::KeyPoint> mvKeys(nKeys), mvKeysUn;
        for (cv::KeyPoint& p : mvKeys) {
            float v[5]; int32_t oct;
            if (fread(v, 4, 5, f) != 5 || fread(&oct, 4, 1, f) != 1) throw std::runtime_error("short keypoint list");
            p.pt.x = v[0]; p.pt.y = v[1]; p.size = v[2]; p.angle = v[3]; p.response = v[4]; p.octave = oct;
        }
        fclose(f);
        ivf::UndistortKeyPoints(mvKeys, mK, mDistCoef, mvKeysUn);
        if (mvKeysUn.size() != mvKeys.size()) throw std::runtime_error("mvKeysUn has another size than mvKeys");
        for (const cv::KeyPoint& p : mvKeysUn) {
            const float v[5] = {p.pt.x, p.pt.y, p.size, p.angle, p.response}; const int32_t oct = p.octave;
            put(v, sizeof v); put(&oct, 4);
        }
        float b[4];
        ivf::ComputeImageBounds(cols, rows, mK, mDistCoef, b[0], b[1], b[2], b[3]);
        put(b, sizeof b);
    } catch (const std::exception& e) { fprintf(stderr, "undistort_driver: %s\n", e.what()); return 1; }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), 1, out.size(), o) != out.size()) return 2;
    fclose(o);
    return 0;
}
