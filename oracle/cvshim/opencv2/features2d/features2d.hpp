/*
 * Stand-in <opencv2/features2d/features2d.hpp> (test infrastructure): cv::FAST and cv::KeyPointsFilter::retainBest,
 * both delegated to the oracle's primitives (orc_fast_detect, orc_retain_best) -- no second restatement of either.
 */
#ifndef IVF_CVSHIM_FEATURES2D_HPP
#define IVF_CVSHIM_FEATURES2D_HPP
#include "../core.hpp"

namespace cv {

/* FAST(image, keypoints, threshold, nonmaxSuppression = true): FAST-9/16; keypoints come out with size 7, angle -1, octave 0 and
 * response = corner score, in row-major order of position */
inline void FAST(InputArray _image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmaxSuppression = true)
{
    CV_Assert(nonmaxSuppression);
    Mat img = _image.getMat();
    keypoints.clear();
    if (img.empty()) return;
    const int cap = img.rows * img.cols;
    std::vector<orc_keypoint> buf((size_t)cap);
    const int n = orc_fast_detect(img.data, (int)img.step1(), img.cols, img.rows, threshold, buf.data(), cap);
    CV_Assert(0 <= n && n <= cap);
    keypoints.reserve((size_t)n);
    for (int i = 0; i < n; i++)
        keypoints.push_back(KeyPoint(Point2f(buf[i].x, buf[i].y), buf[i].size, buf[i].angle, buf[i].response, buf[i].octave, -1));
}

class KeyPointsFilter {
public:
    /* Keeps the n_points strongest keypoints.  OpenCV also keeps every keypoint that ties with the weakest survivor, so its
     * result can be longer than n_points; orc_retain_best states retainBest together with the truncation to n_points that each
     * call site of the reference applies straight after it, and the survivors [0, n_points) are the same either way.
     * class_id is not carried through orc_keypoint: nothing on this path sets it, so it is restored to OpenCV's default -1. */
    static void retainBest(std::vector<KeyPoint>& keypoints, int npoints)
    {
        const int n = (int)keypoints.size();
        std::vector<orc_keypoint> buf((size_t)n);
        for (int i = 0; i < n; i++) {
            const KeyPoint& k = keypoints[i];
            CV_Assert(k.class_id == -1);
            orc_keypoint o = {k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave};
            buf[i] = o;
        }
        const int m = orc_retain_best(buf.data(), n, npoints);
        CV_Assert(0 <= m && m <= n);
        keypoints.resize((size_t)m);
        for (int i = 0; i < m; i++)
            keypoints[i] = KeyPoint(Point2f(buf[i].x, buf[i].y), buf[i].size, buf[i].angle, buf[i].response, buf[i].octave, -1);
    }
};

}  // namespace cv
#endif
