/*
 * Stand-in <opencv2/imgproc/imgproc.hpp> (test infrastructure): cv::resize(INTER_LINEAR) and cv::GaussianBlur(7x7, sigma 2,
 * BORDER_REFLECT_101), both delegated to the oracle's primitives (orc_resize_linear_8u, orc_gauss7_8u).  Any other argument
 * set is refused: the reference's extractor uses no other.
 */
#ifndef IVF_CVSHIM_IMGPROC_HPP
#define IVF_CVSHIM_IMGPROC_HPP
#include "../core.hpp"

namespace cv {

enum InterpolationFlags { INTER_NEAREST = 0, INTER_LINEAR = 1 };

inline void resize(InputArray _src, OutputArray _dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR)
{
    Mat src = _src.getMat();
    CV_Assert(interpolation == INTER_LINEAR && fx == 0 && fy == 0);
    CV_Assert(!src.empty() && dsize.width > 0 && dsize.height > 0);
    _dst.create(dsize, src.type());
    Mat dst = _dst.getMat();
    CV_Assert(dst.data != src.data);
    orc_resize_linear_8u(src.data, (int)src.step1(), src.cols, src.rows, dst.data, (int)dst.step1(), dst.cols, dst.rows);
}

inline void GaussianBlur(InputArray _src, OutputArray _dst, Size ksize, double sigmaX, double sigmaY = 0,
                         int borderType = BORDER_DEFAULT)
{
    CV_Assert(ksize.width == 7 && ksize.height == 7 && sigmaX == 2 && (sigmaY == 2 || sigmaY == 0));
    CV_Assert((borderType & ~BORDER_ISOLATED) == BORDER_REFLECT_101);
    Mat in = _src.getMat();
    CV_Assert(!in.empty() && (!in.isSubmatrix() || (borderType & BORDER_ISOLATED)));
    Mat src = in.clone();                       /* the call may be in place */
    _dst.create(src.size(), src.type());
    Mat dst = _dst.getMat();
    orc_gauss7_8u(src.data, (int)src.step1(), src.cols, src.rows, dst.data, (int)dst.step1());
}

}  // namespace cv
#endif
