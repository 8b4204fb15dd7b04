/*
 * Stand-in <opencv2/core.hpp> (TEST INFRASTRUCTURE ONLY): the part of OpenCV's core module that the reference's
 * ORBextractor.cc / ORBextractor.h use, written from OpenCV's documented behaviour so that the reference's own
 * extractor file compiles unmodified where OpenCV is absent (oracle/Makefile, target `ref`).
 *
 *  - 8-bit single-channel 2-D matrices only; anything else throws cv::Exception, as a failed CV_Assert does.
 *  - Views (operator()(Rect), rowRange, colRange) share storage with their parent.  Views and at<>() check bounds and throw.
 *  - Arithmetic OpenCV owns (cvRound, fastAtan2, and FAST / resize / GaussianBlur / retainBest in the sibling headers) is NOT
 *    restated here: it is delegated to the oracle's orc_* primitives (oracle/ivf_oracle.h), so that orc_set_opencv_variant
 *    applies to this build too.  Only exact integer / copy operations are implemented here.
 */
#ifndef IVF_CVSHIM_CORE_HPP
#define IVF_CVSHIM_CORE_HPP

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "ivf_oracle.h"

#define CV_PI 3.1415926535897932384626433832795
#define CV_8U 0
#define CV_8UC1 0

namespace cv {

typedef unsigned char uchar;

class Exception : public std::runtime_error {
public:
    explicit Exception(const std::string& what) : std::runtime_error(what) {}
};

#define IVF_CV_STR2(x) #x
#define IVF_CV_STR(x) IVF_CV_STR2(x)
#define CV_Assert(expr) \
    do { if (!(expr)) throw ::cv::Exception("cvshim " __FILE__ ":" IVF_CV_STR(__LINE__) ": assertion failed: " #expr); } while (0)

/* ---- scalar helpers ---- */
inline int cvRound(double v) { return orc_cv_round_d(v); }
inline int cvRound(float v) { return orc_cv_round_f(v); }
inline int cvRound(int v) { return v; }
inline int cvFloor(double v) { int i = (int)v; return i - (i > v); }
inline int cvFloor(float v) { int i = (int)v; return i - (i > v); }
inline int cvFloor(int v) { return v; }
inline int cvCeil(double v) { int i = (int)v; return i + (i < v); }
inline int cvCeil(float v) { int i = (int)v; return i + (i < v); }
inline int cvCeil(int v) { return v; }
inline float fastAtan2(float y, float x) { return orc_fast_atan2(y, x); }

/* ---- small value types ---- */
template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T _x, T _y) : x(_x), y(_y) {}
    Point_& operator*=(float s) { x = (T)(x * s); y = (T)(y * s); return *this; }   /* Point2f: plain float products */
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;

template <typename T> struct Size_ {
    T width, height;
    Size_() : width(0), height(0) {}
    Size_(T w, T h) : width(w), height(h) {}
};
typedef Size_<int> Size;

template <typename T> struct Rect_ {
    T x, y, width, height;
    Rect_() : x(0), y(0), width(0), height(0) {}
    Rect_(T _x, T _y, T w, T h) : x(_x), y(_y), width(w), height(h) {}
};
typedef Rect_<int> Rect;

struct Scalar {
    double val[4];
    Scalar() { val[0] = val[1] = val[2] = val[3] = 0; }
    double& operator[](int i) { return val[i]; }
    const double& operator[](int i) const { return val[i]; }
};

/* cv::KeyPoint with OpenCV's defaults */
class KeyPoint {
public:
    KeyPoint() : pt(0, 0), size(0), angle(-1), response(0), octave(0), class_id(-1) {}
    KeyPoint(Point2f _pt, float _size, float _angle = -1, float _response = 0, int _octave = 0, int _class_id = -1)
        : pt(_pt), size(_size), angle(_angle), response(_response), octave(_octave), class_id(_class_id) {}
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
};

enum BorderTypes { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4,
                   BORDER_REFLECT101 = 4, BORDER_DEFAULT = 4, BORDER_ISOLATED = 16 };

/* ---- Mat: CV_8UC1, 2-D, reference-counted storage ---- */
struct MatStep {
    size_t v;
    MatStep() : v(0) {}
    operator size_t() const { return v; }
};

struct ZerosExpr { int rows, cols, type; };   /* what Mat::zeros returns (OpenCV: a MatExpr) */

class Mat {
public:
    int rows, cols;
    uchar* data;
    MatStep step;

    Mat() : rows(0), cols(0), data(nullptr) {}
    Mat(int r, int c, int type) : rows(0), cols(0), data(nullptr) { create(r, c, type); }
    Mat(Size sz, int type) : rows(0), cols(0), data(nullptr) { create(sz.height, sz.width, type); }
    /* a header over memory the caller owns (no copy), as OpenCV's Mat(rows, cols, type, data, step) */
    Mat(int r, int c, int type, void* ext, size_t stride) : rows(r), cols(c), data((uchar*)ext)
    {
        CV_Assert(type == CV_8UC1 && r >= 0 && c >= 0 && stride >= (size_t)c);
        step.v = stride;
        whole_rows_ = r; whole_cols_ = c; base_ = data;
    }
    Mat(const ZerosExpr& e) : rows(0), cols(0), data(nullptr) { *this = e; }

    /* "If the array already has the specified size and type, the method does nothing", else new storage */
    void create(int r, int c, int type)
    {
        CV_Assert(type == CV_8UC1 && r >= 0 && c >= 0);
        if (data && r == rows && c == cols) return;
        release();
        rows = r; cols = c; step.v = (size_t)c;
        buf_ = std::shared_ptr<uchar>(new uchar[(size_t)r * c + 1], std::default_delete<uchar[]>());
        data = base_ = buf_.get();
        whole_rows_ = r; whole_cols_ = c;
    }
    void create(Size sz, int type) { create(sz.height, sz.width, type); }
    void release() { buf_.reset(); data = base_ = nullptr; rows = cols = 0; step.v = 0; whole_rows_ = whole_cols_ = 0; }

    static ZerosExpr zeros(int r, int c, int type) { ZerosExpr e = {r, c, type}; return e; }
    /* assigning the zeros expression re-uses storage of the same size and type (create() above), so a view stays a view */
    Mat& operator=(const ZerosExpr& e)
    {
        create(e.rows, e.cols, e.type);
        for (int y = 0; y < rows; y++) std::memset(ptr(y), 0, (size_t)cols);
        return *this;
    }

    int type() const { return CV_8UC1; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    size_t step1() const { return step.v; }
    size_t elemSize() const { return 1; }
    Size size() const { return Size(cols, rows); }
    bool isSubmatrix() const { return rows != whole_rows_ || cols != whole_cols_; }
    bool isContinuous() const { return step.v == (size_t)cols || rows <= 1; }

    Mat clone() const
    {
        Mat m;
        m.create(rows, cols, CV_8UC1);
        for (int y = 0; y < rows; y++) std::memcpy(m.ptr(y), ptr(y), (size_t)cols);
        return m;
    }

    Mat operator()(const Rect& r) const
    {
        CV_Assert(0 <= r.x && 0 <= r.width && r.x + r.width <= cols && 0 <= r.y && 0 <= r.height && r.y + r.height <= rows);
        Mat m(*this);
        m.data = data + (size_t)r.y * step.v + r.x;
        m.rows = r.height; m.cols = r.width;
        return m;
    }
    Mat rowRange(int startrow, int endrow) const
    {
        CV_Assert(0 <= startrow && startrow <= endrow && endrow <= rows);
        return (*this)(Rect(0, startrow, cols, endrow - startrow));
    }
    Mat colRange(int startcol, int endcol) const
    {
        CV_Assert(0 <= startcol && startcol <= endcol && endcol <= cols);
        return (*this)(Rect(startcol, 0, endcol - startcol, rows));
    }

    uchar* ptr(int y = 0) { CV_Assert(data && 0 <= y && y < rows); return data + (size_t)y * step.v; }
    const uchar* ptr(int y = 0) const { CV_Assert(data && 0 <= y && y < rows); return data + (size_t)y * step.v; }

    template <typename T> T& at(int y, int x)
    {
        static_assert(sizeof(T) == 1, "cvshim Mat holds 8-bit elements only");
        CV_Assert(data && 0 <= y && y < rows && 0 <= x && x < cols);
        return *(T*)(data + (size_t)y * step.v + x);
    }
    template <typename T> const T& at(int y, int x) const
    {
        static_assert(sizeof(T) == 1, "cvshim Mat holds 8-bit elements only");
        CV_Assert(data && 0 <= y && y < rows && 0 <= x && x < cols);
        return *(const T*)(data + (size_t)y * step.v + x);
    }

private:
    std::shared_ptr<uchar> buf_;
    uchar* base_ = nullptr;                  /* first byte of the whole matrix this one is a view of */
    int whole_rows_ = 0, whole_cols_ = 0;
};

/* ---- argument proxies ---- */
class _InputArray {
public:
    _InputArray() : m_(nullptr) {}
    _InputArray(const Mat& m) : m_(const_cast<Mat*>(&m)) {}
    Mat getMat() const { return m_ ? *m_ : Mat(); }
    bool empty() const { return !m_ || m_->empty(); }
    int type() const { return CV_8UC1; }
    Size size() const { return m_ ? m_->size() : Size(); }
protected:
    Mat* m_;
};
class _OutputArray : public _InputArray {
public:
    _OutputArray() {}
    _OutputArray(Mat& m) : _InputArray(m) {}
    void create(int r, int c, int type) const { CV_Assert(m_); m_->create(r, c, type); }
    void create(Size sz, int type) const { create(sz.height, sz.width, type); }
    void release() const { if (m_) m_->release(); }
};
typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;
inline InputArray noArray() { static const _InputArray none; return none; }

/* ---- exact helpers ---- */
inline Scalar sum(InputArray _src)
{
    Mat src = _src.getMat();
    uint64_t s = 0;
    for (int y = 0; y < src.rows; y++) {
        const uchar* p = src.ptr(y);
        for (int x = 0; x < src.cols; x++) s += p[x];
    }
    Scalar r;
    r[0] = (double)s;        /* exact: an 8-bit image would need 2^45 pixels to leave the 53-bit mantissa */
    return r;
}

inline int borderInterpolate101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

/* copyMakeBorder, BORDER_REFLECT_101 with or without BORDER_ISOLATED.  src may be the view inside dst that the border is put
 * around (ComputePyramid does that).  Without BORDER_ISOLATED OpenCV takes the pixels around a sub-matrix from its parent; that
 * case is not needed here and is refused rather than answered differently. */
inline void copyMakeBorder(InputArray _src, OutputArray _dst, int top, int bottom, int left, int right, int borderType)
{
    Mat src = _src.getMat();
    CV_Assert(top >= 0 && bottom >= 0 && left >= 0 && right >= 0 && !src.empty());
    const bool isolated = (borderType & BORDER_ISOLATED) != 0;
    CV_Assert((borderType & ~BORDER_ISOLATED) == BORDER_REFLECT_101);
    CV_Assert(isolated || !src.isSubmatrix());
    _dst.create(src.rows + top + bottom, src.cols + left + right, src.type());
    Mat dst = _dst.getMat();
    for (int y = 0; y < src.rows; y++) {
        uchar* d = dst.ptr(y + top);
        const uchar* s = src.ptr(y);
        if (d + left != s) std::memmove(d + left, s, (size_t)src.cols);
        for (int x = 0; x < left; x++) d[x] = d[left + borderInterpolate101(x - left, src.cols)];
        for (int x = 0; x < right; x++) d[left + src.cols + x] = d[left + borderInterpolate101(src.cols + x, src.cols)];
    }
    for (int y = 0; y < top; y++)
        std::memcpy(dst.ptr(y), dst.ptr(top + borderInterpolate101(y - top, src.rows)), (size_t)dst.cols);
    for (int y = 0; y < bottom; y++)
        std::memcpy(dst.ptr(top + src.rows + y), dst.ptr(top + borderInterpolate101(src.rows + y, src.rows)), (size_t)dst.cols);
}

}  // namespace cv

#endif
