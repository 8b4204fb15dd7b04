"""undistort_ref.py -- TEST-SIDE RESTATEMENT (test infrastructure only) of cv::undistortPoints(src, dst, K, D, cv::Mat(), K) as
Frame::UndistortKeyPoints and Frame::ComputeImageBounds call it (ORB/src/Frame.cc:696-726, :728-756), written from the definition
in DESIGN.md A-14 and not from the kernel: plain Python floats, i.e. IEEE double, one rounding per operation, never fused; the only
float32 steps are the widening of K, D and the point on the way in and the narrowing of the result on the way out.

OpenCV is un-vendored and unpinned in the reference, so this is the library's FROZEN definition (OpenCV 4.x, plain C++ path), like
the other OpenCV primitives; parity with a particular OpenCV build is not claimed.
"""
import numpy as np

F = np.float32


def widen(cam):
    """(fx, fy, cx, cy, k[12]) as Python floats from float32 inputs; cam = (fx, fy, cx, cy, dist) with 0, 4, 5, 8 or 12 coefficients."""
    fx, fy, cx, cy, dist = cam
    dist = [float(F(v)) for v in np.asarray(dist, np.float32).ravel()]
    if len(dist) not in (0, 4, 5, 8, 12):
        raise ValueError("distortion vector of %d coefficients" % len(dist))
    return float(F(fx)), float(F(fy)), float(F(cx)), float(F(cy)), dist + [0.0] * (12 - len(dist))


def undistort_point(cam, px, py, iterations=5):
    """one point (float32 in, float32 out); `iterations` = 5 is the definition, other values only serve the convergence tests"""
    fx, fy, cx, cy, k = widen(cam)
    ifx = 1.0 / fx
    ify = 1.0 / fy
    u = float(F(px))
    v = float(F(py))
    x = (u - cx) * ifx
    y = (v - cy) * ify
    x0 = x
    y0 = y
    for _ in range(iterations):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        if icdist < 0:
            x = (u - cx) * ifx
            y = (v - cy) * ify
            break
        dX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - dX) * icdist
        y = (y0 - dY) * icdist
    xx = fx * x + 0.0 * y + cx
    yy = 0.0 * x + fy * y + cy
    ww = 1.0 / (0.0 * x + 0.0 * y + 1.0)
    return F(xx * ww), F(yy * ww)


def switched_on(cam):
    """mDistCoef.at<float>(0) != 0.0: the reference's only test (Frame.cc:698, :730)"""
    dist = np.asarray(cam[4], np.float32).ravel()
    return len(dist) > 0 and bool(dist[0] != 0)


def undistort_keypoints(cam, kps, iterations=5):
    """Frame::UndistortKeyPoints on a structured keypoint array (fields x, y, ...): only pt changes (Frame.cc:721-724)"""
    out = np.array(kps, copy=True)
    if not switched_on(cam):
        return out
    for i in range(len(out)):
        out["x"][i], out["y"][i] = undistort_point(cam, kps["x"][i], kps["y"][i], iterations)
    return out


def undistort_xy(cam, xy, iterations=5):
    """[n][2] float32 points -> [n][2] float32, always through the iteration (no k1 short cut)"""
    xy = np.asarray(xy, np.float32)
    return np.array([undistort_point(cam, p[0], p[1], iterations) for p in xy], np.float32).reshape(-1, 2)


def image_bounds(cam, width, height):
    """Frame::ComputeImageBounds (Frame.cc:728-756) -> (min_x, min_y, max_x, max_y) float32"""
    if not switched_on(cam):
        return F(0.0), F(0.0), F(width), F(height)
    p = [undistort_point(cam, F(a), F(b)) for a, b in ((0, 0), (width, 0), (0, height), (width, height))]
    return min(p[0][0], p[2][0]), min(p[0][1], p[1][1]), max(p[1][0], p[3][0]), max(p[2][1], p[3][1])


def distort_point(cam, x, y):
    """the forward model (pixel coordinates of the ideal point -> distorted pixel), double: the round-trip check of the tests"""
    fx, fy, cx, cy, k = widen(cam)
    x = (float(x) - cx) / fx
    y = (float(y) - cy) / fy
    r2 = x * x + y * y
    cdist = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * cdist + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
    yd = y * cdist + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
    return fx * xd + cx, fy * yd + cy


def seeded_points(width, height, n=4000, seed=1):
    """n seeded integer points in [19, w-19) x [19, h-19): where an extractor can place a level-0 keypoint"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(19, width - 19, n), rng.integers(19, height - 19, n)], axis=1).astype(np.float32)
