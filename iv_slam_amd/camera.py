"""Camera model of a lens-distorted (non-rectified) camera: Frame::UndistortKeyPoints and Frame::ComputeImageBounds
(ORB/src/Frame.cc:696-726, :728-756) on top of ivf_image_bounds / ivf_undistort_keypoints (include/ivfront.h).

The reference holds mK and mDistCoef as CV_32F (ORB/src/Tracking.cc:106-123), so the values are kept as float32.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, Bounds, CameraC, check, ptr


class Camera:
    """fx, fy, cx, cy and dist = k1, k2, p1, p2[, k3[, k4, k5, k6[, s1, s2, s3, s4]]] (0, 4, 5, 8 or 12 values)."""

    def __init__(self, fx, fy, cx, cy, dist=()):
        self.fx, self.fy, self.cx, self.cy = (np.float32(v) for v in (fx, fy, cx, cy))
        self.dist = np.asarray(dist, np.float32).ravel().copy()
        if len(self.dist) > 12:
            raise ValueError("at most 12 distortion coefficients (tilt terms are not supported)")

    @property
    def K(self):
        """mK: 3x3 float32 (Tracking.cc:106-111)"""
        return np.array([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1]], np.float32)

    @property
    def DistCoef(self):
        """mDistCoef: [n][1] float32 (Tracking.cc:113-123)"""
        return self.dist.reshape(-1, 1).copy()

    def undistorts(self):
        """the reference's only test: mDistCoef.at<float>(0) != 0 (Frame.cc:698, :730)"""
        return len(self.dist) > 0 and bool(self.dist[0] != 0)

    def c_struct(self):
        c = CameraC()
        c.fx, c.fy, c.cx, c.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)
        for i, v in enumerate(self.dist):
            c.dist[i] = float(v)
        c.n_dist = len(self.dist)
        return c

    def image_bounds(self, width, height):
        """(mnMinX, mnMinY, mnMaxX, mnMaxY) as float32 (Frame::ComputeImageBounds, Frame.cc:728-756); host only."""
        b = Bounds()
        cam = self.c_struct()
        check(_lib.load().ivf_image_bounds(C.byref(cam), int(width), int(height), C.byref(b)))
        return tuple(np.float32(v) for v in (b.min_x, b.min_y, b.max_x, b.max_y))

    def undistort_keypoints(self, kps, device_id=0, out=None):
        """mvKeysUn of mvKeys (Frame::UndistortKeyPoints, Frame.cc:696-726): a KP_DTYPE array with pt undistorted on the device,
        every other field copied.  out: None = a new array, or a contiguous KP_DTYPE array of the same length (may be kps itself)."""
        k = np.ascontiguousarray(kps, KP_DTYPE)
        if out is None:
            out = np.empty(len(k), KP_DTYPE)
        assert out.dtype == KP_DTYPE and out.flags.c_contiguous and len(out) == len(k)
        cam = self.c_struct()
        check(_lib.load().ivf_undistort_keypoints(C.byref(cam), ptr(k), len(k), ptr(out), int(device_id)))
        return out

    def undistort_keypoints_device(self, kps_ptr, count_ptr, n_frames, cap, out_ptr, stream_ptr=None):
        """Frame::UndistortKeyPoints for [n_frames][cap] keypoints in device memory (raw pointers, e.g. tensor.data_ptr()) with
        per-frame int32 counts; slots past a count are not written; out_ptr may equal kps_ptr.  Asynchronous on the stream."""
        cam = self.c_struct()
        check(_lib.load().ivf_undistort_keypoints_device(C.byref(cam), kps_ptr, count_ptr, int(n_frames), int(cap), out_ptr, stream_ptr))
