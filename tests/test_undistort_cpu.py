"""Frame::UndistortKeyPoints / Frame::ComputeImageBounds (ORB/src/Frame.cc:696-756) without a GPU: the test-side restatement's
known answers (tests/undistort_ref.py), the host-only ivf_image_bounds against it bit for bit, Settings.camera()
and argument validation.  The device kernel is compared with the same restatement in tests/test_gpu_undistort.py."""
import ctypes as C
import os

import numpy as np
import pytest

import undistort_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = os.path.join(ROOT, "tests", "golden", "settings")
F = np.float32

# name -> image size the reference's examples run these cameras at
CAMERAS = {"TUM1": (640, 480), "TUM2": (640, 480), "EuRoC": (752, 480)}
# Forward-model round trip of the five-iteration result on seeded_points(w, h, 4000, seed=1), measured with undistort_ref.py
# (px): the assertion allows 1.5 x the measured value -- room for another seed, not for another algorithm.
ROUND_TRIP_MEASURED = {"TUM1": 5.000e-3, "TUM2": 4.308e-4, "EuRoC": 0.2908}
# (min_x, min_y, max_x, max_y) float32, as both restatements (the issue's scratch one and undistort_ref.py) give them
BOUNDS = {"TUM1": (10.801185, 14.668615, 626.04785, 473.3119), "TUM2": (12.078635, 11.434566, 629.4173, 473.10013),
          "EuRoC": (-135.79564, -92.875015, 895.5073, 565.5531)}


def load_camera(name):
    from iv_slam_amd import kitti
    return kitti.Settings.load(os.path.join(SETTINGS, name + ".yaml")).camera()


def as_ref(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy, cam.dist)


def f32_bits(values):
    return np.asarray(values, np.float32).view(np.uint32)


def test_only_k1_switches_the_undistortion_on():
    """Frame.cc:698-702, :730, :749-755: k1 == 0 short-cuts whatever k2, p1, p2, k3 say"""
    cam = (F(517.3), F(516.5), F(318.6), F(255.3), [0.0, -0.95, -0.005, 0.0026, 1.16])
    from iv_slam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(3)
    kps = np.zeros(50, KP_DTYPE)
    kps["x"] = rng.uniform(0, 640, 50); kps["y"] = rng.uniform(0, 480, 50); kps["octave"] = rng.integers(0, 8, 50)
    assert U.undistort_keypoints(cam, kps).tobytes() == kps.tobytes()
    assert U.image_bounds(cam, 640, 480) == (0.0, 0.0, 640.0, 480.0)
    on = (cam[0], cam[1], cam[2], cam[3], [0.2] + cam[4][1:])
    assert U.undistort_keypoints(on, kps).tobytes() != kps.tobytes()
    un = U.undistort_keypoints(on, kps)
    for f in ("size", "angle", "response", "octave"):                 # only pt changes (:721-724)
        assert un[f].tobytes() == kps[f].tobytes()


def test_principal_point_is_a_fixed_point_without_tangential_terms():
    """with p1 = p2 = 0 a keypoint at a float-representable (cx, cy) has x = y = 0 in every iteration: it maps to itself exactly"""
    for dist in ([0.26, -0.95, 0.0, 0.0, 1.16], [-0.28, 0.07, 0.0, 0.0], [0.1, 0.2, 0.0, 0.0, 0.05, 0.01, 0.02, 0.03]):
        cam = (F(517.25), F(516.5), F(318.625), F(255.3125), dist)
        x, y = U.undistort_point(cam, F(318.625), F(255.3125))
        assert f32_bits([x, y]).tolist() == f32_bits([318.625, 255.3125]).tolist()


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_forward_model_round_trip(name):
    w, h = CAMERAS[name]
    cam = as_ref(load_camera(name))
    pts = U.seeded_points(w, h, 4000, seed=1)
    un = U.undistort_xy(cam, pts).astype(np.float64)
    worst = 0.0
    for (a, b), p in zip(un, pts.astype(np.float64)):
        xd, yd = U.distort_point(cam, a, b)
        worst = max(worst, float(np.hypot(xd - p[0], yd - p[1])))
    moved = float(np.hypot(*(un - pts).T).max())
    print("%s: round trip %.4g px (measured %.4g), keypoints move by up to %.1f px" % (name, worst, ROUND_TRIP_MEASURED[name], moved))
    assert worst <= 1.5 * ROUND_TRIP_MEASURED[name]
    assert moved > 5.0                                                    # the cameras do distort: the test is not about a no-op


def test_the_iteration_count_is_five():
    """EuRoC has not converged after five iterations, TUM2 has: an implementation that iterates to convergence is wrong on EuRoC"""
    worst = {}
    for name in ("EuRoC", "TUM2"):
        w, h = CAMERAS[name]
        cam = as_ref(load_camera(name))
        pts = U.seeded_points(w, h, 4000, seed=1)
        d = U.undistort_xy(cam, pts, 5).astype(np.float64) - U.undistort_xy(cam, pts, 50).astype(np.float64)
        worst[name] = float(np.hypot(*d.T).max())
        print("%s: 5 vs 50 iterations differ by up to %.4g px" % (name, worst[name]))
    assert worst["EuRoC"] > 0.1
    assert worst["TUM2"] < 0.01


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_image_bounds_equal_the_restatement(name):
    w, h = CAMERAS[name]
    cam = load_camera(name)
    got = cam.image_bounds(w, h)
    exp = U.image_bounds(as_ref(cam), w, h)
    print(name, "bounds", [float(v) for v in got])
    assert f32_bits(got).tolist() == f32_bits(exp).tolist()
    assert f32_bits(got).tolist() == f32_bits(BOUNDS[name]).tolist()
    if name == "EuRoC":
        assert got[0] < 0 and got[1] < 0                                 # a frame grid with a negative origin


def test_image_bounds_without_k1():
    from iv_slam_amd.camera import Camera
    for dist in ([], [0.0, 0.0, 0.0, 0.0], [0.0, -0.95, -0.005, 0.0026, 1.16]):
        cam = Camera(517.3, 516.5, 318.6, 255.3, dist)
        assert not cam.undistorts()
        got = cam.image_bounds(640, 480)
        assert f32_bits(got).tolist() == f32_bits([0, 0, 640, 480]).tolist()
        assert f32_bits(got).tolist() == f32_bits(U.image_bounds(as_ref(cam), 640, 480)).tolist()


def test_image_bounds_more_cameras_bit_for_bit():
    """seeded 4-, 5-, 8- and 12-coefficient cameras: the host text of the per-point function against the restatement"""
    from iv_slam_amd.camera import Camera
    rng = np.random.default_rng(11)
    for n in (4, 5, 8, 12):
        for _ in range(20):
            dist = np.zeros(n, np.float32)
            dist[:4] = rng.uniform(-1, 1, 4) * [0.3, 0.3, 0.005, 0.005]
            dist[4:] = rng.uniform(-0.05, 0.05, n - 4)
            cam = Camera(rng.uniform(400, 800), rng.uniform(400, 800), rng.uniform(300, 400), rng.uniform(200, 280), dist)
            w, h = int(rng.integers(320, 1300)), int(rng.integers(200, 600))
            assert f32_bits(cam.image_bounds(w, h)).tolist() == f32_bits(U.image_bounds(as_ref(cam), w, h)).tolist()


def test_settings_camera():
    """Tracking.cc:101-123: four float32 coefficients, a fifth only when Camera.k3 != 0"""
    from iv_slam_amd import kitti
    for name, n, k1 in (("TUM1", 5, 0.262383), ("TUM2", 5, 0.231222), ("EuRoC", 4, -0.28340811)):
        cam = load_camera(name)
        assert cam.dist.dtype == np.float32 and len(cam.dist) == n and cam.dist[0] == F(k1)
        assert cam.K.dtype == np.float32 and cam.K.shape == (3, 3) and cam.DistCoef.shape == (n, 1)
        assert cam.undistorts()
    S = kitti.Settings.load(os.path.join(SETTINGS, "TUM1.yaml"))
    cam = S.camera()
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == (F(517.306408), F(516.469215), F(318.643040), F(255.313989))
    assert cam.dist.tolist() == [F(0.262383), F(-0.953104), F(-0.005358), F(0.002628), F(1.163314)]
    assert cam.K[0, 0] == cam.fx and cam.K[1, 2] == cam.cy and cam.K[2, 2] == 1
    kc = kitti.Settings.load(os.path.join(SETTINGS, "KITTI00-02.yaml")).camera()
    assert kc.dist.tolist() == [0.0, 0.0, 0.0, 0.0] and not kc.undistorts()          # four zeros, no fifth coefficient
    assert kc.fx == F(718.856)


def test_bad_n_dist_is_refused():
    from iv_slam_amd import _lib
    lib = _lib.load()
    b = _lib.Bounds()
    kps = np.zeros(4, _lib.KP_DTYPE)
    for n in (-1, 1, 2, 3, 6, 7, 9, 11, 13, 14):
        cam = _lib.CameraC(); cam.fx = cam.fy = 500.0; cam.cx = 320.0; cam.cy = 240.0; cam.dist[0] = 0.1; cam.n_dist = n
        assert lib.ivf_image_bounds(C.byref(cam), 640, 480, C.byref(b)) == _lib.IVF_E_INVALID
        assert b"coefficients" in lib.ivf_last_error()
        assert lib.ivf_undistort_keypoints(C.byref(cam), _lib.ptr(kps), 4, _lib.ptr(kps), 0) == _lib.IVF_E_INVALID
        assert lib.ivf_undistort_keypoints_device(C.byref(cam), None, None, 0, 0, None, None) == _lib.IVF_E_INVALID
    cam = _lib.CameraC(); cam.fx = cam.fy = 500.0; cam.n_dist = 4
    assert lib.ivf_image_bounds(None, 640, 480, C.byref(b)) == _lib.IVF_E_INVALID
    assert lib.ivf_image_bounds(C.byref(cam), 0, 480, C.byref(b)) == _lib.IVF_E_INVALID
    assert lib.ivf_image_bounds(C.byref(cam), 640, 480, None) == _lib.IVF_E_INVALID
    # a camera that does not undistort copies, and n == 0 is fine: neither needs a device
    src = np.zeros(4, _lib.KP_DTYPE); src["x"] = [1, 2, 3, 4]; dst = np.zeros(4, _lib.KP_DTYPE)
    assert lib.ivf_undistort_keypoints(C.byref(cam), _lib.ptr(src), 4, _lib.ptr(dst), 0) == _lib.IVF_OK and dst.tobytes() == src.tobytes()
    cam.dist[0] = 0.1
    assert lib.ivf_undistort_keypoints(C.byref(cam), None, 0, None, 0) == _lib.IVF_OK
    with pytest.raises(ValueError):
        from iv_slam_amd.camera import Camera
        Camera(1, 1, 0, 0, np.zeros(14))
    with pytest.raises(ValueError):
        U.widen((1, 1, 0, 0, [0.1, 0.2]))
