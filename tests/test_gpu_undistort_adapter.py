"""The C++ adapter's ivf::UndistortKeyPoints / ivf::ComputeImageBounds (include/ivfront_orbslam.hpp; Frame.cc:696-756) compiled against
the mock cv types by tests/adapter/undistort_driver.cpp and RUN: its output equals the Python binding's, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_undistort import as_ref, load_camera, random_keypoints, seeded_camera8
import undistort_ref as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("undistort_adapter") / "undistort_driver")
    lib_dir = os.path.join(ROOT, "iv_slam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cv_mock"), os.path.join(ROOT, "tests", "adapter", "undistort_driver.cpp"),
                           "-o", exe, "-L", lib_dir, "-livfront", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_driver(driver, tmp_path, cam, w, h, kps):
    from iv_slam_amd._lib import KP_DTYPE
    (tmp_path / "s.bin").write_bytes(struct.pack("<4i4f", w, h, len(cam.dist), len(kps), cam.fx, cam.fy, cam.cx, cam.cy) +
                                     cam.dist.astype(np.float32).tobytes() + kps.tobytes())
    r = subprocess.run([driver, str(tmp_path / "s.bin"), str(tmp_path / "r.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = (tmp_path / "r.bin").read_bytes()
    assert len(blob) == len(kps) * 24 + 16
    return np.frombuffer(blob[:len(kps) * 24], KP_DTYPE), np.frombuffer(blob[len(kps) * 24:], np.float32)


@pytest.mark.parametrize("name", ["TUM1", "EuRoC", "seeded8", "no_k1"])
def test_adapter_equals_the_python_binding(driver, tmp_path, name):
    import iv_slam_amd
    from iv_slam_amd.camera import Camera
    assert iv_slam_amd.load().ivf_device_count() >= 1
    cam = {"seeded8": seeded_camera8, "no_k1": lambda: Camera(517.3, 516.5, 318.6, 255.3, [0.0, -0.95, -0.005, 0.0026, 1.16])}.get(
        name, lambda: load_camera(name))()
    w, h = (752, 480) if name == "EuRoC" else (640, 480)
    for n in (0, 1, 1000):
        kps = random_keypoints(n, w, h, seed=40 + n)
        got, bounds = run_driver(driver, tmp_path, cam, w, h, kps)
        assert got.tobytes() == cam.undistort_keypoints(kps).tobytes()
        assert got.tobytes() == U.undistort_keypoints(as_ref(cam), kps).tobytes()
        assert bounds.tobytes() == np.array(cam.image_bounds(w, h), np.float32).tobytes()
        if name == "no_k1":
            assert got.tobytes() == kps.tobytes() and bounds.tolist() == [0.0, 0.0, float(w), float(h)]
