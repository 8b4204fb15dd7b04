"""The AirSim driver's call contract of the introspection network (Examples/Stereo/stereo_airsim.cc:386-411): u8 cv::resize of the
image to 512x512, forward, u8 map, u8 cv::resize back to the image size -- ivf_fcn_forward_resized / _device_resized against the
composition of the oracle's resize with the existing forward, against the numpy oracle of the network, and feeding the front end."""
import numpy as np
import pytest

import fcn_common as FC
import oracle_lib as O
from iv_slam_amd import fcn_weights, synth

pytestmark = pytest.mark.gpu

BF, B = 386.1448, 386.1448 / 718.856


@pytest.fixture(scope="module")
def iv():
    import iv_slam_amd
    lib = iv_slam_amd.load()
    assert lib.ivf_device_count() >= 1, "no HIP device: libivfront has no CPU fallback"
    return iv_slam_amd


def resize3(img, w, h):
    return np.stack([O.resize_linear(np.ascontiguousarray(img[..., c]), w, h) for c in range(3)], axis=-1)


@pytest.fixture(scope="module")
def kitti_case(iv):
    W = fcn_weights.make_seeded_weights(7)
    fcn = iv.IntrospectionFCN(fcn_weights.pack_blob(W), (512, 512), (512, 512))
    bgr = FC.bgr_image(1242, 375, 57)
    return W, fcn, bgr


def test_host_call_equals_the_host_composition(iv, kitti_case):
    W, fcn, bgr = kitti_case
    got = fcn.forward_resized(bgr, (1242, 375))
    small = resize3(bgr, 512, 512)
    want = O.resize_linear(fcn(small), 1242, 375)
    assert got.shape == (375, 1242) and np.array_equal(got, want)
    # a padded source view gives the same map; the tables of this geometry are reused
    big = np.zeros((375, 1242 + 11, 3), np.uint8); big[:, :1242] = bgr
    assert np.array_equal(fcn.forward_resized(big[:, :1242], (1242, 375)), want)


def test_host_call_against_the_numpy_oracle(iv, kitti_case):
    import fcn_oracle
    W, fcn, bgr = kitti_case
    small = resize3(bgr, 512, 512)
    oc, ou8 = fcn_oracle.forward(W, small, (512, 512))
    u8, cost = fcn(small, want_f32=True)                      # the network step of the resized call (byte-equal: test above)
    assert np.abs(cost - oc).max() < 3e-4
    got = fcn.forward_resized(bgr, (1242, 375))
    want = O.resize_linear(ou8, 1242, 375)
    d = np.abs(got.astype(int) - want.astype(int))
    assert d.max() <= 1 and (d != 0).mean() < 0.01


def test_device_batch_into_the_front_ends_cost_plane(iv):
    """stereo_airsim.cc:386-411 for a batch of 3, written straight into the front end's cost plane (ivf_frontend_cost_plane) and consumed
    by run_color: the plane equals a contiguous output of the same call, the results equal a front end fed those maps through run(), and
    one pair equals the oracle extractor on its map"""
    import torch
    w, h, n, pairs = 640, 240, 400, 3
    dev = torch.device("cuda:0")
    fcn = iv.IntrospectionFCN(fcn_weights.pack_blob(fcn_weights.make_seeded_weights(11)), (512, 512), (512, 512), max_batch=pairs)
    fe = iv.StereoFrontend(w, h, pairs, nfeatures=n, enableIntrospection=True, bf=BF, b=B)
    ref_fe = iv.StereoFrontend(w, h, pairs, nfeatures=n, enableIntrospection=True, bf=BF, b=B)
    st = torch.cuda.current_stream(dev)
    stream = synth.make_stream(pairs, w, h, seed=300)
    L = torch.from_numpy(stream[:, 0].copy()).to(dev); R = torch.from_numpy(stream[:, 1].copy()).to(dev)
    bgr = torch.stack([L, L // 2 + 40, 255 - L // 2], dim=-1).contiguous()
    plane = fe.cost_plane(pairs, st.cuda_stream)
    assert not plane.is_contiguous() and tuple(plane.shape) == (pairs, h, w)
    fcn.forward_device_resized(bgr, plane, (w, h), st.cuda_stream)
    fe.run_color(L, R, plane, st.cuda_stream)
    cost = torch.empty((pairs, h, w), dtype=torch.uint8, device=dev)
    fcn.forward_device_resized(bgr, cost, (w, h), st.cuda_stream)
    ref_fe.run(L, R, cost, st.cuda_stream)
    fe.sync(); ref_fe.sync(); torch.cuda.synchronize()
    fcn.status(st.cuda_stream)
    assert torch.equal(plane, cost)
    hc = cost.cpu().numpy()
    assert not np.array_equal(hc[0], hc[1])
    # image 0 of the batch is the host call's image, up to the batch schedule of the network (test_gpu_fcn.py: <= 1 u8 step at 512x512,
    # which the u8 resize can round into 2 at most)
    single = fcn.forward_resized(bgr[0].cpu().numpy(), (w, h))
    d = np.abs(single.astype(int) - hc[0].astype(int))
    assert d.max() <= 2 and (d != 0).mean() < 0.01
    for p in range(pairs):
        for side in (0, 1):
            a = fe.fetch(p, side); b_ = ref_fe.fetch(p, side)
            assert a["kps"].tobytes() == b_["kps"].tobytes(), (p, side)
            assert np.array_equal(a["desc"], b_["desc"]) and np.array_equal(a["quality"], b_["quality"])
    okL, odL = O.Extractor(n, 1.2, 8, 20, 7, introspection=True)(stream[1, 0], hc[1])
    r = fe.fetch(1, 0)
    assert r["kps"].tobytes() == okL.tobytes() and np.array_equal(r["desc"], odL)
    assert len(okL) > 100


def test_non_square_out_and_other_destination(iv):
    """out = 256x256 (the network's map is upsampled to 256x256, then resized in u8 to a destination that is not the source size)"""
    import torch
    fcn = iv.IntrospectionFCN(fcn_weights.pack_blob(fcn_weights.make_seeded_weights(5)), (512, 512), (256, 256), max_batch=2)
    bgr = FC.bgr_image(1920, 1200, 61)
    got = fcn.forward_resized(bgr, (960, 600))
    want = O.resize_linear(fcn(resize3(bgr, 512, 512)), 960, 600)
    assert got.shape == (600, 960) and np.array_equal(got, want)
    # the device path at batch 1 is the host path's computation
    dev = torch.device("cuda:0")
    out = torch.zeros((1, 600, 960), dtype=torch.uint8, device=dev)
    fcn.forward_device_resized(torch.from_numpy(bgr[None]).to(dev), out, (960, 600))
    torch.cuda.synchronize()
    fcn.status()
    assert np.array_equal(out[0].cpu().numpy(), want)


def test_resized_argument_validation(iv):
    import ctypes as C
    import torch
    from iv_slam_amd import _lib
    lib = _lib.load()
    fcn = iv.IntrospectionFCN(fcn_weights.pack_blob(fcn_weights.make_seeded_weights(5)), (512, 512), (512, 512), max_batch=2)
    dev = torch.device("cuda:0")
    src = torch.zeros((3, 100, 120, 3), dtype=torch.uint8, device=dev); dst = torch.zeros((3, 50, 60), dtype=torch.uint8, device=dev)
    s, d = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    assert lib.ivf_fcn_forward_device_resized(fcn._h, s, 120, 100, 36000, 360, 3, d, 60, 50, 3000, 60, None) == _lib.IVF_E_INVALID  # n > max_batch
    assert lib.ivf_fcn_forward_device_resized(fcn._h, s, 120, 100, 36000, 359, 2, d, 60, 50, 3000, 60, None) == _lib.IVF_E_INVALID
    assert lib.ivf_fcn_forward_device_resized(fcn._h, s, 120, 100, 36000, 360, 2, d, 60, 50, 3000, 59, None) == _lib.IVF_E_INVALID
    assert lib.ivf_fcn_forward_device_resized(fcn._h, s, 120, 100, 36000, 360, 2, d, 60, 50, 2000, 60, None) == _lib.IVF_E_INVALID
    assert lib.ivf_fcn_forward_device_resized(fcn._h, s, 0, 100, 36000, 360, 2, d, 60, 50, 3000, 60, None) == _lib.IVF_E_INVALID
    img = np.zeros((100, 120, 3), np.uint8); out = np.zeros((50, 60), np.uint8)
    assert lib.ivf_fcn_forward_resized(fcn._h, _lib.ptr(img), 120, 100, 359, _lib.ptr(out), 60, 50, 60) == _lib.IVF_E_INVALID
    assert lib.ivf_fcn_forward_resized(fcn._h, _lib.ptr(img), 120, 100, 360, _lib.ptr(out), 60, 50, 59) == _lib.IVF_E_INVALID
    assert lib.ivf_fcn_forward_device_resized(fcn._h, s, 120, 100, 36000, 360, 2, d, 60, 50, 3000, 60, None) == _lib.IVF_OK
    torch.cuda.synchronize()
    fcn.status()
