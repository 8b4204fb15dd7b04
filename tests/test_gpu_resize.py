"""GPU parity of cv::resize INTER_LINEAR on 8-bit images (ivf_resize_*, k_resize) against the CPU oracle's restatement of
OpenCV's fixed-point path (orc_resize_linear_8u).  Bar: bit-exact, 1 and 3 interleaved channels, any geometry."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from iv_slam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def iv():
    import iv_slam_amd
    lib = iv_slam_amd.load()
    assert lib.ivf_device_count() >= 1, "no HIP device: libivfront has no CPU fallback"
    return iv_slam_amd


def image(w, h, channels, seed):
    if channels == 1:
        return synth.make_left(w, h, seed=seed, idx=0) if w >= 16 and h >= 16 else \
            np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    planes = [image(w, h, 1, seed + 17 * c) for c in range(3)]
    return np.stack(planes, axis=-1)


def oracle_resize(img, dw, dh):
    if img.ndim == 2:
        return O.resize_linear(np.ascontiguousarray(img), dw, dh)
    return np.stack([O.resize_linear(np.ascontiguousarray(img[..., c]), dw, dh) for c in range(img.shape[2])], axis=-1)


GEOMS = [((1242, 375), (512, 512)), ((1920, 1200), (512, 512)), ((640, 480), (512, 512)),
         ((512, 512), (1242, 375)), ((512, 512), (1920, 1200)),
         ((320, 200), (512, 512)), ((1024, 1024), (512, 512)), ((640, 480), (640, 480)),
         ((7, 5), (3, 11)), ((1, 1), (4, 4)), ((5, 1), (1, 7))]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("src,dst", GEOMS)
def test_resize_matches_oracle(iv, src, dst, channels):
    img = image(src[0], src[1], channels, seed=3 + src[0] + dst[1])
    got = iv.Resize(src, dst, channels)(img)
    want = oracle_resize(img, dst[0], dst[1])
    assert got.shape == want.shape and np.array_equal(got, want)


def test_exact_2x_is_the_area_average(iv):
    """OpenCV runs an exact 2x INTER_LINEAR downscale as INTER_AREA: (a + b + c + d + 2) >> 2 -- the same bytes as the linear rule"""
    img = image(1024, 1024, 1, seed=9).astype(np.int32)
    area = ((img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert np.array_equal(iv.resize_linear(img.astype(np.uint8), (512, 512)), area)


@pytest.mark.parametrize("channels", [1, 3])
def test_host_call_with_padded_strides(iv, channels):
    src, dst = (1242, 375), (512, 512)
    img = image(*src, channels, seed=21)
    tail = (3,) if channels == 3 else ()
    big = np.full((src[1], src[0] + 37) + tail, 7, np.uint8)
    big[:, :src[0]] = img
    out_big = np.full((dst[1], dst[0] + 13) + tail, 99, np.uint8)
    r = iv.Resize(src, dst, channels)
    r(big[:, :src[0]], out=out_big[:, :dst[0]])
    assert np.array_equal(out_big[:, :dst[0]], oracle_resize(img, *dst))
    assert (out_big[:, dst[0]:] == 99).all()                  # the padding is not written
    # the reverse direction (the cost map back to the image size)
    back = iv.Resize(dst, src, channels)(out_big[:, :dst[0]])
    assert np.array_equal(back, oracle_resize(oracle_resize(img, *dst), *src))


@pytest.mark.parametrize("channels", [1, 3])
def test_device_batch_in_padded_views(iv, channels):
    import torch
    dev = torch.device("cuda:0")
    src, dst, n = (1242, 375), (512, 512), 5
    tail = (3,) if channels == 3 else ()
    imgs = np.stack([image(*src, channels, seed=40 + i) for i in range(n)])
    big = torch.full((n, src[1] + 3, src[0] + 29) + tail, 5, dtype=torch.uint8, device=dev)
    view = big[:, 1:1 + src[1], 2:2 + src[0]]
    view.copy_(torch.from_numpy(imgs).to(dev))
    obig = torch.full((n, dst[1] + 2, dst[0] + 64) + tail, 77, dtype=torch.uint8, device=dev)
    oview = obig[:, :dst[1], 16:16 + dst[0]]
    r = iv.Resize(src, dst, channels)
    r.apply_device(view, out=oview)
    contiguous = r.apply_device(view.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(oview, contiguous)
    host = oview.cpu().numpy()
    for i in range(n):
        assert np.array_equal(host[i], r(imgs[i])), i
        assert np.array_equal(host[i], oracle_resize(imgs[i], *dst)), i
    assert not np.array_equal(host[0], host[1])
    keep = obig.clone(); keep[:, :dst[1], 16:16 + dst[0]] = 77
    assert (keep == 77).all()                                  # nothing outside the views is written


def test_invalid_arguments(iv):
    from iv_slam_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ivf_resize_create(64, 48, 32, 24, 2, 0, C.byref(h)) == _lib.IVF_E_INVALID
    assert b"channels" in lib.ivf_last_error()
    assert lib.ivf_resize_create(64, 48, 32, 24, 1, 99, C.byref(h)) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_create(70000, 48, 32, 24, 1, 0, C.byref(h)) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_create(64, 48, 32, 24, 3, 0, C.byref(h)) == _lib.IVF_OK and h.value
    src = np.zeros((48, 64, 3), np.uint8); dst = np.zeros((24, 32, 3), np.uint8)
    p = _lib.ptr
    assert lib.ivf_resize_apply(h, p(src), 64 * 3 - 1, p(dst), 32 * 3) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_apply(h, p(src), 64 * 3, p(dst), 32 * 3 - 1) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_apply(h, p(src), 64 * 3, p(dst), 32 * 3) == _lib.IVF_OK
    import torch
    d = torch.zeros((2, 48, 64, 3), dtype=torch.uint8, device="cuda:0"); o = torch.zeros((2, 24, 32, 3), dtype=torch.uint8, device="cuda:0")
    args = [C.c_void_p(d.data_ptr()), 64 * 3, 64 * 3 * 48, C.c_void_p(o.data_ptr()), 32 * 3, 32 * 3 * 24]
    assert lib.ivf_resize_apply_device(h, *args, 0, None) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_apply_device(h, *args[:2], 100, *args[3:], 2, None) == _lib.IVF_E_INVALID     # images overlap
    assert lib.ivf_resize_apply_device(h, *args[:4], 32 * 3 - 3, args[5], 2, None) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_apply_device(h, *args, 2, None) == _lib.IVF_OK
    torch.cuda.synchronize()
    lib.ivf_resize_destroy(h)
