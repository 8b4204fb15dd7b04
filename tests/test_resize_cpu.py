"""CPU-side checks of the cv::resize (INTER_LINEAR, 8-bit) axis rule behind ivf_resize and the extractor's pyramid
(ivf_resize_axis_table: host only, no device).  The kernels themselves are checked in test_gpu_resize.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

F = np.float32


def numpy_axis_table(ssize, dsize):
    """OpenCV resize.cpp's INTER_LINEAR table restated: scale = 1. / ((double)dsize / ssize), f = (float)((d + 0.5) * scale - 0.5),
    s = cvFloor(f), 11-bit coefficients saturate_cast<short>((1 - (f - s)) * 2048) / ((f - s) * 2048); rows clip(s), clip(s + 1)."""
    scale = 1.0 / (float(dsize) / ssize)
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    fr = (f - s.astype(F)).astype(F)
    w0 = np.rint((F(1) - fr) * F(2048)).clip(-32768, 32767).astype(np.int16)
    w1 = np.rint(fr * F(2048)).clip(-32768, 32767).astype(np.int16)
    return np.clip(s, 0, ssize - 1).astype(np.int32), np.clip(s + 1, 0, ssize - 1).astype(np.int32), w0, w1


PAIRS = [(1242, 512), (375, 512), (1920, 512), (1200, 512), (512, 1242), (512, 375), (512, 1920), (512, 1200),
         (1024, 512), (512, 1024), (512, 512), (1, 1), (1, 4), (5, 1), (7, 3), (5, 11), (2, 3), (320, 512), (200, 512),
         (640, 512), (480, 512), (3, 4096), (4095, 16), (22233, 3072)]


@pytest.mark.parametrize("ssize,dsize", PAIRS)
def test_axis_table_matches_the_numpy_rule(ssize, dsize):
    from iv_slam_amd import rectify
    got = rectify.resize_axis_table(ssize, dsize)
    want = numpy_axis_table(ssize, dsize)
    for g, w, name in zip(got, want, ("idx0", "idx1", "w0", "w1")):
        assert np.array_equal(g, w), "%s of %d -> %d" % (name, ssize, dsize)


def test_upscaled_top_rows_read_row_zero_twice():
    """375 -> 512 vertically: the first rows have s = -1; cv::resize reads clip(-1) = 0 and clip(0) = 0 there, with the unclipped
    coefficients -- not rows 0 and 1 (what a table holding only clip(s) and a reader taking the next row would give)"""
    from iv_slam_amd import rectify
    i0, i1, w0, w1 = rectify.resize_axis_table(375, 512)
    top = np.flatnonzero((np.arange(512) + 0.5) * (375 / 512) - 0.5 < 0)
    assert len(top) >= 1
    assert (i0[top] == 0).all() and (i1[top] == 0).all()
    assert (w1[top] > 0).all()                  # coefficients are not clipped: the two taps split the weight
    assert i1[top[-1] + 1] == 1
    # last rows of an upscale: s = ssize - 1 reads the last row twice
    assert i0[-1] == 374 and i1[-1] == 374


def test_scale_is_the_inverse_of_the_inverse():
    """a pair for which (double)ssize / dsize and 1. / ((double)dsize / ssize) give different coefficient tables: the library follows
    cv::resize (the latter)"""
    from iv_slam_amd import rectify
    O.lib.orc_resize_coef_mismatches.restype = C.c_int
    O.lib.orc_resize_coef_mismatches.argtypes = [C.c_int, C.c_int]
    ssize, dsize = 22233, 3072
    assert O.lib.orc_resize_coef_mismatches(ssize, dsize) > 0
    got = rectify.resize_axis_table(ssize, dsize)
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * (float(ssize) / dsize) - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    fr = (f - s.astype(F)).astype(F)
    naive = (np.clip(s, 0, ssize - 1), np.rint((F(1) - fr) * F(2048)).astype(np.int16), np.rint(fr * F(2048)).astype(np.int16))
    assert not all(np.array_equal(g, w) for g, w in zip((got[0], got[2], got[3]), naive))
    assert all(np.array_equal(g, w) for g, w in zip(got, numpy_axis_table(ssize, dsize)))


def _pyramid_sizes(w, h, scale_factor=1.2, nlevels=8):
    inv = O.Extractor(1000, scale_factor, nlevels, 20, 7).tables()["inv_scale"]
    return ([O.lib.orc_cv_round_f(float(F(w) * s)) for s in inv], [O.lib.orc_cv_round_f(float(F(h) * s)) for s in inv])


@pytest.mark.parametrize("w,h", [(1242, 375), (1920, 1200)])
def test_pyramid_pairs_read_the_next_row(w, h):
    """the extractor's pyramid packs only idx0 and pyr_tile reads rows idx0 and min(idx0 + 1, ssize - 1): for every level pair of the
    benchmark sizes that is the table's second row on both axes, so the shared table leaves the pyramid where it was"""
    from iv_slam_amd import rectify
    ws, hs = _pyramid_sizes(w, h)
    assert ws[0] == w and hs[0] == h and len(set(ws)) == 8
    for l in range(1, 8):
        for ssize, dsize in ((ws[l - 1], ws[l]), (hs[l - 1], hs[l])):
            i0, i1, w0, w1 = rectify.resize_axis_table(ssize, dsize)
            assert np.array_equal(i1, np.minimum(i0 + 1, ssize - 1)), (l, ssize, dsize)
            assert (i0 <= ssize - 1).all() and (i0 >= 0).all()


def test_axis_table_argument_validation():
    from iv_slam_amd import _lib
    lib = _lib.load()
    a = np.zeros(4, np.int32); b = np.zeros(4, np.int16)
    p = _lib.ptr
    assert lib.ivf_resize_axis_table(0, 4, p(a), p(a), p(b), p(b)) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_axis_table(4, 0, p(a), p(a), p(b), p(b)) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_axis_table(65537, 4, p(a), p(a), p(b), p(b)) == _lib.IVF_E_INVALID
    assert b"65536" in lib.ivf_last_error()
    assert lib.ivf_resize_axis_table(4, 4, None, p(a), p(b), p(b)) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_axis_table(65536, 4, p(a), p(a), p(b), p(b)) == _lib.IVF_OK


def test_handle_argument_validation():
    """checked before any device is looked for: the same answer with and without a GPU"""
    from iv_slam_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    for args in ((1242, 375, 512, 512, 2), (1242, 375, 512, 512, 4), (0, 375, 512, 512, 3), (1242, 375, 512, 0, 1),
                 (70000, 375, 512, 512, 1), (1242, 65537, 512, 512, 3)):
        assert lib.ivf_resize_create(*args, 0, C.byref(h)) == _lib.IVF_E_INVALID, args
        assert not h.value
    assert lib.ivf_resize_create(8, 8, 4, 4, 1, 0, None) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_apply(None, None, 8, None, 4) == _lib.IVF_E_INVALID
    assert lib.ivf_resize_apply_device(None, None, 8, 64, None, 4, 16, 1, None) == _lib.IVF_E_INVALID
    assert lib.ivf_fcn_forward_resized(None, None, 8, 8, 24, None, 8, 8, 8) == _lib.IVF_E_INVALID
    assert lib.ivf_fcn_forward_device_resized(None, None, 8, 8, 192, 24, 1, None, 8, 8, 64, 8, None) == _lib.IVF_E_INVALID
    lib.ivf_resize_destroy(None)
