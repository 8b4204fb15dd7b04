"""ctypes bindings for oracle/_ref/libivf_ref_orb.so (TEST INFRASTRUCTURE): the reference's own ORBextractor.cc, compiled
unmodified against oracle/cvshim/ by `make -C oracle ref` (oracle/ref_orb.cpp is the C ABI).  The library is never committed:
it exists where the reference tree was present at build time, and travels with the working tree from there.

`available()` says whether it can be used; `SKIP_REASON` why not.  A library built from other sources than those on disk is an
ImportError, not a skip: a stale checker must never pass for a current one."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import oracle_lib as O

ORACLE_DIR = O.ORACLE_DIR
REF = os.environ.get("IVF_REFERENCE", "/root/reference/introspective_ORB_SLAM")
SO = os.path.join(ORACLE_DIR, "_ref", "libivf_ref_orb.so")
_OURS = ["ref_orb.cpp", "cvshim/opencv2/core.hpp", "cvshim/opencv2/core/core.hpp", "cvshim/opencv2/highgui/highgui.hpp",
         "cvshim/opencv2/features2d/features2d.hpp", "cvshim/opencv2/imgproc/imgproc.hpp", "ivf_oracle.h"]
_THEIRS = [os.path.join(REF, "src", "ORBextractor.cc"), os.path.join(REF, "include", "ORBextractor.h")]
SKIP_REASON = "oracle/_ref/libivf_ref_orb.so is absent and so is the reference tree it is built from (%s)" % REF


def _sha(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _have_reference():
    return all(os.path.exists(p) for p in _THEIRS)


def _load():
    ours = [os.path.join(ORACLE_DIR, f) for f in _OURS]
    if _have_reference():
        srcs = ours + _THEIRS + [os.path.join(ORACLE_DIR, "libivf_oracle.so")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
            subprocess.check_call(["make", "-C", ORACLE_DIR, "-s", "ref", "REF=" + REF])
    if not os.path.exists(SO):
        return None
    lib = C.CDLL(SO)
    lib.ref_orb_build_id.restype = C.c_char_p
    built = lib.ref_orb_build_id().decode()
    want_ours = _sha(ours)
    if built.split(":")[0] != want_ours or (_have_reference() and built.split(":")[1] != _sha(_THEIRS)):
        raise ImportError("reference library %s is stale: built from %s, the sources on disk are %s:%s -- rebuild with "
                          "`make -C oracle ref`" % (SO, built, want_ours, _sha(_THEIRS) if _have_reference() else "?"))
    return lib


lib = _load()
vp = C.c_void_p
if lib is not None:
    lib.ref_orb_last_error.restype = C.c_char_p
    lib.ref_orb_create.restype = vp; lib.ref_orb_create.argtypes = [C.POINTER(O.Params)]
    lib.ref_orb_destroy.argtypes = [vp]; lib.ref_orb_destroy.restype = None
    lib.ref_orb_tables.argtypes = [vp] * 7; lib.ref_orb_tables.restype = None
    lib.ref_orb_extract.restype = C.c_int
    lib.ref_orb_extract.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]
    for _f in (lib.ref_orb_pyramid_level, lib.ref_orb_quality_level):
        _f.restype = C.c_int
        _f.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ref_orb_level_count.restype = C.c_int; lib.ref_orb_level_count.argtypes = [vp, C.c_int]


def available():
    return lib is not None


class ShimAssertion(RuntimeError):
    """the stand-in OpenCV refused something the reference's code asked of it (an out-of-range view or at<>, ...)"""


class Extractor:
    """ORB_SLAM2::ORBextractor itself; same surface as oracle_lib.Extractor."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, introspection=False):
        self.params = O.Params(nfeatures, scale_factor, nlevels, ini_th, min_th, int(bool(introspection)))
        self.h = lib.ref_orb_create(C.byref(self.params))
        if not self.h:
            raise ValueError("bad extractor params")
        self.nlevels = nlevels
        self.nfeatures = nfeatures

    def __del__(self):
        if getattr(self, "h", None):
            lib.ref_orb_destroy(self.h)
            self.h = None

    def tables(self):
        n = self.nlevels
        sc = np.zeros(n, np.float32); inv = np.zeros(n, np.float32); s2 = np.zeros(n, np.float32)
        is2 = np.zeros(n, np.float32); nf = np.zeros(n, np.int32); um = np.zeros(16, np.int32)
        lib.ref_orb_tables(self.h, O.ptr(sc), O.ptr(inv), O.ptr(s2), O.ptr(is2), O.ptr(nf), O.ptr(um))
        return dict(scale=sc, inv_scale=inv, sigma2=s2, inv_sigma2=is2, features_per_level=nf, umax=um)

    def __call__(self, img, cost=None, cap=None):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        cap = cap or max(2 * self.nfeatures, 64)
        kps = np.zeros(cap, O.KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.uint8)
            assert cost.shape == img.shape
        rc = lib.ref_orb_extract(self.h, O.ptr(img), w, h, w, O.ptr(cost), w, O.ptr(kps), O.ptr(desc), cap, C.byref(n))
        if rc == -4:
            raise ShimAssertion(lib.ref_orb_last_error().decode())
        if rc != 0:
            raise RuntimeError("ref_orb_extract rc=%d" % rc)
        return kps[:n.value].copy(), desc[:n.value].copy()

    def _level(self, fn, level, pad):
        d = vp(); w = C.c_int(); h = C.c_int()
        if fn(self.h, level, pad, C.byref(d), C.byref(w), C.byref(h)) != 0:
            return None
        buf = (C.c_uint8 * (w.value * h.value)).from_address(d.value)
        return np.frombuffer(buf, np.uint8).reshape(h.value, w.value).copy()

    def pyramid(self, level, pad=0):
        return self._level(lib.ref_orb_pyramid_level, level, pad)

    def quality_pyramid(self, level, pad=0):
        return self._level(lib.ref_orb_quality_level, level, pad)

    def level_counts(self):
        return [lib.ref_orb_level_count(self.h, l) for l in range(self.nlevels)]
