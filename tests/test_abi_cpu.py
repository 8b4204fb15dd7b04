"""CPU-side checks of the C-ABI: libivfront.so loads, exports every symbol include/ivfront.h declares,
and fails loudly (no CPU fallback) when no GPU is present.  No compute calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ivf_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from iv_slam_amd import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), "libivfront.so does not export %s" % s
    assert sorted(_lib.EXPORTED_SYMBOLS) == syms, "python binding table and header disagree"
    assert lib.ivf_version() >= 100


def test_build_provenance_is_checked_on_load(monkeypatch):
    """ivf_build_id() = sha256[:16] of the sources the library was linked from; load() refuses a library whose id differs from the
    sources beside it, so a stale .so can produce neither a test result nor a bench line.  Same for the oracle checker."""
    from iv_slam_amd import _lib
    lib = _lib.load()
    assert lib.ivf_build_id().decode() == _lib.source_build_id() and len(_lib.source_build_id()) == 16
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "source_build_id", lambda flags="": "0123456789abcdef")
    monkeypatch.delenv("IVFRONT_LIB", raising=False)
    with pytest.raises(ImportError, match="stale"):
        _lib.load()
    # the id covers the variant flags: the product was built with none
    assert lib.ivf_build_flags().decode() == ""
    import oracle_lib as O
    assert O.BUILD_ID == O.source_build_id() and O.BUILD_ID != "unstamped"


def test_product_library_reads_only_the_documented_environment_switches():
    """r04 verdict: an environment variable must not be able to change what a drop-in ORBextractor returns.  The kernel-variant selectors
    and tuning knobs of the experiments (IVF_FCN_*, IVF_PYR_*, IVF_FAST_ABLATE, ...) exist only in the experiment build
    (make EXPERIMENT=1 -> libivfront_exp.so); the product carries exactly the switches INTEGRATION.md documents, all result-preserving."""
    import re
    from iv_slam_amd import _lib
    blob = open(_lib.LIB_PATH if not os.environ.get("IVFRONT_LIB") else os.path.join(os.path.dirname(_lib.__file__), "libivfront.so"), "rb").read()
    names = sorted(set(m.decode() for m in re.findall(rb"(?<![A-Za-z0-9_])IVF_[A-Z0-9_]{3,}(?![A-Za-z0-9_])", blob)))
    allowed = {"IVF_NO_SIDE_BLUR", "IVF_FRAME_WINDOW_CAP", "IVF_FCN_DEBUG"}
    assert set(names) <= allowed, "undocumented IVF_* strings in the product library: %r" % sorted(set(names) - allowed)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in allowed:
        assert n in doc, "%s is read by the library but not documented in INTEGRATION.md" % n
    if os.path.exists(_lib.EXPERIMENT_LIB_PATH):
        exp = open(_lib.EXPERIMENT_LIB_PATH, "rb").read()
        assert b"IVF_FCN_FUSED4" in exp and b"-DIVF_EXPERIMENT" in exp      # the selectors live there, and the build says what it is


def test_struct_layouts_match_header():
    from iv_slam_amd import _lib
    assert _lib.KP_DTYPE.itemsize == 24 and C.sizeof(_lib.ExtractorParams) == 24
    assert C.sizeof(_lib.Bounds) == 16 and C.sizeof(_lib.FrontendConfig) == 24 * 2 + 6 * 4


def test_no_cpu_fallback_without_gpu():
    from iv_slam_amd import _lib
    lib = _lib.load()
    if lib.ivf_device_count() > 0:
        pytest.skip("a GPU is present")
    import iv_slam_amd as iv
    with pytest.raises(iv.IvfError) as e:
        iv.ORBextractor(1000, 1.2, 8, 20, 7)
    assert e.value.code == _lib.IVF_E_NO_DEVICE and "no CPU path" in str(e.value)
    p = np.zeros((4, 2), np.int32); d = np.zeros((4, 32), np.uint8); out = np.zeros(4, np.int32)
    assert lib.ivf_hamming_pairs(_lib.ptr(d), 4, _lib.ptr(d), 4, _lib.ptr(p), 4, _lib.ptr(out), 0) == _lib.IVF_E_NO_DEVICE


def test_argument_validation_without_gpu():
    from iv_slam_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    bad = _lib.ExtractorParams(1000, 1.2, 99, 20, 7, 0)
    assert lib.ivf_extractor_create(C.byref(bad), 0, C.byref(h)) == _lib.IVF_E_INVALID
    assert b"nlevels" in lib.ivf_last_error()
    bad = _lib.ExtractorParams(1000, 1.2, 8, 5, 7, 0)
    assert lib.ivf_extractor_create(C.byref(bad), 0, C.byref(h)) == _lib.IVF_E_INVALID
    # host helper: DescriptorDistance
    a = np.arange(32, dtype=np.uint8); b = a[::-1].copy()
    assert lib.ivf_hamming(_lib.ptr(a), _lib.ptr(b)) == int(np.unpackbits(a ^ b).sum())


def test_update_quality_scores_host_helper():
    """a18 UpdateQualityScores is host bookkeeping (no GPU needed): product vs oracle, incl. the >0.01 write-back rule and
    the sequential effect of two keypoints sharing a map point."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    import iv_slam_amd as iv
    from iv_slam_amd import _lib
    rng = np.random.default_rng(5)
    n, nm = 400, 150
    assign = rng.integers(-1, nm, n).astype(np.int32)
    kq = rng.uniform(0, 1, n).astype(np.float32); mq = rng.uniform(0, 1, nm).astype(np.float32)
    kq[:50] = mq[np.clip(assign[:50], 0, nm - 1)] - np.float32(0.005)          # changes below the 0.01 threshold
    m = iv.ORBmatcher.__new__(iv.ORBmatcher); m._lib = _lib.load()
    gk, gm = m.UpdateQualityScores(assign, kq, mq)
    ok, om = kq.copy(), mq.copy()
    O.lib.orc_update_quality_scores(O.ptr(assign), n, O.ptr(ok), O.ptr(om))
    assert gk.tobytes() == ok.tobytes() and gm.tobytes() == om.tobytes()
    assert (gm != mq).any() and (gm <= mq).all()
    bad = assign.copy(); bad[3] = nm + 7
    with pytest.raises(iv.IvfError):
        m.UpdateQualityScores(bad, kq, mq)


def test_header_is_plain_c(tmp_path):
    """the boundary is a C ABI: include/ivfront.h must compile as C99 (no C++ types in the signatures) and link against the
    library from a C translation unit"""
    import subprocess
    src = tmp_path / "c_abi.c"
    src.write_text('#include "ivfront.h"\nint main(void) { return ivf_version() > 0 ? 0 : 1; }\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = tmp_path / "c_abi.o"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), "-c", "-o", str(obj), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = os.path.join(root, "iv_slam_amd", "libivfront.so")
    if os.path.exists(lib):
        exe = tmp_path / "c_abi"
        r = subprocess.run(["gcc", "-o", str(exe), str(obj), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_testing_hooks_are_declared_as_such():
    """an ivf_test_* entry point exists for the suite alone: the comment above its declaration says so, and the binding carries it like any
    other symbol (a hook that is exported but unbound, or bound but undeclared, fails test_library_exports_every_declared_symbol)"""
    import re
    from iv_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    hooks = [s for s in header_symbols() if s.startswith("ivf_test_")]
    assert hooks == ["ivf_test_pnp_hypotheses", "ivf_test_retain_best"] == sorted(s for s in _lib.EXPORTED_SYMBOLS if s.startswith("ivf_test_"))
    for name in hooks:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define \w+ \d+\s*)?int\s+%s\s*\(" % name, hdr, flags=re.S)
        assert m and "testing hook" in m.group(1).lower(), name
