"""The argument check of iv_slam_amd/loop.py (no GPU, no library), in the manner of tests/test_track_args_cpu.py, whose stub library, table
entries and corruptions it borrows: every tensor of both LoopSearch methods goes through track._ptr before its address reaches
ivf_tracker_search_by_bow_keyframes / ivf_tracker_search_by_sim3; the module takes no address of its own and has no assert statement; and
include/ivfront.h declares both entry points with the argument counts of _lib._SIGS."""
import ast
import inspect
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import iv_slam_amd
from iv_slam_amd import _lib, loop
from iv_slam_amd.loop import LoopSearch
from test_track_args_cpu import LPB, N, NF, REC, T, Vocabulary, call as _call, corruptions, f32, i32, records, tracker, u8  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {
    "search_by_bow_keyframes": lambda: dict(vocabulary=Vocabulary(), records=records(), pairs=T(i32(N, 2), exact=True), match12=T(i32(N, NF)), nmatches=T(i32(N)),
                                            levelsup=4, select=T(i32(N)), point_flags=T(u8(N, NF)), nn_ratio=0.75, check_orientation=True),
    "search_by_sim3": lambda: dict(records=records(), pairs=T(i32(N, 2), exact=True), poses=T(f32(N, 12), exact=True), kf_points=T(u8(N, NF * LPB)),
                                   sim3=T(f32(N, 16), exact=True), match12=T(i32(N, NF)), matches=T(i32(N, NF)), nfound=T(i32(N)), th=7.5, select=T(i32(N)),
                                   inlier=T(u8(N, NF)), match1=T(i32(N, NF)), match2=T(i32(N, NF))),
}
METHODS = sorted(n for n, f in vars(LoopSearch).items() if inspect.isfunction(f) and not n.startswith("_"))


def searcher():
    return LoopSearch(tracker())


def optional(method):
    return {n for n, p in inspect.signature(getattr(LoopSearch, method)).parameters.items() if p.default is None and n != "stream_ptr"}


def call(s, method, args, omit=()):
    return getattr(s, method)(**{n: (a.x if isinstance(a, T) else a) for n, a in args.items() if n not in omit})


def test_the_table_is_the_methods_and_the_class_is_exported():
    assert sorted(TABLE) == METHODS == ["search_by_bow_keyframes", "search_by_sim3"] and iv_slam_amd.LoopSearch is LoopSearch
    for m in METHODS:
        names = [n for n in inspect.signature(getattr(LoopSearch, m)).parameters if n not in ("self", "stream_ptr")]
        args = TABLE[m]()
        assert list(args) == names, m
        assert all(isinstance(args[n], T) for n in optional(m)), m
    s = searcher()
    assert (s.nfeatures, s.record_bytes, s.device) == (NF, REC, s._tracker.device) and s._h is s._tracker._h


@pytest.mark.parametrize("method", METHODS)
def test_valid_calls_reach_the_library_once_with_every_pointer(method):
    s, args = searcher(), TABLE[method]()
    call(s, method, args)
    (name, full), = s._lib.calls
    assert name == "ivf_tracker_" + method and len(full) == len(_lib._SIGS[name][1])
    where = {}
    for n, a in args.items():
        if isinstance(a, T):
            assert full.count(a.x.data_ptr()) == 1, n
            where[n] = full.index(a.x.data_ptr())
    s._lib.calls.clear()
    call(s, method, args, omit=optional(method))
    (name, bare), = s._lib.calls
    assert len(bare) == len(full)
    for n, k in where.items():
        assert bare[k] == (None if n in optional(method) else args[n].x.data_ptr()), n
    assert [repr(v) for k, v in enumerate(bare) if k not in where.values()] == [repr(v) for k, v in enumerate(full) if k not in where.values()], "the scalars"


@pytest.mark.parametrize("method", METHODS)
def test_a_corrupted_tensor_never_reaches_the_library(method):
    s = searcher()
    tried = 0
    for n, a in TABLE[method]().items():
        if not isinstance(a, T):
            continue
        for what, bad in corruptions(a):
            if bad is None and n in optional(method):
                continue
            args = TABLE[method]()
            args[n] = bad
            try:
                call(s, method, args)
            except AssertionError:
                pass
            else:
                pytest.fail("%s(%s: %s) was not refused" % (method, n, what))
            assert not s._lib.calls, "%s(%s: %s) reached the library" % (method, n, what)
            tried += 1
    assert tried >= 4 * sum(isinstance(a, T) for a in TABLE[method]().values())


def test_the_module_takes_no_address_and_has_no_assert():
    src = open(loop.__file__).read()
    tree = ast.parse(src)
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)], "an assert statement is gone under python -O"
    assert "data_ptr" not in src, "every address is track._ptr's to take"


def test_the_header_declares_both_entry_points_with_the_bound_argument_counts():
    text = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for m in METHODS:
        name = "ivf_tracker_" + m
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert decl, name + " is not declared in include/ivfront.h"
        assert len(decl.group(1).split(",")) == len(_lib._SIGS[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS
