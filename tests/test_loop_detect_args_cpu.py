"""The argument check of LoopSearch.loop_candidates / loop_consistency (iv_slam_amd/loop.py; no GPU, no library), in the manner of
tests/test_loop_args_cpu.py: the stub library, table entries and corruptions of tests/test_track_args_cpu.py.  Every tensor goes through
track._ptr before its address reaches ivf_tracker_loop_candidates / ivf_tracker_loop_consistency, the counts the library receives are
the tensors' own, and include/ivfront.h declares both entry points with the argument counts of _lib._SIGS."""
import inspect
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from iv_slam_amd import _lib, track
from iv_slam_amd.loop import LoopDetect, LoopSearch
from test_track_args_cpu import N, NF, T, corruptions, f32, f64, i32, tracker, u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC, GC, MEM, NCONN = 3, 4, 5, 6                                # max_candidates, group_cap, member_cap, n_conn: all different, none equal to N
TABLE = {
    "loop_candidates": lambda: dict(kf_bow_word=T(i32(N, NF)), kf_bow_value=T(f64(N, NF)), kf_bow_n=T(i32(N), defines=True),
                                    kf_neigh=T(i32(N, track.KF_NEIGH), exact=True), conn_start=T(i32(N + 1), exact=True), conn=T(i32(NCONN), defines=True),
                                    query_kf=T(i32(N), defines=True), query_visible=T(i32(N)), min_score=T(f32(N)), cand=T(i32(N, MC), defines=True),
                                    ncand=T(i32(N)), kf_live=T(u8(N)), query_select=T(i32(N)), scores=T(f32(N, N)), common=T(i32(N, N))),
    "loop_consistency": lambda: dict(kf_record=T(i32(N), defines=True), conn_start=T(i32(N + 1), exact=True), conn=T(i32(NCONN), defines=True),
                                     query_kf=T(i32(N), defines=True), cand=T(i32(N, MC), defines=True), ncand=T(i32(N)), group_member=T(i32(GC, MEM), defines=True),
                                     group_size=T(i32(GC)), group_count=T(i32(GC)), n_groups=T(i32(2), unsized=True), enough=T(i32(N, MC)), nenough=T(i32(N)),
                                     pairs=T(i32(N, MC, 2), exact=True), select=T(i32(N, MC)), status=T(i32(N)), th=3),
}
METHODS = sorted(TABLE)


def searcher():
    return LoopSearch(tracker())


def optional(method):
    return {n for n, p in inspect.signature(getattr(LoopSearch, method)).parameters.items() if p.default is None and n != "stream_ptr"}


def call(s, method, args, omit=()):
    return getattr(s, method)(**{n: (a.x if isinstance(a, T) else a) for n, a in args.items() if n not in omit})


def test_the_table_is_the_methods_of_loop_detect_and_loop_search_has_them():
    assert METHODS == sorted(n for n, f in vars(LoopDetect).items() if inspect.isfunction(f) and not n.startswith("_"))
    for m in METHODS:
        assert getattr(LoopSearch, m) is getattr(LoopDetect, m)
        names = [n for n in inspect.signature(getattr(LoopSearch, m)).parameters if n not in ("self", "stream_ptr")]
        args = TABLE[m]()
        assert list(args) == names, m
        assert all(isinstance(args[n], T) for n in optional(m)), m


@pytest.mark.parametrize("method", METHODS)
def test_valid_calls_reach_the_library_once_with_every_pointer_and_the_tensors_own_counts(method):
    s, args = searcher(), TABLE[method]()
    call(s, method, args)
    (name, full), = s._lib.calls
    assert name == "ivf_tracker_" + method and len(full) == len(_lib._SIGS[name][1])
    where = {}
    for n, a in args.items():
        if isinstance(a, T):
            assert full.count(a.x.data_ptr()) == 1, n
            where[n] = full.index(a.x.data_ptr())
    scalars = [v for k, v in enumerate(full) if k not in where.values() and k != 0]
    if method == "loop_candidates":
        assert scalars == [N, NCONN, N, MC, None]              # n_keyframes, n_conn, n_queries, max_candidates, the stream
    else:
        assert scalars == [N, NCONN, N, MC, 3, GC, MEM, None]  # n_keyframes, n_conn, n_queries, max_candidates, th, group_cap, member_cap, the stream
    s._lib.calls.clear()
    call(s, method, args, omit=optional(method))
    (name, bare), = s._lib.calls
    assert len(bare) == len(full)
    for n, k in where.items():
        assert bare[k] == (None if n in optional(method) else args[n].x.data_ptr()), n


@pytest.mark.parametrize("method", METHODS)
def test_a_corrupted_tensor_never_reaches_the_library(method):
    """wrong element size, wrong kind, not contiguous, wrong device, None, one element too few and, where the count is a dimension, one too many"""
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


def test_wrong_counts_are_refused():
    """tables whose rows are another count than the call's: a cand of another n_queries, a pairs that is not exactly
    [n_queries, max_candidates, 2], a group_member that is not a table, a database one keyframe short of the connected offsets"""
    s = searcher()
    for method, bad in (("loop_candidates", dict(cand=i32(N + 1, MC))), ("loop_candidates", dict(cand=i32(N * MC))), ("loop_candidates", dict(cand=i32(N, 0))),
                        ("loop_candidates", dict(kf_bow_n=i32(N - 1))), ("loop_candidates", dict(query_kf=i32(N + 1))),
                        ("loop_consistency", dict(pairs=i32(N * MC, 2))), ("loop_consistency", dict(pairs=i32(N, MC * 2))), ("loop_consistency", dict(pairs=i32(N, MC, 3))),
                        ("loop_consistency", dict(pairs=i32(N + 1, MC, 2))), ("loop_consistency", dict(group_member=i32(GC * MEM))),
                        ("loop_consistency", dict(group_member=i32(0, MEM))), ("loop_consistency", dict(cand=i32(N + 1, MC))), ("loop_consistency", dict(kf_record=i32(N + 1))),
                        ("loop_consistency", dict(group_size=i32(GC - 1))), ("loop_consistency", dict(n_groups=i32(0)))):
        args = {n: (a.x if isinstance(a, T) else a) for n, a in TABLE[method]().items()}
        args.update(bad)
        with pytest.raises(AssertionError):
            getattr(s, method)(**args)
        assert not s._lib.calls, (method, list(bad))


def test_the_messages_name_the_argument():
    s = searcher()
    args = {n: (a.x if isinstance(a, T) else a) for n, a in TABLE["loop_consistency"]().items()}
    with pytest.raises(AssertionError, match=r"pairs is \[n_queries, max_candidates, 2\].*given torch.int32 \(6, 2\) on cpu"):
        s.loop_consistency(**dict(args, pairs=i32(N * MC, 2)))
    with pytest.raises(AssertionError, match=r"conn_start: expected .*int32.*exactly 3 .*conn_start is \[n_keyframes \+ 1\]"):
        s.loop_consistency(**dict(args, conn_start=i32(N)))
    with pytest.raises(AssertionError, match=r"query_visible: expected .*on cpu.*given torch.int32 \(2,\) on meta"):
        s.loop_candidates(**dict({n: (a.x if isinstance(a, T) else a) for n, a in TABLE["loop_candidates"]().items()}, query_visible=torch.empty(N, dtype=torch.int32, device="meta")))


def test_the_header_declares_both_entry_points_with_the_bound_argument_counts():
    text = open(os.path.join(ROOT, "include", "ivfront.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for m in METHODS:
        name = "ivf_tracker_" + m
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert decl, name + " is not declared in include/ivfront.h"
        assert len(decl.group(1).split(",")) == len(_lib._SIGS[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS
