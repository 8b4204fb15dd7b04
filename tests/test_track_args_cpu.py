"""The one argument check of iv_slam_amd/track.py (no GPU, no library): every tensor of every BatchTracker method goes through it before
its address reaches an ivf_tracker_* entry point.  A tracker made without a handle, on the CPU device, calls a stub library that records
what it receives; one valid argument set per method, at the smallest sizes, is the table every test below walks."""
import ast
import ctypes as C
import inspect

import pytest
import torch

from iv_slam_amd import _lib, track
from iv_slam_amd.track import LOCAL_POINT_BYTES as LPB, BatchTracker, MapView

NF, REC = 8, 48                     # nfeatures and record_bytes of the stub tracker
N = 2                               # records, pairs, frames and keyframes of every call: one-element tensors are always contiguous
MI = 2                              # max_iterations


class Stub:
    """a library whose every function records its arguments and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: (self.calls.append((name, args)), _lib.IVF_OK)[1]


class Vocabulary:
    _h = C.c_void_p(64)


class T:
    """a tensor argument of the table.  exact: its count is a dimension the call states, one element more is refused too; any4: float
    and integer are both taken (draws); unsized: its size is only known on the device, nothing here can be too short; defines: its own
    length IS the count, so one element fewer is another valid call (the [n, width] tables whose width is a count of the call, at width 1
    here, are neither: a narrower one has no column left, a wider one is another valid call)"""

    def __init__(self, x, exact=False, any4=False, unsized=False, defines=False):
        self.x, self.exact, self.any4, self.unsized, self.defines = x, exact, any4, unsized, defines


def i32(*shape): return torch.zeros(shape, dtype=torch.int32)
def f32(*shape): return torch.zeros(shape, dtype=torch.float32)
def f64(*shape): return torch.zeros(shape, dtype=torch.float64)
def u8(*shape): return torch.zeros(shape, dtype=torch.uint8)


def map_view():
    return MapView(points=u8(2 * LPB), obs_offsets=torch.tensor([0, 1, 2], dtype=torch.int32), obs_kf=i32(2), kf_point_offsets=torch.tensor([0, 2], dtype=torch.int32),
                   kf_points=i32(2), kf_neigh=torch.full((1, track.KF_NEIGH), -1, dtype=torch.int32), kf_child_offsets=i32(2), kf_children=i32(0),
                   kf_parent=torch.tensor([-1], dtype=torch.int32))


def records():
    return T(u8(N * REC), defines=True)


# method -> its arguments in signature order: a T for a tensor (optional where the signature's default is None), anything else as it is
TABLE = {
    "run": lambda: dict(records=records(), pairs=T(i32(N, 2), exact=True), assign=T(i32(N, NF)), nmatches=T(i32(N)), poses=T(f32(N, 2, 12), exact=True),
                        point_flags=T(u8(N, NF)), point_quality=T(f32(N, NF)), key_quality=T(f32(N, NF))),
    "search_local": lambda: dict(records=records(), frames=T(i32(N)), points=T(u8(3 * LPB), unsized=True), point_offsets=T(i32(N + 1)), max_points_per_frame=2,
                                 assign=T(i32(N, NF)), nmatches=T(i32(N)), poses=T(f32(N, 12), exact=True), occupied=T(u8(N, NF)), th=1.0, nn_ratio=0.8,
                                 cos_limit=0.5, point_quality=T(f32(3), unsized=True), key_quality=T(f32(N, NF))),
    "points_from_pairs": lambda: dict(records=records(), pairs=T(i32(N, 2), exact=True), assign=T(i32(N, NF)), xw=T(f32(N, NF, 3)), has_point=T(u8(N, NF)),
                                      poses=T(f32(N, 2, 12), exact=True)),
    "points_from_local": lambda: dict(points=T(u8(3 * LPB), unsized=True), point_offsets=T(i32(N + 1), defines=True), assign=T(i32(N, NF)), xw=T(f32(N, NF, 3)),
                                      has_point=T(u8(N, NF))),
    "search_by_bow": lambda: dict(vocabulary=Vocabulary(), records=records(), pairs=T(i32(N, 2), exact=True), assign=T(i32(N, NF)), nmatches=T(i32(N)), levelsup=4,
                                  select=T(i32(N)), point_flags=T(u8(N, NF)), nn_ratio=0.7, check_orientation=True, point_quality=T(f32(N, NF)),
                                  key_quality=T(f32(N, NF))),
    "points_from_keyframe": lambda: dict(pairs=T(i32(N, 2), exact=True), kf_xw=T(f32(N, NF, 3), exact=True), assign=T(i32(N, NF)), xw=T(f32(N, NF, 3)),
                                         has_point=T(u8(N, NF))),
    "bow_vectors": lambda: dict(vocabulary=Vocabulary(), records=records(), frames=T(i32(N), defines=True), bow_word=T(i32(N, NF)), bow_value=T(f64(N, NF)),
                                bow_n=T(i32(N))),
    "reloc_candidates": lambda: dict(vocabulary=Vocabulary(), kf_bow_word=T(i32(N, NF)), kf_bow_value=T(f64(N, NF)), kf_bow_n=T(i32(N)),
                                     kf_neigh=T(i32(N, track.KF_NEIGH), exact=True), kf_record=T(i32(N)), bow_word=T(i32(N, NF)), bow_value=T(f64(N, NF)),
                                     bow_n=T(i32(N)), frame_record=T(i32(N)), cand=T(i32(N, 1)), ncand=T(i32(N)), pairs=T(i32(N, 2)), select=T(i32(N)),
                                     kf_live=T(u8(N)), kf_reloc_score=T(f32(N)), scores=T(f32(N, N)), common=T(i32(N, N))),
    "search_reloc": lambda: dict(records=records(), pairs=T(i32(N, 2), exact=True), kf_points=T(u8(N, NF * LPB)), assign=T(i32(N, NF)), nmatches=T(i32(N)), th=10.0,
                                 orb_dist=100, select=T(i32(N)), poses=T(f32(N, 12), exact=True), found=T(u8(N, NF)), check_orientation=True,
                                 point_quality=T(f32(N, NF)), key_quality=T(f32(N, NF))),
    "filter_assign": lambda: dict(assign=T(i32(N, NF), exact=True), mask=T(u8(N, NF)), keep_when_set=True, found=T(u8(N, NF))),
    "optimize_pose": lambda: dict(records=records(), frames=T(i32(N)), xw=T(f32(N, NF, 3)), has_point=T(u8(N, NF)), poses=T(f32(N, 12), exact=True),
                                  outlier=T(u8(N, NF)), ninliers=T(i32(N)), quality=T(f32(N, NF)), n_rounds=4, chi2=T(f32(N, NF))),
    "update_local_map": lambda: dict(map_view=map_view(), frame_points=T(i32(N, NF), exact=True), local_kf=T(i32(N, 1)), n_local_kf=T(i32(N)),
                                     ref_kf=T(i32(N)), points=T(u8(N, LPB)), point_ids=T(i32(N, 1)), point_offsets=T(i32(N + 1)),
                                     n_local_points=T(i32(N)), occupied=T(u8(N, NF))),
    "create_map_points": lambda: dict(vocabulary=Vocabulary(), records=T(u8(N * REC)), kf=T(i32(N), exact=True), neigh=T(i32(N, 1)),
                                      poses=T(f32(N, 12), exact=True), has_point=T(u8(N, NF)), new_point=T(u8(N, NF * LPB)), new_neigh=T(i32(N, NF)),
                                      new_idx2=T(i32(N, NF)), new_order=T(i32(N, NF)), new_quality=T(f32(N, NF)), n_new=T(i32(N)), levelsup=4,
                                      key_quality=T(f32(N, NF)), F12=T(f32(N, 1, 9), exact=True), kf_order=T(i32(N), exact=True), matches=T(i32(N, 1, NF)),
                                      stage=T(u8(N, 1, NF))),
    "merge_local": lambda: dict(point_ids=T(i32(N, 1)), point_offsets=T(i32(N + 1)), assign=T(i32(N, NF)), frame_points=T(i32(N, NF), exact=True)),
    "points_from_map": lambda: dict(map_view=map_view(), frame_points=T(i32(N, NF), exact=True), xw=T(f32(N, NF, 3)), has_point=T(u8(N, NF)), quality=T(f32(N, NF)),
                                    point_quality=T(f32(2))),
    "close_local_map": lambda: dict(map_view=map_view(), outlier=T(u8(N, NF)), frame_points=T(i32(N, NF), exact=True), ninliers=T(i32(N)), only_tracking=False,
                                    stereo=True),
    "solve_pnp": lambda: dict(records=records(), frames=T(i32(N)), xw=T(f32(N, NF, 3)), has_point=T(u8(N, NF)), draws=T(i32(N, MI, 4), any4=True),
                              poses=T(f32(N, 12), exact=True), inlier=T(u8(N, NF)), ninliers=T(i32(N)), max_iterations=MI, probability=0.99, min_inliers=10,
                              epsilon=0.5, th2=5.991, iterations=T(i32(N)), hyp_poses=T(f32(N, MI, 12)), hyp_ninliers=T(i32(N, MI))),
    "pnp_hypotheses": lambda: dict(records=records(), frames=T(i32(N), defines=True), xw=T(f32(N, NF, 3)), has_point=T(u8(N, NF)), draws=T(i32(N, MI, 4), any4=True),
                                   taps=T(f64(N, MI, track.PNP_TAP_DOUBLES)), hyp_poses=T(f32(N, MI, 12)), hyp_ninliers=T(i32(N, MI)), max_iterations=MI,
                                   probability=0.99, min_inliers=10, epsilon=0.5, th2=5.991),
    "solve_sim3": lambda: dict(records=T(u8(N * REC)), pairs=T(i32(N, 2), exact=True), poses=T(f32(N, 12), exact=True), kf_xw=T(f32(N, NF, 3), exact=True),
                               point_flags=T(u8(N, NF)), match12=T(i32(N, NF)), draws=T(i32(N, MI, 3), any4=True), sim3=T(f32(N, 16), exact=True),
                               inlier=T(u8(N, NF)), ninliers=T(i32(N)), max_iterations=MI, probability=0.99, min_inliers=20, fix_scale=True, select=T(i32(N)),
                               state=T(i32(N, 2), exact=True), iterations=T(i32(N)), hyp_sim3=T(f32(N, MI, 16)), hyp_ninliers=T(i32(N, MI))),
}
ENTRY = {"pnp_hypotheses": "ivf_test_pnp_hypotheses"}                      # the testing hook; every other method m calls ivf_tracker_<m>
METHODS = sorted(n for n, f in vars(BatchTracker).items() if inspect.isfunction(f) and not n.startswith("_"))


def tracker():
    t = object.__new__(BatchTracker)
    t.device, t.nfeatures, t.record_bytes, t._lib, t._h = torch.device("cpu"), NF, REC, Stub(), C.c_void_p(16)
    return t


def optional(method):
    return {n for n, p in inspect.signature(getattr(BatchTracker, method)).parameters.items() if p.default is None and n != "stream_ptr"}


def call(t, method, args, omit=()):
    return getattr(t, method)(**{n: (a.x if isinstance(a, T) else a) for n, a in args.items() if n not in omit})


def test_the_table_is_the_methods():
    assert sorted(TABLE) == METHODS, "every BatchTracker method has its argument set here"
    for m in METHODS:
        names = [n for n in inspect.signature(getattr(BatchTracker, m)).parameters if n not in ("self", "stream_ptr")]
        args = TABLE[m]()
        assert list(args) == names, m
        assert all(isinstance(args[n], T) for n in optional(m)), m


@pytest.mark.parametrize("method", METHODS)
def test_valid_calls_reach_the_library_once_with_every_pointer(method):
    t, args = tracker(), TABLE[method]()
    call(t, method, args)
    (name, full), = t._lib.calls
    assert name == ENTRY.get(method, "ivf_tracker_" + method) and len(full) == len(_lib._SIGS[name][1])
    where = {}
    for n, a in args.items():
        if isinstance(a, T):
            assert full.count(a.x.data_ptr()) == 1, n
            where[n] = full.index(a.x.data_ptr())
    t._lib.calls.clear()
    call(t, method, args, omit=optional(method))
    (name, bare), = t._lib.calls
    assert len(bare) == len(full)
    for n, k in where.items():
        assert bare[k] == (None if n in optional(method) else args[n].x.data_ptr()), n
    assert [repr(v) for k, v in enumerate(bare) if k not in where.values()] == [repr(v) for k, v in enumerate(full) if k not in where.values()], "the scalars"


def corruptions(a):
    """(what, tensor or None) for every way the tensor argument a can be wrong"""
    x = a.x
    n, last = x.numel(), x.shape[:-1]
    resized = {torch.int32: torch.int64, torch.float32: torch.float64, torch.uint8: torch.int32, torch.float64: torch.float32}[x.dtype]
    out = [("element size", x.to(resized)), ("not contiguous", x.new_zeros(last + (2 * x.shape[-1],))[..., ::2]), ("device", torch.empty_like(x, device="meta")),
           ("None", None)]
    if not a.any4 and x.dtype != torch.uint8:
        out.append(("kind", x.to({torch.int32: torch.float32, torch.float32: torch.int32, torch.float64: torch.int64}[x.dtype])))
    if not (a.unsized or a.defines):
        out.append(("one too few", x.new_zeros(last + (x.shape[-1] - 1,)) if x.dim() > 1 else x.new_zeros(n - 1)))
    if a.exact:
        out.append(("one too many", x.new_zeros(last + (x.shape[-1] + 1,)) if x.dim() > 1 else x.new_zeros(n + 1)))
    return out


@pytest.mark.parametrize("method", METHODS)
def test_a_corrupted_tensor_never_reaches_the_library(method):
    t = tracker()
    tried = 0
    for n, a in TABLE[method]().items():
        if not isinstance(a, T):
            continue
        for what, bad in corruptions(a):
            if bad is None and n in optional(method):
                continue
            assert bad is None or what != "not contiguous" or not bad.is_contiguous()
            args = TABLE[method]()
            args[n] = bad
            try:
                call(t, method, args)
            except AssertionError:
                pass
            else:
                pytest.fail("%s(%s: %s) was not refused" % (method, n, what))
            assert not t._lib.calls, "%s(%s: %s) reached the library" % (method, n, what)
            tried += 1
    assert tried >= 4 * sum(isinstance(a, T) for a in TABLE[method]().values())


def test_a_map_view_elsewhere_is_refused():
    t = tracker()
    for m in ("update_local_map", "points_from_map", "close_local_map"):
        view = map_view()
        view.device = torch.device("meta")
        for bad in (view, None, view.c):
            with pytest.raises(AssertionError):
                call(t, m, dict(TABLE[m](), map_view=bad))
    assert not t._lib.calls


def test_map_view_refuses_bad_tables():
    i = lambda *v: torch.tensor(v, dtype=torch.int32)
    pts = u8(2 * LPB)
    ok = dict(points=pts, obs_offsets=i(0, 1, 2), obs_kf=i(0, 0), kf_point_offsets=i(0, 2), kf_points=i(0, 1),
              kf_neigh=torch.full((1, track.KF_NEIGH), -1, dtype=torch.int32), kf_child_offsets=i(0, 0), kf_children=i(), kf_parent=i(-1))
    v = MapView(**ok)
    assert v.device == torch.device("cpu") and (v.c.n_points, v.c.n_keyframes, v.c.n_obs, v.c.n_kf_points, v.c.n_children) == (2, 1, 2, 2, 0)
    assert v.c.points == pts.data_ptr() and v.c.kf_children is None and v.c.kf_live is None and v.c.kf_order is None
    for bad in (dict(points=pts[:LPB]), dict(kf_neigh=torch.full((1, track.KF_NEIGH - 1), -1, dtype=torch.int32)), dict(kf_order=i(0, 0)),
                dict(obs_kf=torch.zeros(2, dtype=torch.int64)), dict(kf_parent=torch.empty(1, dtype=torch.int32, device="meta")),
                dict(points=torch.empty_like(pts, device="meta")), dict(kf_live=torch.ones(1, dtype=torch.float32)), dict(obs_offsets=i())):
        with pytest.raises(AssertionError):
            MapView(**dict(ok, **bad))


def test_the_messages_name_the_argument_and_both_sides():
    t, args = tracker(), TABLE["run"]()
    args["poses"] = f32(N, 12)
    with pytest.raises(AssertionError, match=r"poses: expected .*float32.*exactly 48 .*per PAIR: \[n_pairs, 2, 12\].*given torch.float32 \(2, 12\) on cpu"):
        call(t, "run", args)
    with pytest.raises(AssertionError, match=r"kf_neigh is \[n_keyframes, 10\]"):
        call(t, "reloc_candidates", dict(TABLE["reloc_candidates"](), kf_neigh=i32(N, 9)))


def test_the_checks_survive_python_O_and_one_function_takes_addresses():
    tree = ast.parse(open(track.__file__).read())
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)], "an assert statement is gone under python -O"
    takers = {f.name for f in ast.walk(tree) if isinstance(f, ast.FunctionDef) for n in ast.walk(f) if isinstance(n, ast.Attribute) and n.attr == "data_ptr"}
    assert takers == {"_ptr"}
