"""Host layer of the batched front end (ivf_api.hip): image sources are arguments of each run, the batch / image lookups return the
documented codes, the cost plane is bounded and allocated lazily by whichever call needs it first.
All at 637 x 241, 400 features, 2 pairs: odd width (the row's last 16-byte piece), four images (the blur runs on the lent side stream)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from iv_slam_amd import synth
from iv_slam_amd._lib import IVF_E_INVALID, IVF_E_STATE, IVF_OK, KP_DTYPE, Bounds, ptr

pytestmark = pytest.mark.gpu

BF = 386.1448
B = BF / 718.856
W, H, N, PAIRS = 637, 241, 400, 2


@pytest.fixture(scope="module")
def iv():
    import iv_slam_amd
    lib = iv_slam_amd.load()
    assert lib.ivf_device_count() >= 1, "no HIP device: libivfront has no CPU fallback"
    return iv_slam_amd


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def padded(t, top, left):
    """a view with the shape of t inside a larger tensor: own image / row strides, odd byte offset"""
    import torch
    shape = list(t.shape); shape[1] += top + 3; shape[2] += left + 8
    big = torch.zeros(shape, dtype=torch.uint8, device=t.device)
    v = big[:, top:top + t.shape[1], left:left + t.shape[2]]
    v.copy_(t)
    assert not v.is_contiguous()
    return v


def fetch_all(fe):
    return [[fe.fetch(p, side) for side in (0, 1)] for p in range(PAIRS)]


def assert_same_results(got, want, tag):
    for p in range(PAIRS):
        for side in (0, 1):
            a, b = got[p][side], want[p][side]
            assert sorted(a) == sorted(b)
            for key in a:          # kps, desc, quality and, on the left, uright and depth
                assert a[key].tobytes() == b[key].tobytes(), "%s: pair %d side %d: %s differs" % (tag, p, side, key)
    assert sum(len(got[p][0]["kps"]) for p in range(PAIRS)) > 100, tag


def test_image_sources_belong_to_the_call(iv):
    """Seven runs on one handle, colour (padded views, strides per side) and plain grey by turns, so that each of the three batch contexts serves
    both kinds: every plain run equals, byte for byte, the same plain run on a fresh front end -- nothing of an earlier run's sources is left on a context."""
    rng = np.random.default_rng(9)
    mk = dict(nfeatures=N, enableIntrospection=True, bf=BF, b=B)
    fe = iv.StereoFrontend(W, H, PAIRS, **mk)
    kinds = []
    for it in range(7):
        stream = synth.make_stream(PAIRS, W, H, seed=300 + it)
        cost = to_dev(np.stack([synth.make_cost_map(W, H, seed=300 + it, idx=i) for i in range(PAIRS)]))
        if it % 2 == 0:
            col = np.stack([np.clip(stream[:, 0].astype(int) + rng.integers(-40, 41, stream[:, 0].shape), 0, 255) for _ in range(3)], axis=-1).astype(np.uint8)
            fe.run_color(padded(to_dev(col), 1, 5), padded(to_dev(stream[:, 1]), 4, 3), padded(cost, 1, 0), rgb=bool(it & 2))
            fe.sync()
        else:
            L, R = to_dev(stream[:, 0]), to_dev(stream[:, 1])
            fe.run(L, R, cost); fe.sync()
            fresh = iv.StereoFrontend(W, H, PAIRS, **mk)
            fresh.run(L, R, cost); fresh.sync()
            assert_same_results(fetch_all(fe), fetch_all(fresh), "plain run %d" % it)
        kinds.append((it % 3, it % 2))
    assert {k for k in kinds} == {(c, kind) for c in range(3) for kind in (0, 1)}


def test_batch_lookup_return_codes(iv):
    """The codes of the calls that look up a held batch or one of its images, on a fresh handle and after one run (include/ivfront.h)."""
    import torch
    lib = iv.load()
    fe = iv.StereoFrontend(W, H, PAIRS, nfeatures=N, bf=BF, b=B)
    h = fe._h
    kps = np.zeros(N, KP_DTYPE); n = C.c_int(-1); rec = C.c_size_t(0); un = C.c_void_p(); frame = C.c_void_p()
    bounds = Bounds(0.0, 0.0, float(W), float(H))

    def fetch_of(age, pair):
        return lib.ivf_frontend_fetch_of(h, age, pair, 0, ptr(kps), None, N, C.byref(n), None, None, None)

    def fetch_un(age, pair):
        return lib.ivf_frontend_fetch_undistorted(h, age, pair, ptr(kps), N, C.byref(n))

    def frame_of(age, pair):
        rc = lib.ivf_frame_create_from_frontend(h, age, pair, 0, C.byref(bounds), C.byref(frame))
        assert (rc == IVF_OK) == bool(frame.value)
        if frame.value:
            lib.ivf_frame_destroy(frame)
        return rc

    def pack(age, block):
        return lib.ivf_frontend_pack_gather_block_of(h, age, None if block is None else block.data_ptr(), 0 if block is None else block.numel(), C.byref(rec), None)

    def no_batch(ages):
        for age in ages:
            assert fetch_of(age, 0) == IVF_E_STATE, age
            assert "no batch of age %d is held" % age in lib.ivf_last_error().decode()
            assert lib.ivf_frontend_undistorted(h, age, C.byref(un)) == IVF_E_STATE, age
            assert fetch_un(age, 0) == IVF_E_STATE, age
            assert frame_of(age, 0) == IVF_E_STATE, age
            assert lib.ivf_frontend_batch_stream(h, age) is None, age

    # a fresh handle holds no batch
    no_batch((-1, 0, 1, 2, 3))
    assert lib.ivf_frontend_fetch(h, 0, 0, ptr(kps), None, N, C.byref(n), None, None, None) == IVF_E_INVALID
    for age in (0, 2, 5, -1):                      # the record size is answered whatever the age
        rec.value = 0
        assert pack(age, None) == IVF_OK and rec.value == fe.gather_record_bytes() > 0
    block = torch.zeros(PAIRS * rec.value, dtype=torch.uint8, device="cuda:0")
    assert pack(-1, block) == IVF_E_INVALID and pack(3, block) == IVF_E_INVALID
    assert pack(0, block) == IVF_E_STATE and pack(2, block) == IVF_E_STATE

    stream = synth.make_stream(PAIRS, W, H, seed=311)
    fe.run(to_dev(stream[:, 0]), to_dev(stream[:, 1])); fe.sync()
    # one batch, of age 0, without a camera
    no_batch((-1, 1, 2, 3))
    assert fetch_of(0, 0) == IVF_OK and n.value > 50
    plain = kps[:n.value].copy()
    assert fetch_of(0, -1) == IVF_E_INVALID and fetch_of(0, PAIRS) == IVF_E_INVALID
    assert frame_of(0, -1) == IVF_E_INVALID and frame_of(0, PAIRS) == IVF_E_INVALID
    assert frame_of(0, PAIRS - 1) == IVF_OK
    assert lib.ivf_frontend_fetch(h, 0, 0, ptr(kps), None, N, C.byref(n), None, None, None) == IVF_OK
    assert lib.ivf_frontend_undistorted(h, 0, C.byref(un)) == IVF_E_STATE
    kps[:] = 0; n.value = -1
    assert fetch_un(0, 0) == IVF_OK and kps[:n.value].tobytes() == plain.tobytes()      # no camera: mvKeysUn == mvKeys, the plain fetch
    assert fetch_un(0, PAIRS) == IVF_E_INVALID
    assert lib.ivf_frontend_batch_stream(h, 0) is not None
    assert pack(-1, block) == IVF_E_INVALID and pack(3, block) == IVF_E_INVALID
    assert pack(1, block) == IVF_E_STATE and pack(0, block) == IVF_OK
    assert pack(7, None) == IVF_OK
    torch.cuda.synchronize()
    assert int(block[:4].cpu().numpy().view(np.int32)[0]) == len(plain)


def test_cost_plane_is_bounded_by_max_pairs(iv):
    fe = iv.StereoFrontend(W, H, PAIRS, nfeatures=N, enableIntrospection=True, bf=BF, b=B)
    for n in (0, PAIRS + 1):
        with pytest.raises(ValueError):
            fe.cost_plane(n)
    assert tuple(fe.cost_plane(PAIRS).shape) == (PAIRS, H, W)


@pytest.fixture(scope="module")
def plain_scene():
    """two pairs, their cost maps, and what Frame.cc:130-143 gives for extractors built with enableIntrospection = 0: the plain keypoints, and
    mvKeyQualScore of the left ones read from the cost image"""
    stream = synth.make_stream(PAIRS, W, H, seed=43)
    cost = np.stack([synth.make_cost_map(W, H, seed=43, idx=i) for i in range(PAIRS)])
    want = []
    for p in range(PAIRS):
        okL, odL = O.Extractor(N, 1.2, 8, 20, 7)(stream[p, 0])
        c = cost[p][O.c_round(okL["y"]), O.c_round(okL["x"])].astype(np.float32)
        q = (np.float64(1.0) / (np.float64(1.0) + (c / np.float32(256)).astype(np.float64))).astype(np.float32)
        want.append((okL, odL, (np.float32(2) * q - np.float32(1)).astype(np.float32)))
    return stream, cost, want


@pytest.mark.parametrize("first", ["cost_plane", "run"])
def test_lazy_cost_plane_whichever_call_comes_first(iv, plain_scene, first):
    """A front end whose extractors ignore the map allocates its cost planes on first use: by ivf_frontend_cost_plane (the producer writes the maps
    there, the run skips their ingest) or by a run that brings a cost batch.  Either way the results are those of
    test_gpu_parity.py::test_quality_scores_without_extractor_introspection."""
    import torch
    stream, cost, want = plain_scene
    fe = iv.StereoFrontend(W, H, PAIRS, nfeatures=N, enableIntrospection=False, bf=BF, b=B)
    L, R, Cm = to_dev(stream[:, 0]), to_dev(stream[:, 1]), to_dev(cost)
    sptr = torch.cuda.current_stream().cuda_stream
    if first == "cost_plane":
        plane = fe.cost_plane(PAIRS, sptr)
        plane.copy_(Cm)
        fe.run_color(L, R, plane, sptr)
    else:
        fe.run(L, R, Cm, sptr)
    fe.sync()
    for p in range(PAIRS):
        okL, odL, q = want[p]
        rl = fe.fetch(p, 0)
        assert rl["kps"].tobytes() == okL.tobytes() and np.array_equal(rl["desc"], odL), "pair %d: plain keypoints" % p
        assert np.array_equal(rl["quality"], q), "pair %d" % p
        assert (fe.fetch(p, 1)["quality"] == 1.0).all()
    assert len(want[0][0]) > 100
