"""Device Frame::UndistortKeyPoints (ORB/src/Frame.cc:696-726; k_undistort_keys) against the test-side
restatement tests/undistort_ref.py: every comparison is on the float32 BIT PATTERNS, no tolerance.  Per-call and batched entry
points, the front end with a camera set (mvKeysUn beside an untouched mvKeys), gather records + the tracker step with the
undistorted bounds against oracle/projection_oracle.py, and the resident frame's grid with EuRoC's negative origin."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import undistort_ref as U
from iv_slam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = os.path.join(ROOT, "tests", "golden", "settings")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
F = np.float32

# camera -> (image size, bf of the synthetic rig, seed of the synthetic pair); the sizes are those the reference's examples use
RIGS = {"EuRoC": ((752, 480), 47.90639, 21), "TUM1": ((640, 480), 40.0, 22)}


@pytest.fixture(scope="module")
def iv():
    import iv_slam_amd
    assert iv_slam_amd.load().ivf_device_count() >= 1, "no HIP device: libivfront has no CPU fallback"
    return iv_slam_amd


def load_camera(name):
    from iv_slam_amd import kitti
    return kitti.Settings.load(os.path.join(SETTINGS, name + ".yaml")).camera()


def seeded_camera8():
    from iv_slam_amd.camera import Camera
    rng = np.random.default_rng(8)
    dist = np.concatenate([rng.uniform(-1, 1, 4) * [0.3, 0.3, 0.005, 0.005], rng.uniform(-0.05, 0.05, 4)]).astype(np.float32)
    return Camera(611.25, 608.5, 330.75, 236.125, dist)


def as_ref(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy, cam.dist)


def random_keypoints(n, w, h, seed):
    from iv_slam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KP_DTYPE)
    k["x"] = rng.uniform(0, w, n).astype(F); k["y"] = rng.uniform(0, h, n).astype(F)
    k["x"][: n // 2] = np.floor(k["x"][: n // 2])                         # level-0 keypoints sit on integers
    k["size"] = rng.uniform(31, 111, n); k["angle"] = rng.uniform(0, 360, n); k["response"] = rng.uniform(7, 200, n)
    k["octave"] = rng.integers(0, 8, n)
    return k


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.frombuffer(a.tobytes(), np.uint32), np.frombuffer(b.tobytes(), np.uint32))


@pytest.mark.parametrize("name", ["TUM1", "TUM2", "EuRoC", "seeded8"])
def test_undistort_keypoints_equals_the_restatement(iv, name):
    cam = seeded_camera8() if name == "seeded8" else load_camera(name)
    w, h = (752, 480) if name == "EuRoC" else (640, 480)
    for n in (0, 1, 1000, 4096):
        kps = random_keypoints(n, w, h, seed=100 + n)
        exp = U.undistort_keypoints(as_ref(cam), kps)
        keep = kps.copy()
        got = cam.undistort_keypoints(kps)                                  # out of place
        assert same_bits(got, exp), "%s n=%d: differs at %r" % (name, n, np.nonzero(got != exp)[0][:8])
        assert kps.tobytes() == keep.tobytes()
        for f in ("size", "angle", "response", "octave"):                   # only pt changes (Frame.cc:721-724)
            assert got[f].tobytes() == kps[f].tobytes()
        if n:
            assert (got["x"] != kps["x"]).any()
        inplace = kps.copy()
        assert cam.undistort_keypoints(inplace, out=inplace) is inplace     # in place
        assert same_bits(inplace, exp)


def test_undistort_keypoints_without_k1_copies(iv):
    from iv_slam_amd.camera import Camera
    cam = Camera(517.3, 516.5, 318.6, 255.3, [0.0, -0.95, -0.005, 0.0026, 1.16])
    kps = random_keypoints(500, 640, 480, seed=5)
    assert cam.undistort_keypoints(kps).tobytes() == kps.tobytes()


def test_batched_device_entry_respects_the_counts(iv):
    import torch
    from iv_slam_amd._lib import KP_DTYPE
    dev = torch.device("cuda:0")
    frames, cap = 8, 1000
    counts = np.array([0, 1, 999, 1000, 500, 64, 257, 1000], np.int32)
    for name in ("EuRoC", "seeded8"):
        cam = seeded_camera8() if name == "seeded8" else load_camera(name)
        kps = random_keypoints(frames * cap, 752, 480, seed=9).reshape(frames, cap)
        sentinel = np.zeros((frames, cap), KP_DTYPE)
        sentinel.view(np.uint32)[:] = 0xDEADBEEF
        exp = sentinel.copy()
        for f in range(frames):
            exp[f, :counts[f]] = U.undistort_keypoints(as_ref(cam), kps[f, :counts[f]])
        d_in = torch.from_numpy(kps.view(np.uint8).reshape(-1).copy()).to(dev)
        d_cnt = torch.from_numpy(counts).to(dev)
        d_out = torch.from_numpy(sentinel.view(np.uint8).reshape(-1).copy()).to(dev)
        cam.undistort_keypoints_device(d_in.data_ptr(), d_cnt.data_ptr(), frames, cap, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(KP_DTYPE).reshape(frames, cap)
        assert same_bits(got, exp), "%s: frames that differ %r" % (name, [f for f in range(frames) if got[f].tobytes() != exp[f].tobytes()])
        assert d_in.cpu().numpy().tobytes() == kps.tobytes()
        # in place: slots past the count keep the input
        cam.undistort_keypoints_device(d_in.data_ptr(), d_cnt.data_ptr(), frames, cap, d_in.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_in.cpu().numpy().view(KP_DTYPE).reshape(frames, cap)
        for f in range(frames):
            assert same_bits(got[f, :counts[f]], exp[f, :counts[f]]) and got[f, counts[f]:].tobytes() == kps[f, counts[f]:].tobytes()
    # a camera whose k1 is 0 copies the keypoints below each count and nothing else
    from iv_slam_amd.camera import Camera
    off = Camera(500, 500, 320, 240, [0.0, 0.3, 0.001, 0.001])
    d_in = torch.from_numpy(kps.view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.from_numpy(sentinel.view(np.uint8).reshape(-1).copy()).to(dev)
    off.undistort_keypoints_device(d_in.data_ptr(), d_cnt.data_ptr(), frames, cap, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(KP_DTYPE).reshape(frames, cap)
    for f in range(frames):
        assert got[f, :counts[f]].tobytes() == kps[f, :counts[f]].tobytes() and got[f, counts[f]:].tobytes() == sentinel[f, counts[f]:].tobytes()


def sequence(name, frames=8, shift=3):
    """consecutive frames of one synthetic scene shifted `shift` px per frame, left and right"""
    (w, h), bf, seed = RIGS[name]
    L, R = synth.make_pair(w, h, seed=seed, idx=0)
    lefts = np.stack([np.roll(L, shift * k, axis=1) for k in range(frames)]); rights = np.stack([np.roll(R, shift * k, axis=1) for k in range(frames)])
    return lefts, rights


def make_frontend(iv, name, frames=8):
    (w, h), bf, _ = RIGS[name]
    cam = load_camera(name)
    return iv.StereoFrontend(w, h, frames, nfeatures=1000, bf=bf, fx=float(cam.fx)), cam


def fetch_all(fe, n, undistorted=False, age=0):
    return [fe.fetch(k, 0, age=age, undistorted=undistorted) for k in range(n)], [fe.fetch(k, 1, age=age) for k in range(n)]


def pack(fe, frames, age=0):
    import torch
    block = torch.zeros(frames * fe.gather_record_bytes(), dtype=torch.uint8, device=torch.device("cuda:0"))
    fe.pack_gather_block(block, age=age)
    fe.sync(); torch.cuda.synchronize()
    return block


@pytest.mark.parametrize("name", ["EuRoC", "TUM1"])
def test_frontend_with_a_camera(iv, name):
    """mvKeysUn = restatement(mvKeys) for two consecutive runs; everything a run produced before is byte-equal to a handle without
    a camera; set_camera(None) and a k1 == 0 camera give the records of a handle that never had one; records carry mvKeysUn."""
    import torch
    from iv_slam_amd.camera import Camera
    from iv_slam_amd.frontend import unpack_gather_records
    dev = torch.device("cuda:0")
    frames = 8
    lefts, rights = sequence(name, frames)
    dL = torch.from_numpy(lefts).to(dev); dR = torch.from_numpy(rights).to(dev)
    dL2 = torch.from_numpy(np.ascontiguousarray(lefts[::-1])).to(dev); dR2 = torch.from_numpy(np.ascontiguousarray(rights[::-1])).to(dev)
    fe, cam = make_frontend(iv, name, frames)
    plain, _ = make_frontend(iv, name, frames)
    fe.set_camera(cam)
    fe.run(dL, dR); fe.run(dL2, dR2)                                         # two consecutive runs, both held
    plain.run(dL, dR); plain.run(dL2, dR2)
    fe.sync(); plain.sync()
    for age in (1, 0):
        gl, gr = fetch_all(fe, frames, undistorted=True, age=age)
        pl, pr = fetch_all(plain, frames, age=age)
        for k in range(frames):
            for key in ("kps", "desc", "uright", "depth", "quality"):
                assert gl[k][key].tobytes() == pl[k][key].tobytes(), "%s run age %d pair %d: left %s changed by the camera" % (name, age, k, key)
            for key in ("kps", "desc", "quality"):
                assert gr[k][key].tobytes() == pr[k][key].tobytes()
            assert len(gl[k]["kps"]) > 300
            exp = U.undistort_keypoints(as_ref(cam), gl[k]["kps"])
            assert same_bits(gl[k]["kps_un"], exp), "%s run age %d pair %d: mvKeysUn differs from the restatement" % (name, age, k)
        recs = unpack_gather_records(pack(fe, frames, age).cpu().numpy(), 1000)
        precs = unpack_gather_records(pack(plain, frames, age).cpu().numpy(), 1000)
        for k in range(frames):
            assert recs[k]["kps"].tobytes() == gl[k]["kps_un"].tobytes()       # the records carry mvKeysUn ...
            for key in ("desc", "uright", "depth"):                            # ... and nothing else changes
                assert recs[k][key].tobytes() == precs[k][key].tobytes()
            assert precs[k]["kps"].tobytes() == pl[k]["kps"].tobytes()
    assert fe.undistorted_device_ptr(0) != fe.undistorted_device_ptr(1)
    # without a camera a run has no mvKeysUn buffer, and fetch(..., undistorted=True) returns mvKeys (Frame.cc:698-702)
    with pytest.raises(iv.IvfError):
        plain.undistorted_device_ptr(0)
    assert plain.fetch(0, 0, undistorted=True)["kps_un"].tobytes() == pl[0]["kps"].tobytes()
    # switching the camera off again / a camera that does not undistort: records byte-equal to the handle that never had one
    want = pack(plain, frames).cpu().numpy().tobytes()
    for off in (None, Camera(cam.fx, cam.fy, cam.cx, cam.cy, [0.0] + [float(v) for v in cam.dist[1:]])):
        fe.set_camera(cam); fe.run(dL, dR)
        fe.set_camera(off); fe.run(dL2, dR2)
        assert pack(fe, frames).cpu().numpy().tobytes() == want
        assert fe.fetch(3, 0, undistorted=True)["kps_un"].tobytes() == pl[3]["kps"].tobytes()
        recs = unpack_gather_records(pack(fe, frames, age=1).cpu().numpy(), 1000)     # the run before still holds its mvKeysUn
        assert recs[2]["kps"].tobytes() != fe.fetch(2, 0, age=1)["kps"].tobytes()


@pytest.mark.parametrize("name", ["EuRoC", "TUM1"])
def test_tracker_on_undistorted_records(iv, name):
    """gather records of a front end with a camera -> ivf_tracker_run with bounds = ivf_image_bounds == the projection oracle fed
    the same undistorted keypoints and bounds.  Checked on the CPU with the oracle alone before this ran on a GPU: every pair of
    both rigs has well over retry_below matches (EuRoC 184-210, TUM1 387-407 on the first pairs) and EuRoC's frames hold more than 30
    keypoints at an undistorted x < 0."""
    from test_gpu_track import check_pairs, run_tracker, scale_table
    from iv_slam_amd.frontend import unpack_gather_records
    import torch
    dev = torch.device("cuda:0")
    frames = 8
    (w, h), bf, _ = RIGS[name]
    lefts, rights = sequence(name, frames)
    fe, cam = make_frontend(iv, name, frames)
    fe.set_camera(cam)
    fe.run(torch.from_numpy(lefts).to(dev), torch.from_numpy(rights).to(dev))
    recs = unpack_gather_records(pack(fe, frames).cpu().numpy(), 1000)
    bounds = cam.image_bounds(w, h)
    assert np.array_equal(np.array(bounds, F).view(np.uint32), np.array(U.image_bounds(as_ref(cam), w, h), F).view(np.uint32))
    for k in range(frames):                                                  # the same undistorted keypoints the oracle is fed
        assert same_bits(recs[k]["kps"], U.undistort_keypoints(as_ref(cam), fe.fetch(k, 0)["kps"]))
    tcam = dict(nf=1000, scale=scale_table(), fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=F(bf), b=F(F(bf) / cam.fx),
                bounds=tuple(float(v) for v in bounds))
    pairs = [(k, k + 1) for k in range(frames - 1)] + [(4, 1)]
    retry_below = 20
    assign, nm = run_tracker(iv, tcam, recs, pairs, retry_below=retry_below)
    check_pairs(tcam, recs, pairs, assign, nm, retry_below=retry_below, what=name)
    print(name, "matches per pair", nm.tolist(), "bounds", tcam["bounds"])
    assert (nm > retry_below).any(), "vacuous: no pair has more than retry_below matches"
    if name == "EuRoC":
        assert bounds[0] < 0 and bounds[1] < 0
        neg = [int(((r["kps"]["x"] < 0) | (r["kps"]["y"] < 0)).sum()) for r in recs]
        print("EuRoC keypoints at a negative undistorted coordinate per frame", neg)
        assert max(neg) >= 1, "vacuous: no keypoint left of / above the distorted image's origin"
        matched_neg = sum(int(((recs[b]["kps"]["x"][:len(recs[b]["kps"])] < 0) & (assign[p, :len(recs[b]["kps"])] >= 0)).sum()) for p, (a, b) in enumerate(pairs))
        print("EuRoC matched keypoints at x < 0:", matched_neg)


def test_resident_frame_grid_with_a_negative_origin(iv):
    """ivf_frame_create_from_frontend + ivf_frame_grid with EuRoC's bounds = AssignFeaturesToGrid of mvKeysUn (Frame.cc:415-430)"""
    from test_gpu_frame import _np_grid
    import torch
    dev = torch.device("cuda:0")
    frames = 8
    (w, h), _, _ = RIGS["EuRoC"]
    lefts, rights = sequence("EuRoC", frames)
    fe, cam = make_frontend(iv, "EuRoC", frames)
    fe.set_camera(cam)
    fe.run(torch.from_numpy(lefts).to(dev), torch.from_numpy(rights).to(dev))
    bounds = tuple(float(v) for v in cam.image_bounds(w, h))
    assert bounds[0] < 0 and bounds[1] < 0
    for pair in (0, 5):
        got = fe.fetch(pair, 0, undistorted=True)
        un = got["kps_un"]
        assert same_bits(un, U.undistort_keypoints(as_ref(cam), got["kps"])) and (un["x"] < 0).any()
        f = iv.DeviceFrame.from_frontend(fe, pair, 0, bounds)
        st, ix = f.grid()
        es, ei = _np_grid(un, bounds)
        assert np.array_equal(st, es) and np.array_equal(ix, ei)
        # the C oracle's GetFeaturesInArea on mvKeysUn agrees with the grid's content around a keypoint left of the origin
        i = int(np.argmin(un["x"]))
        near = O.features_in_area(un, bounds, float(un["x"][i]), float(un["y"][i]), 30.0, -1, -1)
        assert i in set(int(v) for v in near)
        # the right frame is never undistorted (Frame.cc:145: left keypoints only)
        fr = iv.DeviceFrame.from_frontend(fe, pair, 1, (0.0, 0.0, float(w), float(h)))
        rs, ri = fr.grid()
        es, ei = _np_grid(fe.fetch(pair, 1)["kps"], (0.0, 0.0, float(w), float(h)))
        assert np.array_equal(rs, es) and np.array_equal(ri, ei)
