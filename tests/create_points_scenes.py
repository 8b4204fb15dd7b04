"""create_points_scenes.py -- hand-made scenes for the batched CreateNewMapPoints (test infrastructure only), shared by
tests/test_create_points_cpu.py (the restatement meets every expectation, every stage code is reached, every injected fault is caught) and
tests/test_gpu_create_points.py (ivf_tracker_create_map_points byte for byte against the restatement).  Everything is drawn from fixed seeds.

The camera has fx = fy = 512 and bf = 256, the stereo depths are powers of two and the poses of the exact scenes are translations: the
UnprojectStereo branches are then pure float arithmetic without a rounding, and a depth, a right coordinate or a translation can be put ON
a gate and one float beside it (straddle()).  Scenes whose matches go through the SVD stay one clear step away from every gate.  Where a
scene passes F12 itself it is the line y = y0 for every keypoint of the current keyframe (a = 0, b = 1, c = -y0): every neighbour keypoint
on that row passes CheckDistEpipolarLine with a distance of exactly 0, whatever the geometry."""
import numpy as np

import create_points_ref as R
import track_bow_scenes as TB
from projection_ref import F, neg_rt_mul, scale_table

NF = 64
TREE = TB.TREES[3]
LEVELSUP = 1
KP_DTYPE = TB.KP_DTYPE
CAM = dict(fx=F(512.0), fy=F(512.0), cx=F(320.0), cy=F(240.0), bf=F(256.0), b=F(0.5), scale=scale_table(8, 1.2), bounds=(0.0, 0.0, 640.0, 480.0))
Y0 = 240.0
I3 = np.eye(3, dtype=F)


def pose(Ow, Rm=I3):
    """Tcw [3, 4] of a camera with rotation Rcw = Rm at the centre Ow"""
    Rm = np.asarray(Rm, F)
    t = (-(Rm.astype(np.float64) @ np.asarray(Ow, np.float64))).astype(F)
    return np.concatenate([Rm, t.reshape(3, 1)], axis=1).astype(F)


def line_f12(y0=Y0):
    f = np.zeros(9, F); f[7] = 1.0; f[8] = -F(y0)
    return f


def straddle(refused, lo, hi):
    """adjacent floats (a, b) between lo and hi with refused(a) != refused(b), by bisection on the float32 bit patterns (same sign)"""
    a, b = np.array([lo, hi], F).view(np.uint32).astype(np.int64)
    ra = refused(F(lo))
    assert ra != refused(F(hi))
    while abs(b - a) > 1:
        m = (a + b) // 2
        if refused(np.array([m], np.int64).astype(np.uint32).view(F)[0]) == ra:
            a = m
        else:
            b = m
    return tuple(np.array([a, b], np.int64).astype(np.uint32).view(F))


class Rec:
    """one gather record under construction"""

    def __init__(self):
        self.f = []

    def add(self, x, y, desc, octave=0, ur=-1.0, depth=-1.0):
        self.f.append((F(x), F(y), int(octave), F(ur), F(depth), desc)); return len(self.f) - 1

    def stereo(self, x, y, desc, depth, octave=0, dur=0.0):
        """a keypoint with the right coordinate of its depth (+ dur)"""
        return self.add(x, y, desc, octave, F(F(F(x) - F(CAM["bf"] / F(depth))) + F(dur)), depth)

    def done(self):
        n = len(self.f)
        kp = np.zeros(n, KP_DTYPE)
        kp["x"] = [f[0] for f in self.f]; kp["y"] = [f[1] for f in self.f]; kp["octave"] = [f[2] for f in self.f]; kp["size"] = 31
        return dict(kps=kp, desc=np.array([f[5] for f in self.f], np.uint8).reshape(n, 32), uright=np.array([f[3] for f in self.f], F),
                    depth=np.array([f[4] for f in self.f], F))


class Scene:
    def __init__(self, name, seed, n_rec):
        self.name = name; self.b = TB.Builder(TREE, seed); self.recs = [Rec() for _ in range(n_rec)]
        self.node = self.b.nodes[seed % len(self.b.nodes)]
        self.expect = {}; self.has = {}

    def twins(self, flips=3):
        """a descriptor and its twin at Hamming distance `flips`, far from every other pair"""
        p = self.b.payload()
        return self.b.desc(self.node, p), self.b.desc(self.node, self.b.flipped(p, self.b.pick(flips)))

    def finish(self, poses, kf, neigh, F12=None, quality=False, kf_order=None):
        recs = [r.done() for r in self.recs]
        n = len(recs)
        has = np.zeros((n, NF), np.uint8)
        for (r, i), v in self.has.items():
            has[r, i] = v
        kq = np.random.default_rng(7).uniform(0.1, 1.0, (n, NF)).astype(F) if quality else None
        return dict(name=self.name, records=recs, poses=np.stack(poses).astype(F), has_point=has, kf=kf, neigh=list(neigh),
                    F12=None if F12 is None else np.stack(F12).astype(F), key_quality=kq, kf_order=kf_order, expect=self.expect)


def project(T, X):
    Xc = T[:3, :3].astype(np.float64) @ np.asarray(X, np.float64) + T[:3, 3]
    return float(CAM["fx"]) * Xc[0] / Xc[2] + float(CAM["cx"]), float(CAM["fy"]) * Xc[1] / Xc[2] + float(CAM["cy"]), Xc[2]


def svd_scene():
    """computed F12, sideways motion with a small rotation, true 3D points: every match goes through the SVD, one clear step from the gates"""
    s = Scene("svd_real", 1, 2)
    c, sn = np.cos(0.05), np.sin(0.05)
    T = [pose((0, 0, 0)), pose((1.0, 0.1, 0.0), [[c, 0, sn], [0, 1, 0], [-sn, 0, c]])]
    rng = np.random.default_rng(5)

    def pair(X, o1=0, o2=0, stereo1=False):
        d1, d2 = s.twins()
        u1, v1, z1 = project(T[0], X); u2, v2, _ = project(T[1], X)
        i1 = s.recs[0].stereo(u1, v1, d1, z1, o1) if stereo1 else s.recs[0].add(u1, v1, d1, o1)
        s.recs[1].add(u2, v2, d2, o2)
        return i1
    for _ in range(6):
        s.expect[(0, pair((rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(8, 14))))] = R.BY_SVD
    s.expect[(0, pair((1.0, 0.5, 300.0)))] = R.LOW_PARALLAX                  # cos of 1 / 300 rad is above 0.9998
    s.expect[(0, pair((0.5, 0.5, 10.0), o1=4, o2=0))] = R.RATIO_LOW           # 1.2^4 = 2.07 against ratioDist * 1.8 = 1.8
    s.expect[(0, pair((-0.5, 0.5, 10.0), o1=0, o2=4))] = R.RATIO_HIGH
    s.expect[(0, pair((0.3, -0.4, 9.0), stereo1=True))] = R.BY_SVD            # a stereo keypoint whose rays still have more parallax
    s.recs[1].add(50.0, 50.0, s.b.desc(s.node, s.b.payload()))               # nobody's twin
    return s.finish(T, 0, [1], quality=True)


def chi2_svd_scene():
    """SVD matches whose rows disagree (F12 given: the epipolar gate cannot refuse them): the least-squares point splits the error"""
    s = Scene("svd_chi2", 2, 2)
    T = [pose((0, 0, 0)), pose((1.0, 0.0, 0.0))]

    def pair(X, dy1, o1, o2):
        d1, d2 = s.twins()
        u1, v1, _ = project(T[0], X); u2, _, _ = project(T[1], X)
        s.recs[1].add(u2, Y0, d2, o2)
        return s.recs[0].add(u1, Y0 + dy1, d1, o1)
    s.expect[(0, pair((0.5, 0.0, 10.0), 20.0, 0, 0))] = R.CHI2_1_MONO        # 10 px in each image against 2.4
    s.expect[(0, pair((-0.5, 0.0, 10.0), 8.0, 7, 7))] = R.BY_SVD             # 4 px in each against 8.7
    s.expect[(0, pair((0.0, 0.0, 10.0), 8.0, 7, 0))] = R.CHI2_2_MONO         # 16 passes 5.991 * 1.2^14 = 77 in the keyframe and fails 5.991 in the neighbour
    return s.finish(T, 0, [1], F12=[line_f12()])


def forward_pair(s, r2, x1, o1=0, o2=1, depth=8.0, dx2=0.0, stereo2=False, dur1=0.0, dur2=0.0, c2=4.0, flips=3, d=None):
    """a stereo keypoint of record 0 on row Y0 at `depth` and its image in a camera c2 ahead of it (identity rotations): exact floats"""
    d1, d2 = d or s.twins(flips)
    i1 = s.recs[0].stereo(x1, Y0, d1, depth, o1, dur1)
    z2 = depth - c2
    x2 = float(CAM["cx"]) + (x1 - float(CAM["cx"])) * depth / z2 + dx2
    i2 = s.recs[r2].stereo(x2, Y0, d2, z2, o2, dur2) if stereo2 else s.recs[r2].add(x2, Y0, d2, o2)
    return i1, i2


def stereo_scene():
    """forward motion, F12 given: the rays of a point near the axis are almost parallel, so UnprojectStereo decides; exact floats"""
    s = Scene("stereo_forward", 3, 2)
    T = [pose((0, 0, 0)), pose((0, 0, 4.0))]
    E = s.expect
    E[(0, forward_pair(s, 1, 322.0)[0])] = R.BY_STEREO1
    E[(0, forward_pair(s, 1, 316.0, dx2=2.0)[0])] = R.BY_STEREO1              # 4 < 5.991 * 1.44
    E[(0, forward_pair(s, 1, 314.0, dx2=3.0)[0])] = R.CHI2_2_MONO             # 9 > 8.63
    E[(0, forward_pair(s, 1, 312.0, o2=0, dx2=2.5)[0])] = R.CHI2_2_MONO       # 6.25 between 5.991 and 7.8: `7.8` for a mono keypoint lets it pass
    E[(0, forward_pair(s, 1, 324.0, dur1=2.5)[0])] = R.BY_STEREO1             # 6.25 < 7.8
    E[(0, forward_pair(s, 1, 326.0, dur1=3.0)[0])] = R.CHI2_1_STEREO          # 9 > 7.8
    # both stereo: only the current keyframe's cosine is computed (:377-380), although the neighbour is closer
    E[(0, forward_pair(s, 1, 328.0, stereo2=True)[0])] = R.BY_STEREO1
    E[(0, forward_pair(s, 1, 330.0, stereo2=True, dur2=3.0, o2=0)[0])] = R.CHI2_2_STEREO
    E[(0, forward_pair(s, 1, 332.0, stereo2=True, dur2=3.0)[0])] = R.BY_STEREO1
    # the current keypoint mono, the neighbour's stereo: UnprojectStereo(2)
    d1, d2 = s.twins()
    i1 = s.recs[0].add(334.0, Y0, d1, 0); s.recs[1].stereo(320.0 + 14.0 * 2.0, Y0, d2, 4.0, 1)
    E[(0, i1)] = R.BY_STEREO2
    # both mono near the axis: nothing to fall back on
    d1, d2 = s.twins()
    i1 = s.recs[0].add(326.0, Y0, d1, 0); s.recs[1].add(320.0 + 6.0 * 2.0, Y0, d2, 1)
    E[(0, i1)] = R.LOW_PARALLAX
    # z: a right coordinate with a depth of exactly 0 puts the point into the camera centre, z1 == 0; a depth of 4 into the neighbour's, z2 == 0
    d1, d2 = s.twins()
    i1 = s.recs[0].add(330.0, Y0, d1, 0, ur=300.0, depth=0.0); s.recs[1].add(100.0, Y0, d2, 0)
    E[(0, i1)] = R.Z1
    d1, d2 = s.twins()
    i1 = s.recs[0].add(320.0, Y0, d1, 0, ur=256.0, depth=4.0); s.recs[1].add(110.0, Y0, d2, 0)
    E[(0, i1)] = R.Z2
    d1, d2 = s.twins()
    i1 = s.recs[0].stereo(320.0, Y0, d1, np.nextafter(F(4.0), F(5.0))); s.recs[1].add(320.0, Y0, d2, 0)
    E[(0, i1)] = R.RATIO_LOW                                                  # one float behind it: z2 > 0, the point is at the lens
    return s.finish(T, 0, [1], F12=[line_f12()], quality=True)


def gate_scene():
    """one on-axis stereo keypoint at depth 8 per neighbour, the neighbour on the axis at c: the chi-square and scale gates ON their limit
    and one float beside it.  ratioDist = (8 - c) / 8 against ratioOctave = 1."""
    s = Scene("exact_gates", 4, 9)
    T = [pose((0, 0, 0))]
    d = s.twins()
    s.recs[0].stereo(320.0, Y0, d[0], 8.0, 0)

    def stage_at(c, dur=0.0, o1=0, o2=0, info=False):
        s1 = R.triangulate(CAM, T[0], pose((0, 0, c)), np.zeros(3, F), np.array([0, 0, c], F), dict(x=F(320), y=F(Y0), octave=o1),
                           F(F(320.0 - 32.0) + F(dur)), F(8.0), dict(x=F(320), y=F(Y0), octave=o2), F(-1), F(-1))
        return s1 if info else s1[0]
    lo = straddle(lambda c: stage_at(c) == R.RATIO_LOW, 1.0, 7.0)               # created below, RATIO_LOW from here on
    hi = straddle(lambda c: stage_at(c) == R.RATIO_HIGH, -1.0, -20.0)           # behind the keyframe: ratioDist > 1.8
    for r, c in enumerate(lo + hi):
        T.append(pose((0, 0, c))); s.recs[1 + r].add(320.0, Y0, d[1], 0)
        s.expect[(r, 0)] = stage_at(c)
    assert [s.expect[(r, 0)] for r in range(4)] == [R.BY_STEREO1, R.RATIO_LOW, R.BY_STEREO1, R.RATIO_HIGH]
    return s, T


def exact_scenes():
    """gate_scene's neighbours cannot share one keyframe (each creates the point and blocks the next): one slot per neighbour"""
    s, T = gate_scene()
    out = []
    for r in range(4):
        sc = Scene("exact_ratio_%d" % r, 4, 2)
        sc.recs[0].f = list(s.recs[0].f); sc.recs[1].f = list(s.recs[1 + r].f)
        sc.expect[(0, 0)] = s.expect[(r, 0)]
        out.append(sc.finish([T[0], T[1 + r]], 0, [1], F12=[line_f12()]))
    out += chi_window_scenes()
    return out


def chi_window_scenes():
    """The chi-square of a mono neighbour keypoint ON its limit.  The neighbour stands 4 ahead on the axis and looks aside, so that the
    on-axis point at depth 8 projects near u = 0, where the floats are fine: errX moves in steps whose squares are closer than the floats
    around 5.991 sigma^2.  Two scenes one step of errX apart: the largest sum that passes, and the float above 5.991 sigma^2, which
    a compare against the FLOAT product 5.991f * sigma^2 would still let pass."""
    c, sn = F(512.0 / np.hypot(512.0, 320.0)), F(320.0 / np.hypot(512.0, 320.0))
    T1 = pose((0, 0, 0)); T2 = pose((0, 0, 4.0), [[c, 0, -sn], [0, 1, 0], [sn, 0, c]])
    x3D = np.array([0.0, 0.0, 8.0], F)
    z2 = F(R.dot3(T2[2, :3], x3D) + float(T2[2, 3]))
    x = F(R.dot3(T2[0, :3], x3D) + float(T2[0, 3])); invz = F(np.float64(1.0) / np.float64(z2))
    u = F(F(F(CAM["fx"] * x) * invz) + CAM["cx"])
    found = {}
    # the octave pairs (o2 - 1, o2) are tried in turn: for some the float product lies below 5.991 sigma^2, for some no square lands there
    for o2 in range(1, 8):
        sig = F(CAM["scale"][o2] * CAM["scale"][o2]); lim = 5.991 * float(sig)
        bits = int(np.array([F(u + F(np.sqrt(lim)))], F).view(np.int32)[0])
        found = {}
        for step in range(-400, 400):
            k = np.array([bits + step], np.int32).view(F)[0]
            refused, ssum = R._reprojection(CAM, T2, x3D, z2, dict(x=k, y=F(Y0)), F(-1), False, sig, None)
            if refused and not ssum > F(F(5.991) * sig):
                found["refused"] = k
            if not refused and ("passes" not in found or ssum >= best):
                found["passes"] = k; best = ssum               # the largest sum of the scan that passes: one step of errX beside
        if len(found) == 2:
            break
    assert len(found) == 2, "no keypoint puts the sum on 5.991 sigma^2: %r" % (found,)
    out = []
    for n, name in enumerate(("passes", "refused")):
        sc = Scene("exact_chi2_%d" % n, 4, 2)
        d = sc.twins()
        sc.recs[0].stereo(320.0, Y0, d[0], 8.0, o2 - 1); sc.recs[1].add(found[name], Y0, d[1], o2)
        sc.expect[(0, 0)] = (R.BY_STEREO1, R.CHI2_2_MONO)[n]
        out.append(sc.finish([T1, T2], 0, [1], F12=[line_f12()]))
    return out


def baseline_scene():
    """baseline == b is not `<`: the neighbour takes part; one float less and it is skipped"""
    s = Scene("baseline", 5, 3)
    below = np.nextafter(F(0.5), F(0.0))
    T = [pose((0, 0, 0)), pose((below, 0, 0)), pose((0.5, 0, 0))]
    for r in (1, 2):
        d1, d2 = s.twins()
        s.recs[0].stereo(300.0 + 20 * r, Y0, d1, 8.0); s.recs[r].add(300.0 + 20 * r - 32.0, Y0, d2, 0)
    s.expect[(0, 0)] = R.BASELINE; s.expect[(0, 1)] = R.BASELINE
    s.expect[(1, 0)] = R.NONE                                                 # its twin lives in the skipped neighbour
    s.expect[(1, 1)] = None                                                   # matched: whatever the geometry says, but not NONE / BASELINE
    return s.finish(T, 0, [1, 2], F12=[line_f12(), line_f12()])


def ranks_scene(order):
    """the serial dependence between the ranks of one keyframe, the shared idx2, the last equal minimum, a -1 and an out-of-range neighbour,
    key qualities, and kf_order in the given direction"""
    s = Scene("ranks_" + ("reversed" if order else "identity"), 6, 3)
    T = [pose((0, 0, 0)), pose((0, 0, 4.0)), pose((0, 0, 4.0))]
    E = s.expect
    # a: refused at rank 0 (its image there is 3 px off), created at rank 1; b, behind it in the record, created at rank 0 and skipped at rank 1
    da = s.twins(); db = s.twins()
    a, _ = forward_pair(s, 1, 322.0, dx2=3.0, d=da); s.recs[2].add(320.0 + 2.0 * 2.0, Y0, da[1], 1)
    b, _ = forward_pair(s, 1, 324.0, d=db); s.recs[2].add(320.0 + 4.0 * 2.0, Y0, db[1], 1)
    E[(0, a)] = R.CHI2_2_MONO; E[(2, a)] = R.BY_STEREO1; E[(0, b)] = R.BY_STEREO1; E[(2, b)] = R.NONE
    # c and e take the same idx2
    p = s.b.payload(); base = s.b.desc(s.node, p)
    c = s.recs[0].stereo(326.0, Y0, s.b.desc(s.node, s.b.flipped(p, s.b.pick(2))), 8.0)
    e = s.recs[0].stereo(326.0, Y0, s.b.desc(s.node, s.b.flipped(p, s.b.pick(3))), 8.0)
    s.shared = s.recs[1].add(320.0 + 6.0 * 2.0, Y0, base, 1)
    E[(0, c)] = R.BY_STEREO1; E[(0, e)] = R.BY_STEREO1
    # g: two candidates at the same distance, the later one wins (the earlier one is 3 px off and would be refused)
    p = s.b.payload(); x = s.b.pick(3); y = s.b.pick(3, avoid=x)
    g = s.recs[0].stereo(328.0, Y0, s.b.desc(s.node, p), 8.0)
    s.recs[1].add(320.0 + 8.0 * 2.0 + 3.0, Y0, s.b.desc(s.node, s.b.flipped(p, x)), 1)
    s.recs[1].add(320.0 + 8.0 * 2.0, Y0, s.b.desc(s.node, s.b.flipped(p, y)), 1)
    E[(0, g)] = R.BY_STEREO1
    # h holds a point already; its twin is free
    dh = s.twins()
    h, _ = forward_pair(s, 1, 330.0, d=dh); s.has[(0, h)] = 1
    E[(0, h)] = R.NONE
    # a neighbour keypoint that holds a point takes no part either
    dj = s.twins()
    j, j2 = forward_pair(s, 1, 332.0, d=dj); s.has[(1, j2)] = 1
    E[(0, j)] = R.NONE
    return s.finish(T, 0, [1, -1, 2, 99], F12=[line_f12()] * 4, quality=True, kf_order=np.array([2, 1, 0], np.int32) if order else None)


def dist_zero_scene():
    """x3D == the neighbour's centre although z2 > 0: Ow = -R^T t and z2 = r3 . x3D + tz round differently.  The translation is searched
    for among the floats around -R x3D; the neighbour keypoint sits where that point projects, whatever that is."""
    x3D = np.array([1.0, 0.0, 8.0], F)                                         # UnprojectStereo of (384, Y0) at depth 8 under the identity
    T1 = pose((0, 0, 0))
    kp1 = dict(x=F(384.0), y=F(Y0), octave=0)
    # the neighbour looks elsewhere (rotations about y from 0.3 rad on), so that the two rays have no parallax to triangulate with
    for ang, k, m in ((0.3 + 0.1 * a, k, m) for a in range(28) for k in range(-3, 4) for m in range(-3, 4)):
        c, sn = F(np.cos(ang)), F(np.sin(ang))
        Rm = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], F)
        t0 = (-(Rm.astype(np.float64) @ x3D.astype(np.float64))).astype(F)
        t = t0.copy()
        for _ in range(abs(k)):
            t[0] = np.nextafter(t[0], F(np.sign(k) * 1e9))
        for _ in range(abs(m)):
            t[2] = np.nextafter(t[2], F(np.sign(m) * 1e9))
        T2 = np.concatenate([Rm, t.reshape(3, 1)], axis=1).astype(F)
        Ow2 = neg_rt_mul(Rm, t)
        z2 = F(R.dot3(Rm[2], x3D) + float(t[2]))
        if Ow2.tobytes() != x3D.tobytes() or not z2 > 0:
            continue
        with np.errstate(all="ignore"):
            x2 = F(R.dot3(Rm[0], x3D) + float(t[0])); y2 = F(R.dot3(Rm[1], x3D) + float(t[1])); invz = F(1.0 / float(z2))
            u2 = F(F(F(CAM["fx"] * x2) * invz) + CAM["cx"]); v2 = F(F(F(CAM["fy"] * y2) * invz) + CAM["cy"])
            kp2 = dict(x=u2, y=v2, octave=0)
            code, _ = R.triangulate(CAM, T1, T2, np.zeros(3, F), Ow2, kp1, F(384.0 - 32.0), F(8.0), kp2, F(-1), F(-1))
        if code == R.DIST_ZERO and np.isfinite(u2) and np.isfinite(v2):
            s = Scene("dist_zero", 8, 2)
            d1, d2 = s.twins()
            s.recs[0].stereo(384.0, Y0, d1, 8.0); s.recs[1].add(u2, v2, d2, 0)
            s.expect[(0, 0)] = R.DIST_ZERO
            return s.finish([T1, T2], 0, [1], F12=[line_f12(v2)])
    raise AssertionError("no translation puts the centre on the point with z2 > 0")


def w_zero_scene():
    """the columns of A are orthogonal as they stand, the Jacobi turns nothing, the shortest column is the third: v = (0, 0, 1, 0)"""
    s = Scene("w_zero", 9, 2)
    T = [pose((0, 1.0, 0)), pose((0, -1.0, 0))]
    d1, d2 = s.twins()
    s.recs[0].add(320.0 + 128.0, Y0, d1); s.recs[1].add(320.0 - 128.0, Y0, d2)      # xn = (+-0.25, 0)
    s.expect[(0, 0)] = R.W_ZERO
    return s.finish(T, 0, [1], F12=[line_f12()])


def edge_scenes():
    """a current keyframe outside the block; one whose keypoints all hold a point; one without keypoints"""
    out = []
    s = Scene("bad_keyframe", 10, 2)
    forward_pair(s, 1, 322.0)
    out.append(s.finish([pose((0, 0, 0)), pose((0, 0, 4.0))], 7, [1], F12=[line_f12()]))
    s = Scene("nothing_eligible", 11, 2)
    for x in (322.0, 324.0):
        i1, _ = forward_pair(s, 1, x); s.has[(0, i1)] = 1; s.expect[(0, i1)] = R.NONE
    out.append(s.finish([pose((0, 0, 0)), pose((0, 0, 4.0))], 0, [1], F12=[line_f12()]))
    s = Scene("empty_keyframe", 12, 2)
    s.recs[1].add(100.0, Y0, s.b.desc(s.node, s.b.payload()))
    out.append(s.finish([pose((0, 0, 0)), pose((0, 0, 4.0))], 0, [1]))
    return out


def all_scenes():
    return [svd_scene(), chi2_svd_scene(), stereo_scene()] + exact_scenes() + [baseline_scene(), ranks_scene(False), ranks_scene(True),
                                                                                dist_zero_scene(), w_zero_scene()] + edge_scenes()


def run_ref(sc, fault=None):
    return R.create_new_map_points(CAM, TREE, LEVELSUP, sc["records"], sc["poses"], sc["has_point"], sc["kf"], sc["neigh"], sc["key_quality"], sc["F12"],
                                   sc["kf_order"], fault)
