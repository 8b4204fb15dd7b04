"""projection_scenes.py -- hand-made scenes for the two projection searches of the batched tracker (ivf_tracker_search_local,
ivf_tracker_run): keypoints and map points placed ON every comparison of Frame::isInFrustum, MapPoint::PredictScale, GetFeaturesInArea and
the two ORBmatcher::SearchByProjection loops, and one step beside it.  The camera makes the arithmetic exact: fx = fy = 256, cx = 320,
cy = 120, bf = 128, b = 0.5, a 640 x 240 image, points at depth 4 (u = 320 + 64 x, v = 120 + 64 y, ur = u - 32), identity or pure-translation
poses.  A point ON the optical axis with normal (0, 0, c) has viewCos == c to the bit (4 c / 4 in double) and dist == its depth.

Every scene carries what it was built for: `expect` = (query, outcome code, intermediates by value), `holds` = (current keypoint, the query
that must hold it at the end or -1).  tests/test_projection_scenes_cpu.py checks those against the restatement tests/projection_ref.py and
the C oracle; tests/test_gpu_projection_scenes.py runs the device on the same scenes."""
import numpy as np

import projection_ref as R

F = np.float32
UP, DOWN = F(np.inf), F(-np.inf)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
NF = 256
SCALE = R.scale_table()
CAM = dict(nf=NF, scale=SCALE, fx=F(256.0), fy=F(256.0), cx=F(320.0), cy=F(120.0), bf=F(128.0), b=F(0.5), bounds=(0.0, 0.0, 640.0, 240.0))
I4 = np.eye(4, dtype=F)
_rng = np.random.default_rng(20240)


def nxt(x, to=UP, steps=1):
    x = F(x)
    for _ in range(steps):
        x = np.nextafter(x, to)
    return x


def new_desc():
    """a descriptor of its own: random descriptors lie about 128 bits apart, far beyond TH_HIGH"""
    return _rng.integers(0, 256, 32).astype(np.uint8)


def at_distance(desc, d, shift=0):
    """desc with d bits flipped, starting at bit `shift`"""
    bits = np.unpackbits(desc)
    for j in range(d):
        bits[(shift + j) % 256] ^= 1
    return np.packbits(bits)


def world(u, v, z=4.0):
    """the point that projects to (u, v) from the origin at depth z; exact for the dyadic values the scenes use"""
    return np.array([(u - 320.0) * z / 256.0, (v - 120.0) * z / 256.0, z], F)


def spot(j):
    """projections far enough apart that no window of radius < 20 reaches a neighbour's keypoints"""
    return 48.0 + 48.0 * (j % 12), 40.0 + 40.0 * (j // 12)


def translation(tz):
    T = I4.copy(); T[2, 3] = F(tz)
    return T


def _record(kx, ky, ko, ka, kd, kur, kdepth):
    n = len(kx)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = np.array(kx, F); kps["y"] = np.array(ky, F); kps["octave"] = np.array(ko, np.int32); kps["angle"] = np.array(ka, F)
    kps["size"] = 31; kps["response"] = 20
    return dict(kps=kps, desc=np.array(kd, np.uint8).reshape(n, 32), uright=np.array(kur, F), depth=np.array(kdepth, F))


class _Keys:
    def __init__(self):
        self.kx, self.ky, self.ko, self.ka, self.kd, self.kur, self.kz = [], [], [], [], [], [], []

    def add(self, x, y, octave, desc, ur=-1.0, angle=0.0, depth=-1.0):
        self.kx.append(F(x)); self.ky.append(F(y)); self.ko.append(int(octave)); self.ka.append(F(angle)); self.kd.append(np.array(desc, np.uint8))
        self.kur.append(F(ur)); self.kz.append(F(depth))
        return len(self.kx) - 1

    def record(self):
        assert len(self.kx) <= NF
        return _record(self.kx, self.ky, self.ko, self.ka, self.kd, self.kur, self.kz)


# =================================================================================================================================
# SearchLocalPoints
# =================================================================================================================================
class Local:
    def __init__(self, name, th=1.0, nn_ratio=0.8, cos_limit=0.5, max_points=None):
        self.name, self.th, self.nn_ratio, self.cos_limit, self.max_points = name, th, nn_ratio, cos_limit, max_points
        self.keys = _Keys(); self.occ = []; self.points = []; self.expect = []; self.holds = []
        self.T = I4

    @property
    def group(self):
        return (self.th, self.nn_ratio, self.cos_limit, self.max_points)

    def kp(self, x, y, octave, desc, ur=-1.0, occupied=False):
        self.occ.append(bool(occupied))
        return self.keys.add(x, y, octave, desc, ur)

    def pt(self, pos, desc, lv=0, c=0.9, normal=None, minDist=None, maxDist=None, skip=False, nObs=1):
        """a map point seen from the origin; by default its distance sits in the middle of level lv's interval and its normal points
        along the ray, scaled by c (viewCos ~ c: 0.9 -> radius 4, 1.0 -> radius 2.5)"""
        pos = np.asarray(pos, F)
        dist = float(np.sqrt((pos.astype(np.float64) ** 2).sum()))
        if maxDist is None:
            maxDist = F(dist * 1.2 ** (lv - 0.5))
        if minDist is None:
            minDist = F(F(maxDist) / SCALE[-1])
        if normal is None:
            normal = (pos.astype(np.float64) / dist * c).astype(F)
        self.points.append(dict(pos=pos, normal=np.asarray(normal, F), minDist=F(minDist), maxDist=F(maxDist), desc=np.array(desc, np.uint8),
                                skip=bool(skip), nObs=int(nObs)))
        return len(self.points) - 1

    def want(self, p, outcome, **vals):
        self.expect.append((p, outcome, vals))

    def hold(self, k, p):
        self.holds.append((k, p))

    def done(self):
        self.rec = self.keys.record()
        self.occupied = np.array(self.occ, bool)
        return self

    def simple(self, j, outcome, lv=0, octave=None, d=0, c=0.9, nObs=1, **vals):
        """one point on spot j with one keypoint at its projection, descriptor distance d"""
        u, v = spot(j)
        desc = new_desc()
        p = self.pt(world(u, v), desc, lv=lv, c=c, nObs=nObs)
        k = self.kp(u, v, lv if octave is None else octave, at_distance(desc, d))
        self.want(p, outcome, **vals)
        self.hold(k, p if outcome == R.ACCEPTED else -1)
        return p, k


def _witness_octaves(s, desc, lv, x0, y0):
    """keypoints at octaves lv-2 .. lv+1 around (x0, y0); the ones outside [lv-1, lv] carry the smallest distances, so a level predicted
    one off hands the point to another keypoint.  Returns {octave: keypoint}."""
    out = {}
    for j, (o, d) in enumerate(((lv - 2, 1), (lv - 1, 6), (lv, 4), (lv + 1, 2))):
        if 0 <= o <= 7:
            out[o] = s.kp(x0 + (j % 2), y0 + (j // 2), o, at_distance(desc, d))
    return out


def local_z_sign():
    s = Local("z_sign")
    da, db = new_desc(), new_desc()
    a = s.pt([0, 0, -2.0 ** -20], da, normal=[0, 0, -1])
    b = s.pt([0, 0, 2.0 ** -20], db, normal=[0, 0, 1])
    ka = s.kp(321, 120, 0, da); kb = s.kp(320, 121, 0, db)
    s.want(a, R.BEHIND, pcz=F(-2.0 ** -20)); s.want(b, R.ACCEPTED, pcz=F(2.0 ** -20), u=F(320), v=F(120), level=0, radius=F(2.5), n_window=2)
    s.hold(ka, -1); s.hold(kb, b)
    return s.done()


def local_image_bounds():
    """u = 64 x + 320: x = 5 is u = 640 exactly; the first x above 5 rounds back onto 640 (tie to even), the second is the float after
    640.  x = -5 - 2^-21 is u = -2^-15, the first attainable u below 0.  v likewise with y = +-1.875: 240 + 2^-16 and -2^-17."""
    s = Local("image_bounds", th=3.0)
    for name, pin, pout, wit, uv_in, uv_out in (
            ("right", [5, 0, 4], [nxt(5, UP, 2), 0, 4], (632, 120), (640, 120), (nxt(640), 120)),
            ("left", [-5, 0, 4], [nxt(-5, DOWN), 0, 4], (8, 120), (0, 120), (F(-2.0 ** -15), 120)),
            ("bottom", [0, 1.875, 4], [0, nxt(1.875, UP, 2), 4], (320, 234), (320, 240), (320, nxt(240))),
            ("top", [0, -1.875, 4], [0, nxt(-1.875, DOWN), 4], (320, 6), (320, 0), (320, F(-2.0 ** -17)))):
        di, do = new_desc(), new_desc()
        a = s.pt(pin, di); b = s.pt(pout, do)
        ka = s.kp(wit[0], wit[1], 0, di); kb = s.kp(wit[0], wit[1], 0, do)
        s.want(a, R.ACCEPTED, u=F(uv_in[0]), v=F(uv_in[1]), radius=F(12), n_window=2); s.want(b, R.OUT_OF_IMAGE, u=F(uv_out[0]), v=F(uv_out[1]))
        s.hold(ka, a); s.hold(kb, -1)
    return s.done()


def _first(pred, x, to):
    for _ in range(64):
        if pred(x):
            return x
        x = nxt(x, to)
    raise AssertionError("no float found")


def local_dist_range():
    """on the axis at depth 4: dist == 4.  0.8f * 5 rounds to 4 (dist == 0.8f * minDist: inside); the first minDist above 5 whose product
    exceeds 4 is outside.  Likewise a maxDist with 1.2f * maxDist == 4 and the one below it."""
    s = Local("dist_range")
    near_out = _first(lambda m: F(F(0.8) * m) > F(4), F(5), UP)
    far_in = _first(lambda m: F(F(1.2) * m) == F(4), nxt(F(4.0 / 1.2), DOWN, 8), UP)
    far_out = _first(lambda m: F(F(1.2) * m) < F(4), far_in, DOWN)
    assert F(F(0.8) * F(5)) == F(4)
    for name, mind, maxd, lv, oc in (("near_in", 5, 8, 4, R.ACCEPTED), ("near_out", near_out, 8, 4, R.TOO_NEAR),
                                     ("far_in", 1, far_in, 0, R.ACCEPTED), ("far_out", 1, far_out, 0, R.TOO_FAR)):
        d = new_desc()
        p = s.pt([0, 0, 4], d, normal=[0, 0, 0.75], minDist=mind, maxDist=maxd)
        k = s.kp(320 + len(s.points) - 2, 120, lv, d)
        if oc == R.ACCEPTED:
            s.want(p, oc, dist=F(4), level=lv, view_cos=F(0.75), radius=F(F(4) * SCALE[lv]), n_window=2)
        else:
            s.want(p, oc, dist=F(4))
        s.hold(k, p if oc == R.ACCEPTED else -1)
    return s.done()


def local_view_cos(limit):
    s = Local("view_cos_%g" % limit, cos_limit=limit)
    for c, oc in ((F(limit), R.ACCEPTED), (nxt(F(limit), DOWN), R.VIEW_ANGLE)):
        d = new_desc()
        p = s.pt([0, 0, 4], d, normal=[0, 0, c])
        k = s.kp(320 + len(s.points) - 1, 120, 0, d)
        s.want(p, oc, view_cos=c); s.hold(k, p if oc == R.ACCEPTED else -1)
    return s.done()


def local_radius_cos(th):
    """float32(0.998) lies above the double 0.998: radius 2.5; the float below it: radius 4.  Each point's keypoint sits 3 th away."""
    s = Local("radius_cos_th%g" % th, th=th)
    c = F(0.998)
    assert float(c) > 0.998 > float(nxt(c, DOWN))
    da, db = new_desc(), new_desc()
    a = s.pt([0, 0, 4], da, normal=[0, 0, c]); b = s.pt([0, 0, 4], db, normal=[0, 0, nxt(c, DOWN)])
    ka = s.kp(320 + 3 * th, 120, 0, da); kb = s.kp(320, 120 + 3 * th, 0, db)
    s.want(a, R.EMPTY_WINDOW, view_cos=c, radius=F(2.5 * th), n_window=0, level=0)
    s.want(b, R.ACCEPTED, view_cos=nxt(c, DOWN), radius=F(4.0 * th), n_window=2, level=0)
    s.hold(ka, -1); s.hold(kb, b)
    return s.done()


def scale_quotient(max_dist, dist=4.0):
    return F(R.logf(F(F(max_dist) / F(dist))) / R.logf(SCALE[1]))


def level_edge(k):
    """the two adjacent maxDist floats between which logf(maxDist / 4) / logf(1.2f) passes k: (q <= k, q > k)"""
    m = F(4.0 * 1.2 ** k)
    while scale_quotient(m) > k:
        m = nxt(m, DOWN)
    while scale_quotient(nxt(m)) <= k:
        m = nxt(m)
    return m, nxt(m)


def local_predict_scale(k):
    s = Local("predict_scale_%d" % k)
    lo, hi = level_edge(k)
    rows = []
    for m, lv, dy in ((lo, k, 0), (hi, min(k + 1, 7), 2)):
        d = new_desc()
        p = s.pt([0, 0, 4], d, minDist=1, maxDist=m)
        rows.append((p, lv, _witness_octaves(s, d, lv, 319, 119 + dy)))
    s.edge = (lo, hi)
    n_oct = np.bincount(s.keys.ko, minlength=9)
    for p, lv, w in rows:
        s.want(p, R.ACCEPTED, level=lv, dist=F(4), radius=F(F(4) * SCALE[lv]), n_window=int(n_oct[max(lv - 1, 0):lv + 1].sum()), best_dist=4, best_level=lv)
        if lv > 0:
            s.want(p, R.ACCEPTED, best_dist2=6, best_level2=lv - 1)
        for o, kk in w.items():
            s.hold(kk, p if o == lv else -1)
    return s.done()


def local_scale_clamps():
    """ratio exactly 1 (logf gives 0: level 0), ratio below 1 (negative: clamped to 0), ratio 4 > 1.2^7 (8: clamped to 7)"""
    s = Local("scale_clamps")
    rows = []
    for j, (m, lv) in enumerate(((4.0, 0), (3.5, 0), (16.0, 7))):
        d = new_desc()
        p = s.pt([0, 0, 4], d, minDist=1, maxDist=m)
        rows.append((p, lv, _witness_octaves(s, d, lv, 319, 118 + 2 * j)))
    n_oct = np.bincount(s.keys.ko, minlength=9)
    for p, lv, w in rows:
        s.want(p, R.ACCEPTED, level=lv, radius=F(F(4) * SCALE[lv]), n_window=int(n_oct[max(lv - 1, 0):lv + 1].sum()), best_dist=4)
        for o, kk in w.items():
            s.hold(kk, p if o == lv else -1)
    return s.done()


def local_window_edge():
    """radius 4 (th == 1, level 0): |dx| == 4 is outside (strict <), the float before it inside; the same in y and on the negative side"""
    s = Local("window_edge")
    for j, (sx, sy, inside) in enumerate(((1, 0, False), (1, 0, True), (0, 1, False), (0, 1, True), (-1, 0, False), (-1, 0, True), (0, -1, False),
                                          (0, -1, True))):
        u, v = spot(j)
        d = new_desc()
        p = s.pt(world(u, v), d)
        # the keypoint at u +- 4 exactly, or at the float before it (u + 4 - 2^-22 is no float: the step is one of the keypoint's own)
        x = F(u + 4 * sx); y = F(v + 4 * sy)
        if inside:
            x = nxt(x, F(u)) if sx else x; y = nxt(y, F(v)) if sy else y
        k = s.kp(x, y, 0, d)
        s.want(p, R.ACCEPTED if inside else R.EMPTY_WINDOW, radius=F(4), n_window=1 if inside else 0, u=F(u), v=F(v))
        s.hold(k, p if inside else -1)
    return s.done()


def local_stereo_check():
    """ur = u - 32; radius 4: |ur - uRight| == 4 is admitted (the test is >), the next float is refused; uRight <= 0: no test"""
    s = Local("stereo_check")
    for j, (off, to, ok) in enumerate(((4, None, True), (4, UP, False), (-4, None, True), (-4, DOWN, False))):
        u, v = spot(j)
        d = new_desc()
        p = s.pt(world(u, v), d)
        ur = F(u - 32 + off)
        if to is not None:
            ur = nxt(ur, to)
        k = s.kp(u, v, 0, d, ur=ur)
        s.want(p, R.ACCEPTED if ok else R.ALL_BLOCKED, ur=F(u - 32), radius=F(4), n_window=1, n_admitted=1 if ok else 0)
        s.hold(k, p if ok else -1)
    for j, ur in ((4, 0.0), (5, -1.0), (6, -300.0)):
        u, v = spot(j)
        d = new_desc()
        p = s.pt(world(u, v), d)
        k = s.kp(u, v, 0, d, ur=ur)
        s.want(p, R.ACCEPTED, n_admitted=1); s.hold(k, p)
    return s.done()


def local_occupancy():
    s = Local("occupancy")
    # the best candidate is occupied before the call: the next one wins
    u, v = spot(0); d = new_desc(); p = s.pt(world(u, v), d)
    k1 = s.kp(u, v, 0, d, occupied=True); k2 = s.kp(u + 1, v, 0, at_distance(d, 10))
    s.want(p, R.ACCEPTED, n_window=2, n_admitted=1, best_dist=10, best_dist2=256); s.hold(k1, -1); s.hold(k2, p)
    # a blocked candidate is no second best: 40 alone passes, 40 against 45 would fail the ratio test
    u, v = spot(1); d = new_desc(); p = s.pt(world(u, v), d)
    k1 = s.kp(u, v, 0, at_distance(d, 40)); k2 = s.kp(u + 1, v, 0, at_distance(d, 45, 100), occupied=True)
    s.want(p, R.ACCEPTED, n_window=2, n_admitted=1, best_dist=40, best_dist2=256, best_level2=-1); s.hold(k1, p); s.hold(k2, -1)
    # every candidate blocked
    u, v = spot(2); d = new_desc(); p = s.pt(world(u, v), d)
    k1 = s.kp(u, v, 0, d, occupied=True); k2 = s.kp(u + 1, v, 0, d, occupied=True)
    s.want(p, R.ALL_BLOCKED, n_window=2, n_admitted=0); s.hold(k1, -1); s.hold(k2, -1)
    # a point without observations is overwritten by a later one; nmatches counts both
    u, v = spot(3); d = new_desc(); p1 = s.pt(world(u, v), d, nObs=0); p2 = s.pt(world(u, v), d)
    k = s.kp(u, v, 0, d)
    s.want(p1, R.ACCEPTED_THEN_REPLACED); s.want(p2, R.ACCEPTED, n_admitted=1); s.hold(k, p2)
    # a point with observations blocks the later one
    u, v = spot(4); d = new_desc(); p1 = s.pt(world(u, v), d); p2 = s.pt(world(u, v), d)
    k = s.kp(u, v, 0, d)
    s.want(p1, R.ACCEPTED); s.want(p2, R.ALL_BLOCKED, n_window=1, n_admitted=0); s.hold(k, p1)
    return s.done()


def local_th_high_and_ratio():
    s = Local("th_high_and_ratio")
    s.simple(0, R.ACCEPTED, d=100, best_dist=100, best_dist2=256, best_level2=-1, n_window=1)              # TH_HIGH, and a lone candidate: no ratio test
    s.simple(1, R.OVER_TH_HIGH, d=101, best_dist=101)
    assert F(F(0.8) * F(50)) == F(40)
    for j, (d1, o1, d2, o2, lv, oc) in ((2, (40, 0, 50, 0, 0, R.ACCEPTED)), (3, (41, 0, 50, 0, 0, R.RATIO_FAILED)),       # 40 > 0.8f * 50 is false in float
                                        (4, (41, 1, 50, 0, 1, R.ACCEPTED)), (7, (30, 0, 30, 0, 0, R.RATIO_FAILED))):     # other octave: no test; a tie is second
        u, v = spot(j); d = new_desc(); p = s.pt(world(u, v), d, lv=lv)
        k1 = s.kp(u, v, o1, at_distance(d, d1)); k2 = s.kp(u + 1, v, o2, at_distance(d, d2, 128))
        s.want(p, oc, best_dist=d1, best_dist2=d2, best_level=o1, best_level2=o2, best_idx=k1, n_window=2, level=lv)
        s.hold(k1, p if oc == R.ACCEPTED else -1); s.hold(k2, -1)
    # ties in distance, other octaves (no ratio test): the first in walk order wins.  Same cell: the lower index
    u, v = spot(5); d = new_desc(); p = s.pt(world(u, v), d, lv=1)
    k1 = s.kp(u + 0.25, v, 0, at_distance(d, 30)); k2 = s.kp(u + 0.75, v, 1, at_distance(d, 30, 128))
    assert R.cell_of(u + 0.25, v, CAM["bounds"]) == R.cell_of(u + 0.75, v, CAM["bounds"])
    s.want(p, R.ACCEPTED, best_idx=k1, best_dist=30, best_dist2=30); s.hold(k1, p); s.hold(k2, -1)
    # different cells: the higher index lies in the earlier column
    u, v = spot(6); d = new_desc(); p = s.pt(world(u, v), d, lv=1)
    k1 = s.kp(u + 1.5, v, 1, at_distance(d, 30)); k2 = s.kp(u - 1.5, v, 0, at_distance(d, 30, 128))
    assert R.cell_of(u - 1.5, v, CAM["bounds"])[0] < R.cell_of(u + 1.5, v, CAM["bounds"])[0]
    s.want(p, R.ACCEPTED, best_idx=k2, best_dist=30, best_dist2=30); s.hold(k1, -1); s.hold(k2, p)
    # and the same layout one row apart instead of one column
    u, v = spot(8); d = new_desc(); p = s.pt(world(u, v), d, lv=1)
    k1 = s.kp(u, v + 3, 1, at_distance(d, 30)); k2 = s.kp(u, v - 3, 0, at_distance(d, 30, 128))
    c1, c2 = R.cell_of(u, v + 3, CAM["bounds"]), R.cell_of(u, v - 3, CAM["bounds"])
    assert c1[0] == c2[0] and c2[1] < c1[1]
    s.want(p, R.ACCEPTED, best_idx=k2); s.hold(k1, -1); s.hold(k2, p)
    return s.done()


def local_second_at_256():
    """ORBmatcher.cc:76-121: bestDist2 starts at 256 and `dist < bestDist2` is strict, so a second candidate AT 256 never becomes second
    best: bestLevel2 stays -1 and no ratio test is made.  nn_ratio 0.3: 80 > 0.3f * 256 would reject."""
    s = Local("second_at_256", nn_ratio=0.3)
    for j, (d1, d2, first256, oc, b2, l2) in enumerate(((80, 256, False, R.ACCEPTED, 256, -1), (80, 255, False, R.RATIO_FAILED, 255, 0),
                                                         (76, 256, False, R.ACCEPTED, 256, -1), (80, 256, True, R.ACCEPTED, 256, -1))):
        u, v = spot(j); d = new_desc(); p = s.pt(world(u, v), d)
        if first256:
            k2 = s.kp(u + 0.5, v, 0, at_distance(d, d2)); k1 = s.kp(u + 1, v, 0, at_distance(d, d1))
        else:
            k1 = s.kp(u + 0.5, v, 0, at_distance(d, d1)); k2 = s.kp(u + 1, v, 0, at_distance(d, d2))
        s.want(p, oc, best_dist=d1, best_dist2=b2, best_level=0, best_level2=l2, n_window=2, n_admitted=2)
        s.hold(k1, p if oc == R.ACCEPTED else -1); s.hold(k2, -1)
    return s.done()


def _lattice(n, cols, step, x0, y0):
    return [(x0 + step * (i % cols), y0 + step * (i // cols)) for i in range(n)]


def local_long_lists(variant):
    """windows of exactly 63, 64 and 65 admitted candidates (th 3: radius 12), the best at the LAST place of the walk and the second at the
    FIRST.  Variant 'accept': best 10 against 25.  Variant 'ratio': best 22 against 25 fails the ratio test -- unless the first place is lost
    (then the second best is a 60 and the point is accepted) or the last (then the 25 is accepted)."""
    s = Local("long_lists_" + variant, th=3.0)
    best = 10 if variant == "accept" else 22
    for u, n in ((96.0, 63), (320.0, 64), (544.0, 65)):
        v = 120.0
        d = new_desc(); p = s.pt(world(u, v), d)
        ks = [s.kp(x, y, 0, at_distance(d, 60, 3 * i)) for i, (x, y) in enumerate(_lattice(n, 9, 2.5, u - 10, v - 8.75))]
        rec = s.keys.record()
        order = R.features_in_area(R.build_grid(rec["kps"], CAM["bounds"]), rec["kps"], CAM["bounds"], u, v, F(12), -1, 0)
        order = [k for k in order if k in set(ks)]
        assert len(order) == n
        s.keys.kd[order[0]] = at_distance(d, 25); s.keys.kd[order[-1]] = at_distance(d, best, 100)
        s.want(p, R.ACCEPTED if variant == "accept" else R.RATIO_FAILED, n_window=n, n_admitted=n, best_dist=best, best_dist2=25, best_idx=order[-1], radius=F(12))
        for k in ks:
            s.hold(k, p if (variant == "accept" and k == order[-1]) else -1)
    return s.done()


def local_group(n):
    """n points in the list (the greedy kernel walks them 16 at a time): every one on its own spot, every third without observations; the
    LAST point stands on the first one's spot and takes its keypoint over -- a dependence across every group boundary in between"""
    s = Local("group_%d" % n)
    first = None
    for j in range(n - 1):
        u, v = spot(j); d = new_desc()
        p = s.pt(world(u, v), d, nObs=0 if j % 3 == 0 else 1)
        k = s.kp(u, v, 0, at_distance(d, j % 7))
        if j == 0:
            first = (p, k, d, u, v)
        else:
            s.want(p, R.ACCEPTED, best_dist=j % 7); s.hold(k, p)
    p0, k0, d0, u0, v0 = first
    p = s.pt(world(u0, v0), d0)
    s.want(p0, R.ACCEPTED_THEN_REPLACED); s.want(p, R.ACCEPTED); s.hold(k0, p)
    assert len(s.points) == n
    return s.done()


def local_empty_list():
    s = Local("empty_list")
    for j in range(5):
        u, v = spot(j); s.hold(s.kp(u, v, 0, new_desc()), -1)
    return s.done()


def local_cut_list():
    """max_points_per_frame = 10 cuts a list of 20: the later ten are never looked at"""
    s = Local("cut_list", max_points=10)
    for j in range(20):
        u, v = spot(j); d = new_desc()
        p = s.pt(world(u, v), d); k = s.kp(u, v, 0, d)
        if j < 10:
            s.want(p, R.ACCEPTED)
        s.hold(k, p if j < 10 else -1)
    return s.done()


def local_skipped():
    s = Local("skipped")
    u, v = spot(0); d = new_desc()
    p = s.pt(world(u, v), d, skip=True); k = s.kp(u, v, 0, d)
    s.want(p, R.SKIPPED); s.hold(k, -1)
    s.simple(1, R.ACCEPTED)
    return s.done()


def local_scenes():
    out = [local_z_sign(), local_image_bounds(), local_dist_range(), local_view_cos(0.5), local_view_cos(0.8), local_radius_cos(1.0), local_radius_cos(3.0)]
    out += [local_predict_scale(k) for k in range(8)]
    out += [local_scale_clamps(), local_window_edge(), local_stereo_check(), local_occupancy(), local_th_high_and_ratio(), local_second_at_256(),
            local_long_lists("accept"), local_long_lists("ratio")]
    out += [local_group(n) for n in (16, 17, 32, 33)]
    out += [local_empty_list(), local_cut_list(), local_skipped()]
    return out


# =================================================================================================================================
# TrackWithMotionModel
# =================================================================================================================================
class Motion:
    def __init__(self, name, th=7.0, th_retry=14.0, retry_below=0, check_orientation=True, th_depth=0.0, points_block=True, use_flags=False,
                 T_cur=None, passes=1):
        self.name = name
        self.kw = dict(th=th, th_retry=th_retry, retry_below=retry_below, check_orientation=check_orientation, th_depth=th_depth, points_block=points_block)
        self.use_flags = use_flags
        self.T_last = I4; self.T_cur = I4 if T_cur is None else T_cur
        self.lastk = _Keys(); self.curk = _Keys(); self.fl = []; self.expect = []; self.holds = []; self.passes = passes

    @property
    def group(self):
        return tuple(sorted(self.kw.items())) + (self.use_flags,)

    def lk(self, x, y, octave, desc, depth=4.0, angle=0.0, flag=3):
        self.fl.append(flag)
        return self.lastk.add(x, y, octave, desc, ur=(F(x) - CAM["bf"] / F(depth)) if depth > 0 else -1.0, angle=angle, depth=depth)

    def ck(self, x, y, octave, desc, ur=-1.0, angle=0.0):
        return self.curk.add(x, y, octave, desc, ur=ur, angle=angle)

    def want(self, i, outcome, **vals):
        self.expect.append((i, outcome, vals))

    def hold(self, k, i):
        self.holds.append((k, i))

    def done(self):
        self.last = self.lastk.record(); self.cur = self.curk.record()
        self.flags = np.array(self.fl, np.uint8) if self.use_flags else None
        return self

    def twin(self, j, outcome, d=0, octave=0, depth=4.0, flag=3, angle_l=0.0, angle_c=0.0, **vals):
        u, v = spot(j); desc = new_desc()
        i = self.lk(u, v, octave, desc, depth=depth, angle=angle_l, flag=flag)
        k = self.ck(u, v, octave, at_distance(desc, d), angle=angle_c)
        self.want(i, outcome, **vals); self.hold(k, i if outcome == R.M_ACCEPTED else -1)
        return i, k


def motion_direction(tz, name, lo, hi, winner):
    """tlc.z = -tz against b = 0.5: AT b neither forward nor backward (octaves o-1 .. o+1), one float beyond forward ([o, inf)) or backward
    ([0, o]).  Keypoints at octaves 2, 3, 4 and 7 with distances 3, 4, 2, 1 under a last keypoint of octave 3: each mode has its own winner."""
    s = Motion("direction_" + name, T_cur=translation(tz))
    d = new_desc()
    i = s.lk(320, 120, 3, d)
    ks = {o: s.ck(320 + j, 120, o, at_distance(d, dd)) for j, (o, dd) in enumerate(((2, 3), (3, 4), (4, 2), (7, 1)))}
    s.want(i, R.M_ACCEPTED, u=F(320), v=F(120), min_level=lo, max_level=hi, radius=F(F(7) * SCALE[3]), best_idx=ks[winner])
    for o, k in ks.items():
        s.hold(k, i if o == winner else -1)
    return s.done()


def motion_gates():
    """identity poses, depth 4: a last keypoint at (x, y) projects to (x, y) exactly; radius 7 at octave 0"""
    s = Motion("gates")
    s.twin(0, R.NO_DEPTH, depth=-1.0); s.twin(1, R.NO_DEPTH, depth=0.0)
    for (x_in, y_in), (x_out, y_out), wit in (((640, 120), (nxt(640), 120), (634, 120)), ((0, 120), (F(-2.0 ** -15), 120), (6, 120)),
                                              ((320, 240), (320, nxt(240)), (320, 236)), ((320, 0), (320, F(-2.0 ** -17)), (320, 4))):
        di, do = new_desc(), new_desc()
        a = s.lk(x_in, y_in, 0, di); b = s.lk(x_out, y_out, 0, do)
        ka = s.ck(wit[0], wit[1], 0, di); kb = s.ck(wit[0], wit[1], 0, do)
        s.want(a, R.M_ACCEPTED, u=F(x_in), v=F(y_in), radius=F(7), n_window=2); s.want(b, R.M_OUT_OF_IMAGE, u=F(x_out), v=F(y_out))
        s.hold(ka, a); s.hold(kb, -1)
    # stereo consistency: ur = x - 32
    for j, (ur_of, ok) in enumerate(((lambda u: F(u - 32 + 7), True), (lambda u: nxt(F(u - 32 + 7)), False), (lambda u: F(u - 32 - 7), True),
                                     (lambda u: nxt(F(u - 32 - 7), DOWN), False), (lambda u: F(0.0), True), (lambda u: F(-1.0), True))):
        u, v = spot(12 + j); d = new_desc()
        i = s.lk(u, v, 0, d); k = s.ck(u, v, 0, d, ur=ur_of(u))
        s.want(i, R.M_ACCEPTED if ok else R.ALL_REFUSED, ur=F(u - 32), n_window=1, n_admitted=1 if ok else 0); s.hold(k, i if ok else -1)
    s.twin(24, R.M_ACCEPTED, d=100, best_dist=100); s.twin(25, R.M_OVER_TH_HIGH, d=101, best_dist=101)
    # first-minimum ties: same cell (the lower index), different cells (the higher index in the earlier column)
    u, v = spot(26); d = new_desc(); i = s.lk(u, v, 0, d)
    k1 = s.ck(u + 0.25, v, 0, at_distance(d, 30)); k2 = s.ck(u + 0.75, v, 0, at_distance(d, 30, 128))
    assert R.cell_of(u + 0.25, v, CAM["bounds"]) == R.cell_of(u + 0.75, v, CAM["bounds"])
    s.want(i, R.M_ACCEPTED, best_idx=k1, best_dist=30, n_window=2); s.hold(k1, i); s.hold(k2, -1)
    u, v = spot(30); d = new_desc(); i = s.lk(u, v, 0, d)
    k1 = s.ck(u + 1.5, v, 0, at_distance(d, 30)); k2 = s.ck(u - 1.5, v, 0, at_distance(d, 30, 128))
    assert R.cell_of(u - 1.5, v, CAM["bounds"])[0] < R.cell_of(u + 1.5, v, CAM["bounds"])[0]
    s.want(i, R.M_ACCEPTED, best_idx=k2, best_dist=30, n_window=2); s.hold(k1, -1); s.hold(k2, i)
    # nothing near
    u, v = spot(28); i = s.lk(u, v, 0, new_desc()); s.want(i, R.M_EMPTY_WINDOW, n_window=0)
    return s.done()


def motion_behind():
    """the camera moved 8 forward: a point at depth 4 is behind it (invzc < 0), one at depth 16 projects with zc = 8"""
    s = Motion("behind", T_cur=translation(-8.0))
    da, db = new_desc(), new_desc()
    a = s.lk(320, 120, 0, da, depth=4.0); b = s.lk(352, 120, 0, db, depth=16.0)
    ka = s.ck(320, 120, 0, da); kb = s.ck(384, 120, 0, db)
    s.want(a, R.M_BEHIND, zc=F(-4)); s.want(b, R.M_ACCEPTED, zc=F(8), u=F(384), v=F(120), min_level=0, max_level=-1)
    s.hold(ka, -1); s.hold(kb, b)
    return s.done()


def motion_flags():
    """explicit point flags (bit 0: a point, bit 1: it has observations and blocks) and a keypoint claimed twice.  22 matches in rotation
    bin 0, two in bin 6 (angle difference 180): bin 6 is under a tenth of bin 0 and is removed (ORBmatcher.cc:1500-1510 sets the KEYPOINT to
    NULL, whoever holds it by then, and takes one off nmatches per entry)."""
    s = Motion("flags", use_flags=True)
    s.twin(0, R.FLAG_OFF, flag=0); s.twin(1, R.FLAG_OFF, flag=2)
    for j in range(20):
        s.twin(2 + j, R.M_ACCEPTED, flag=3 if j % 2 else 1, bin=0)
    # first claim (no observations) in the removed bin, second claim kept: the keypoint ends empty
    u, v = spot(24); d = new_desc()
    q1 = s.lk(u, v, 0, d, angle=180.0, flag=1); q2 = s.lk(u, v, 0, d, flag=3); k = s.ck(u, v, 0, d)
    s.want(q1, R.ROT_REMOVED, bin=6, best_idx=k); s.want(q2, R.M_ACCEPTED, bin=0, best_idx=k, kept=False); s.hold(k, -1)
    # the reverse: first claim kept, second removed
    u, v = spot(25); d = new_desc()
    q3 = s.lk(u, v, 0, d, flag=1); q4 = s.lk(u, v, 0, d, angle=180.0, flag=3); k = s.ck(u, v, 0, d)
    s.want(q3, R.M_ACCEPTED_THEN_REPLACED, bin=0, best_idx=k, kept=False); s.want(q4, R.ROT_REMOVED, bin=6, best_idx=k); s.hold(k, -1)
    # a blocking first claim: the second query skips the keypoint and takes the next best
    u, v = spot(26); d = new_desc()
    q5 = s.lk(u, v, 0, d, flag=3); q6 = s.lk(u, v, 0, d, flag=3); k1 = s.ck(u, v, 0, d); k2 = s.ck(u + 1, v, 0, at_distance(d, 20))
    s.want(q5, R.M_ACCEPTED, best_idx=k1); s.want(q6, R.M_ACCEPTED, best_idx=k2, n_window=2, n_admitted=1, best_dist=20); s.hold(k1, q5); s.hold(k2, q6)
    # a non-blocking first claim: the second query takes the same keypoint
    u, v = spot(27); d = new_desc()
    q7 = s.lk(u, v, 0, d, flag=1); q8 = s.lk(u, v, 0, d, flag=3); k1 = s.ck(u, v, 0, d); k2 = s.ck(u + 1, v, 0, at_distance(d, 20))
    s.want(q7, R.M_ACCEPTED_THEN_REPLACED, best_idx=k1); s.want(q8, R.M_ACCEPTED, best_idx=k1, n_admitted=2, kept=True); s.hold(k1, q8); s.hold(k2, -1)
    return s.done()


TH_DEPTH = 8.0


def motion_close_rule(n_close):
    """UpdateLastFrame: n_close points with z <= mThDepth (three of them AT it) and six beyond it at depths 10, 10, 12, 12, 14, 16, indices
    shuffled.  Sorted by (depth, index) the walk takes max(100, n_close) + 1 points; the two at depth 10 show the index tie-break when only
    one of them is taken.  Every last keypoint has one twin in the current frame."""
    s = Motion("close_rule_%d" % n_close, th=2.0, th_retry=4.0, th_depth=TH_DEPTH)
    depths = [1.0 + j / 16.0 for j in range(n_close - 3)] + [TH_DEPTH] * 3
    far = [10.0, 10.0, 12.0, 12.0, 14.0, 16.0]
    zs = depths + far
    perm = np.random.default_rng(n_close).permutation(len(zs))
    zs = [zs[j] for j in perm]
    n_taken_far = max(0, max(100, n_close) + 1 - n_close) if n_close + len(far) > 100 else len(far)
    far_sorted = sorted((z, i) for i, z in enumerate(zs) if z > TH_DEPTH)
    taken_far = set(i for _, i in far_sorted[:n_taken_far])
    for i, z in enumerate(zs):
        u, v = 30.0 + 38.0 * (i % 16), 20.0 + 28.0 * (i // 16)
        d = new_desc()
        q = s.lk(u, v, 0, d, depth=z); k = s.ck(u, v, 0, d)
        taken = z <= TH_DEPTH or i in taken_far
        s.want(q, R.M_ACCEPTED if taken else R.BEYOND_CLOSE_RULE); s.hold(k, q if taken else -1)
    s.n_taken = len([z for z in zs if z <= TH_DEPTH]) + len(taken_far)
    return s.done()


def motion_counts():
    """windows of exactly 16 and 17 candidates (a row of the speculative pass against a query walked alone) and of 63, 64 and 65 (the list, its
    cap, the re-walk), the best at the LAST place of the walk"""
    s = Motion("counts")
    for u, n in ((64.0, 16), (192.0, 17), (320.0, 63), (448.0, 64), (576.0, 65)):
        v = 120.0; d = new_desc()
        i = s.lk(u, v, 0, d)
        ks = [s.ck(x, y, 0, at_distance(d, 60, 3 * j)) for j, (x, y) in enumerate(_lattice(n, 9, 1.5, u - 6, v - 5.25))]
        rec = s.curk.record()
        order = [k for k in R.features_in_area(R.build_grid(rec["kps"], CAM["bounds"]), rec["kps"], CAM["bounds"], u, v, F(7), -1, 1) if k in set(ks)]
        assert len(order) == n
        s.curk.kd[order[-1]] = at_distance(d, 10, 100); s.curk.kd[order[0]] = at_distance(d, 11, 50)
        s.want(i, R.M_ACCEPTED, n_window=n, n_admitted=n, best_dist=10, best_idx=order[-1])
        for k in ks:
            s.hold(k, i if k == order[-1] else -1)
    return s.done()


def motion_retry(n_first):
    """th 3, th_retry 9, retry_below 5.  Every last keypoint has a twin 1 px away at distance 50 and a better one 6 px away that only the
    retry reaches; one more last keypoint has nothing but the far twin.  Four first-pass matches: the retry runs from a cleared frame, the
    near twins end empty.  Five: no retry, the far twins stay empty."""
    s = Motion("retry_%d" % n_first, th=3.0, th_retry=9.0, retry_below=5, passes=2 if n_first < 5 else 1)
    retried = n_first < 5
    for j in range(n_first):
        u, v = spot(j); d = new_desc()
        i = s.lk(u, v, 0, d); near = s.ck(u + 1, v, 0, at_distance(d, 50)); far = s.ck(u + 6, v, 0, at_distance(d, 10, 100))
        s.want(i, R.M_ACCEPTED, best_idx=far if retried else near, radius=F(9 if retried else 3), n_window=2 if retried else 1)
        s.hold(near, -1 if retried else i); s.hold(far, i if retried else -1)
    u, v = spot(12); d = new_desc()
    i = s.lk(u, v, 0, d); far = s.ck(u + 6, v, 0, d)
    s.want(i, R.M_ACCEPTED if retried else R.M_EMPTY_WINDOW); s.hold(far, i if retried else -1)
    return s.done()


ROTATIONS = [(0.0, 0.0, 0)] * 10 + [(15.0, 0.0, 1), (14.999, 0.0, 0), (10.0, 20.0, 12), (5.0, 15.0, 12), (345.0, 0.0, 12), (890.0, 0.0, 0), (44.9, 0.0, 1),
                                    (45.0, 0.0, 2), (100.0, 0.0, 3)]


def motion_rotation():
    """angle differences on bin edges (rot * (1.0f / 30), roundf): 15 -> bin 1, 14.999 -> 0, 45 -> 2, 44.9 -> 1, 345 -> 12; a negative rot
    (10 - 20 + 360 = 350 -> 12).  With angles in [0, 360) rot / 30 stays below 12.5, so the reference's `bin == HISTO_LENGTH` wrap cannot
    happen; an out-of-range last angle of 890 (bin 30 -> 0) runs that statement all the same.  Bins: 0 holds 12, 12 holds 3, 1 holds 2;
    bins 2 and 3 hold one match each and are removed."""
    s = Motion("rotation")
    for j, (al, ac, b) in enumerate(ROTATIONS):
        s.twin(j, R.M_ACCEPTED if b in (0, 12, 1) else R.ROT_REMOVED, angle_l=al, angle_c=ac, bin=b, negative_rot=al < ac, wrapped=al > 360)
    return s.done()


def motion_scenes():
    b = F(0.5)
    return [motion_direction(-b, "at_b", 2, 4, 4), motion_direction(nxt(-b, DOWN), "forward", 3, -1, 7),
            motion_direction(b, "at_minus_b", 2, 4, 4), motion_direction(nxt(b, UP), "backward", 0, 3, 2),
            motion_gates(), motion_behind(), motion_flags(), motion_close_rule(99), motion_close_rule(100), motion_close_rule(101), motion_close_rule(30),
            motion_counts(), motion_retry(4), motion_retry(5), motion_rotation()]


# =================================================================================================================================
# the three sides of a scene: the restatement, the oracle (projection_oracle around the C oracle), and their comparison
# =================================================================================================================================
def frame_dict(rec, T):
    return dict(kps=rec["kps"], desc=rec["desc"], uright=rec["uright"], depth=rec["depth"], T=T, scale=SCALE, fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"],
                cy=CAM["cy"], mbf=CAM["bf"], mb=CAM["b"], bounds=CAM["bounds"])


def local_points(sc):
    return sc.points if sc.max_points is None else sc.points[:sc.max_points]


def ref_local(sc):
    return R.search_local(CAM, sc.rec, sc.T, local_points(sc), sc.occupied, sc.th, sc.nn_ratio, sc.cos_limit)


def oracle_local(O, PO, sc):
    cur = frame_dict(sc.rec, sc.T); cur["logScale"] = F(O.lib.orc_logf(float(SCALE[1])))
    return PO.search_local_points_frame(O, cur, local_points(sc), sc.occupied, F(sc.th), F(sc.nn_ratio), sc.cos_limit)


def ref_motion(sc):
    k = sc.kw
    return R.track_motion(CAM, sc.last, sc.cur, sc.T_last, sc.T_cur, k["th"], k["th_retry"], k["retry_below"], k["check_orientation"], k["th_depth"],
                          k["points_block"], sc.flags)


def oracle_motion(O, PO, sc, quality=None):
    k = sc.kw
    return PO.track_with_motion_model_matches(O, frame_dict(sc.cur, sc.T_cur), frame_dict(sc.last, sc.T_last), F(k["th"]), F(k["th_retry"]), k["retry_below"],
                                              k["check_orientation"], k["th_depth"], k["points_block"], sc.flags, quality=quality)


def describe(names, outcome, infos, q):
    """what a failure message says about query q"""
    keys = ("u", "v", "level", "radius", "n_window", "n_admitted", "best_dist", "best_dist2", "best_idx")
    return "query %d: %s (%s)" % (q, names[outcome[q]], ", ".join("%s %s" % (k, infos[q][k]) for k in keys if k in infos[q]))


def explain(names, got, exp, outcome, infos):
    """the keypoints on which two assignments differ, with the outcome of every query involved"""
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    lines = []
    for k in bad[:6]:
        qs = sorted(set(int(q) for q in (got[k], exp[k]) if 0 <= q < len(outcome)))
        lines.append("keypoint %d holds %d, expected %d; %s" % (k, got[k], exp[k], "; ".join(describe(names, outcome, infos, q) for q in qs)))
    return "\n".join(lines)
