"""mapping_scenes.py -- hand-made scenes for the per-call mapping and loop-closing searches (SearchByProjection(KF, Scw), both Fuse,
SearchBySim3, SearchForInitialization, SearchByBoW(KF, KF), SearchForTriangulation): keypoints and queries ON every comparison of the reference's
loops and one step beside it -- the next integer for a descriptor distance, the neighbouring float32 for a float.  A 640 x 480 image
(10 x 10 px grid cells) is cut into 4 x 4 tiles of 160 x 120; every scene of a window search lives in tiles of its own, at absolute
coordinates, so the scenes of one search also run concatenated into one call.  The BoW-driven searches have no windows: their scenes are
kept apart by node ids.

Every scene carries `expect` = (item, outcome code, intermediates by value) and `holds` = what every output slot must contain.
tests/test_mapping_scenes_cpu.py checks both against the restatement tests/mapping_ref.py and the C oracle; tests/test_gpu_mapping_scenes.py
runs the device on the same scenes.

Gates no scene stands on, and why:
  * mono chi-square `e2*invSigma2 > 5.99` made in float instead of double: float(5.99) lies BELOW the double 5.99, so `x > 5.99` and
    `x > 5.99f` agree for every float x.  The scenes stand on both sides of 5.99 (the float below and the float above); the float-for-double
    fault is shown at 7.8, whose float lies above the double.
  * `nMinCellX >= mnGridCols` / `nMaxCellX < 0` (a window wholly off the grid): the contract hands over projections that passed IsInImage, and
    a radius is positive, so no query reaches them; the windows here leave the grid on each side and are clamped.
  * rot == 360 -> bin 30 -> 0: angles lie in [0, 360), see the rotation cases of tests/test_gpu_parity.py, which stay as they are."""
import numpy as np

import mapping_ref as R
from projection_ref import scale_table
from projection_scenes import nxt, at_distance, KP_DTYPE, UP, DOWN

F = np.float32
BOUNDS = (0.0, 0.0, 640.0, 480.0)
SCALE = scale_table()
SIGMA2 = (SCALE * SCALE).astype(F)                          # mvLevelSigma2 (ORBextractor.cc:427-433)
INV_SIGMA2 = (F(1.0) / SIGMA2).astype(F)                    # mvInvLevelSigma2
LOOSE = np.full(8, 2.0 ** -12, F)                           # a gate no keypoint of a window scene fails
_rng = np.random.default_rng(77001)
QKEYS = ("u", "v", "ur", "radius", "level", "desc", "valid")
QTYPES = dict(u=F, v=F, ur=F, radius=F, level=np.int32, desc=np.uint8, valid=np.uint8)


def new_desc():
    """random descriptors lie about 128 bits apart, far beyond TH_HIGH"""
    return _rng.integers(0, 256, 32).astype(np.uint8)


def tile(tx, ty):
    return 160.0 * tx, 120.0 * ty


def ulps(x, n):
    """the 2n+1 float32 around x > 0"""
    return (np.array(x, F).reshape(1).view(np.int32) + np.arange(-n, n + 1, dtype=np.int32)).view(F)


def hit(fn, target, xs, ys):
    """the first (x, y) of xs x ys with fn(x, y) == target exactly; fn works on float32 arrays, one rounding per operation"""
    X, Y = np.meshgrid(np.asarray(xs, F), np.asarray(ys, F), indexing="ij")
    k = np.argwhere(fn(X, Y) == F(target))
    if not len(k):
        return None
    return F(X[tuple(k[0])]), F(Y[tuple(k[0])])


class Keys:
    def __init__(self):
        self.rows = []

    def add(self, x, y, octave, desc, ur=-1.0, angle=0.0):
        self.rows.append((F(x), F(y), int(octave), np.array(desc, np.uint8), F(ur), F(angle)))
        return len(self.rows) - 1

    def record(self):
        n = len(self.rows)
        kps = np.zeros(n, KP_DTYPE)
        for f, j in (("x", 0), ("y", 1), ("octave", 2), ("angle", 5)):
            kps[f] = [r[j] for r in self.rows]
        kps["size"] = 31; kps["response"] = 20
        return dict(kps=kps, desc=np.array([r[3] for r in self.rows], np.uint8).reshape(n, 32), uright=np.array([r[4] for r in self.rows], F))


def _queries(rows):
    n = len(rows)
    q = {k: np.array([r[k] for r in rows], QTYPES[k]) for k in QKEYS if k != "desc"}
    q["desc"] = np.array([r["desc"] for r in rows], np.uint8).reshape(n, 32)
    return q


NO_QUERY = dict(u=0.0, v=0.0, ur=0.0, radius=1.0, level=0, desc=np.zeros(32, np.uint8), valid=0)


class Scene:
    """search: keyframe | fuse | fuse_scw | sim3 | init | bow | triangulation.  k2 = the frame the windows run on / KF2 / F2; k1 = KF1 / F1."""

    def __init__(self, name, search, **params):
        self.name, self.search, self.params = name, search, params
        self.k1, self.k2 = Keys(), Keys()
        self.q, self.q21, self.pre = [], {}, {}
        self.has1, self.has2, self.st1, self.st2, self.prev = [], [], [], [], []
        self.fv1, self.fv2 = {}, {}
        self.expect, self.holds = [], {}

    @property
    def group(self):
        return (self.search,) + tuple((k, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else v) for k, v in sorted(self.params.items()))

    def kp(self, x, y, octave, desc, ur=-1.0, angle=0.0):
        return self.k2.add(x, y, octave, desc, ur, angle)

    def want(self, item, outcome, **vals):
        self.expect.append((item, outcome, vals))

    def hold(self, slot, value):
        assert slot not in self.holds
        self.holds[slot] = value

    # -- window searches: one projected map point
    def query(self, u, v, radius, level, desc, best, outcome, ur=0.0, valid=1, beside=-1, **vals):
        """best = the keypoint of k2 the query must end on (-1: none).  What that means for the output is the search's: vpMatched[best] = the
        query (keyframe), best_idx[query] = best (fuse), vnMatch1[slot] = best and a reverse query that agrees (sim3).  beside = a keypoint the
        query just misses: sim3 gives it a reverse query too, so that a forward search that did reach it would show in the result."""
        i = len(self.q)
        self.q.append(dict(u=F(u), v=F(v), ur=F(ur), radius=F(radius), level=int(level), desc=np.array(desc, np.uint8), valid=int(valid)))
        self.want(i, outcome, **vals)
        if self.search == "keyframe":
            if best >= 0:
                self.hold(best, i)
        elif self.search == "sim3":
            p1 = (min(float(u), 630.0), min(float(v), 470.0))            # slot i of KF1: near where its point projects (and inside KF1's grid),
            self.k1.add(p1[0], p1[1], 0, desc)                           # with the point's descriptor, so that the reverse query agrees
            self.hold(i, best)
            if max(best, beside) >= 0:
                self.q21[max(best, beside)] = dict(u=F(p1[0]), v=F(p1[1]), ur=F(0), radius=F(3), level=0, desc=np.array(desc, np.uint8), valid=1)
        else:
            self.hold(i, best)
        return i

    # -- BoW-driven searches: one feature on either side
    def f1(self, node, desc, has=None, stereo=0, x=0.0, y=0.0, octave=0, angle=0.0):
        i = self.k1.add(x, y, octave, desc, angle=angle)
        self.has1.append(int((self.search == "bow") if has is None else has)); self.st1.append(int(stereo))
        if node is not None:
            self.fv1.setdefault(node, []).append(i)
        return i

    def f2(self, node, desc, has=None, stereo=0, x=0.0, y=0.0, octave=0, angle=0.0):
        i = self.k2.add(x, y, octave, desc, angle=angle)
        self.has2.append(int((self.search == "bow") if has is None else has)); self.st2.append(int(stereo))
        if node is not None:
            self.fv2.setdefault(node, []).append(i)
        return i

    def done(self):
        self.rec1, self.rec2 = self.k1.record(), self.k2.record()
        n1, n2 = len(self.rec1["kps"]), len(self.rec2["kps"])
        assert n1 <= 256 and n2 <= 256
        if self.search in ("keyframe", "fuse", "fuse_scw", "sim3"):
            self.Q = _queries(self.q)
        if self.search == "keyframe":
            self.matched = np.full(n2, -1, np.int32)
            for k, v in self.pre.items():
                self.matched[k] = v
            for k in range(n2):
                self.holds.setdefault(k, int(self.matched[k]))
        if self.search == "sim3":
            self.Q21 = _queries([self.q21.get(k, NO_QUERY) for k in range(n2)])
        if self.search == "init":
            self.prev_xy = np.array(self.prev, F).reshape(-1, 2)
        if self.search in ("bow", "triangulation", "init"):
            for k in range(n1):
                self.holds.setdefault(k, -1)
        for a in ("has1", "has2", "st1", "st2"):
            setattr(self, a, np.array(getattr(self, a), np.uint8))
        return self


# =================================================================================================================================
# windows: the scenes every window search runs (KeyFrame::GetFeaturesInArea and the level test)
# =================================================================================================================================
def w_strict_radius(s):
    """|dx| < r, |dy| < r are strict (KeyFrame.cc:638): a keypoint exactly r = 8 from the centre is out, the float before it is in"""
    ox, oy = tile(1, 1)
    for j, (sx, sy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        for k, inside in enumerate((False, True)):
            u, v = ox + 20 + 40 * j, oy + 30 + 60 * k
            x, y = F(u + 8 * sx), F(v + 8 * sy)
            if inside:
                x, y = nxt(x, F(u)) if sx else x, nxt(y, F(v)) if sy else y
            d = new_desc()
            kp = s.kp(x, y, 0, at_distance(d, 10))
            if inside:
                s.query(u, v, 8, 0, d, kp, R.ACCEPTED, n_window=1, best_dist=10, best_idx=kp)
            else:
                s.query(u, v, 8, 0, d, -1, R.EMPTY_WINDOW, beside=kp, n_window=0)


def w_off_grid(s):
    """windows that leave the grid on each side (clamped, :611-625), and keypoints PosInGrid leaves out of the grid: posX = round(x / 10) = 64
    for x >= 635, posY = 48 for y >= 475 -- inside the window and nearest by descriptor, but in no cell"""
    for (u, v), (kx, ky), lost in (((3, 60), (1, 62), None), ((80, 3), (83, 1), None), ((637, 420), (634, 421), (636, 419)), ((500, 477), (502, 474), (499, 476))):
        d = new_desc()
        kp = s.kp(kx, ky, 0, at_distance(d, 20))
        if lost:
            s.kp(lost[0], lost[1], 0, d)
        s.query(u, v, 8, 0, d, kp, R.ACCEPTED, n_window=1, best_dist=20, best_idx=kp)


def w_cell_straddle(s):
    """a window over four cells (a cell is round(x / 10): x = 365 is a boundary).  Window order = ix outer, iy inner: of two keypoints at the
    same distance the one in the lower ix wins although its index is the higher"""
    ox, oy = tile(2, 1)
    u, v = ox + 45, oy + 45
    d = new_desc()
    a = s.kp(u + 3, v - 3, 0, at_distance(d, 12))            # cell (ix + 1, iy)
    b = s.kp(u + 3, v + 3, 0, at_distance(d, 30))            # cell (ix + 1, iy + 1)
    c = s.kp(u - 3, v + 3, 0, at_distance(d, 12, 100))       # cell (ix, iy + 1): same distance as a, earlier in the walk
    e = s.kp(u - 3, v - 3, 0, at_distance(d, 40))            # cell (ix, iy)
    s.query(u, v, 6, 0, d, c, R.ACCEPTED, n_window=4, best_dist=12, best_idx=c)


def w_octaves(s):
    """the level test [level - 1, level] with octaves level - 2 .. level + 1 in the window, the smallest distances outside"""
    ox, oy = tile(1, 2)
    u, v = ox + 40, oy + 40
    d = new_desc()
    k = {o: s.kp(u + o - 2, v + 1, o, at_distance(d, dist)) for o, dist in ((1, 1), (2, 6), (3, 4), (4, 2))}
    s.query(u, v, 7, 3, d, k[3], R.ACCEPTED, n_window=4, n_level=2, best_dist=4, best_idx=k[3])
    u, v = ox + 100, oy + 40
    d = new_desc()
    s.kp(u + 1, v, 1, d); s.kp(u - 1, v, 4, d)
    s.query(u, v, 7, 3, d, -1, R.SKIPPED_LEVEL, n_window=2, n_level=0)
    u, v = ox + 40, oy + 90
    d = new_desc()
    s.kp(u + 1, v, 1, d); k0 = s.kp(u - 1, v, 0, at_distance(d, 9))
    s.query(u, v, 5, 0, d, k0, R.ACCEPTED, n_window=2, n_level=1, best_dist=9)


def w_many(s, n):
    """n candidates in one window: the resident frame's device list holds 128, the 129th sends the query through the host grid"""
    ox, oy = tile(0, 1 if n == 128 else 2)
    u, v = ox + 80.5, oy + 60.5
    d = new_desc()
    best = -1
    for j in range(n):
        far = new_desc()
        k = s.kp(ox + 73 + (j % 16), oy + 55 + (j // 16), 0, at_distance(d, 20) if j == n - 3 else far)
        if j == n - 3:
            best = k
    s.query(u, v, 12, 0, d, best, R.ACCEPTED, n_window=n, n_level=n, best_dist=20, best_idx=best)


WINDOWS = (("strict_radius", w_strict_radius), ("off_grid", w_off_grid), ("cell_straddle", w_cell_straddle), ("octaves", w_octaves),
           ("window_128", lambda s: w_many(s, 128)), ("window_129", lambda s: w_many(s, 129)))


def window_scenes(search, **params):
    out = []
    for name, build in WINDOWS:
        s = Scene(name, search, **params)
        build(s)
        out.append(s.done())
    return out


def _invalid(s, ox, oy):
    d = new_desc()
    s.kp(ox + 20, oy + 100, 0, d)
    s.query(ox + 20, oy + 100, 5, 0, d, -1, R.INVALID, valid=0)


# =================================================================================================================================
# SearchByProjection(KeyFrame*, Scw, ...)
# =================================================================================================================================
def keyframe_gates():
    s = Scene("occupancy_and_th", "keyframe")
    ox, oy = tile(2, 2)
    # vpMatched[idx] occupied on entry (-2): skipped although it is the nearest
    u, v = ox + 20, oy + 20; d = new_desc()
    a = s.kp(u + 1, v, 0, at_distance(d, 5)); b = s.kp(u - 1, v, 0, at_distance(d, 20))
    s.pre[a] = -2
    s.query(u, v, 5, 0, d, b, R.ACCEPTED, n_window=2, n_compared=1, best_dist=20)
    # a keypoint an EARLIER query took (>= 0) is skipped by a later one
    u, v = ox + 60, oy + 20; d = new_desc()
    a = s.kp(u + 1, v, 0, at_distance(d, 10)); b = s.kp(u - 1, v, 0, at_distance(d, 30))
    s.query(u, v, 5, 0, d, a, R.ACCEPTED, n_compared=2, best_dist=10)
    s.query(u, v, 5, 0, at_distance(d, 7, 50), b, R.ACCEPTED, n_compared=1, best_dist=37)
    # only occupied candidates: one on entry, one taken in this call
    u, v = ox + 100, oy + 20; d = new_desc()
    a = s.kp(u + 1, v, 0, d); b = s.kp(u - 1, v, 0, d)
    s.pre[a] = -2
    s.query(u, v, 5, 0, d, b, R.ACCEPTED, n_compared=1)
    s.query(u, v, 5, 0, d, -1, R.OCCUPIED, n_window=2, n_compared=0)
    # bestDist <= TH_LOW (:400)
    for j, dist in enumerate((50, 51)):
        u, v = ox + 20 + 40 * j, oy + 60; d = new_desc()
        a = s.kp(u, v + 1, 0, at_distance(d, dist))
        s.query(u, v, 5, 0, d, a if dist == 50 else -1, R.ACCEPTED if dist == 50 else R.OVER_TH, best_dist=dist)
    # equal distances: `dist<bestDist` keeps the first in window order (same cell: insertion order)
    u, v = ox + 100, oy + 61; d = new_desc()
    a = s.kp(u + 1, v, 0, at_distance(d, 15)); b = s.kp(u + 1, v + 1, 0, at_distance(d, 15, 64))
    s.query(u, v, 5, 0, d, a, R.ACCEPTED, n_compared=2, best_dist=15, best_idx=a)
    _invalid(s, ox, oy)
    return s.done()


def keyframe_scenes():
    return window_scenes("keyframe") + [keyframe_gates()]


# =================================================================================================================================
# Fuse
# =================================================================================================================================
def chi2_v(u, v, ur, kx, ky, kur, inv, stereo):
    """e2 * invSigma2 as :926-942 says it, on float32 arrays"""
    ex = F(u) - kx; ey = F(v) - ky
    e2 = ex * ex + ey * ey
    if stereo:
        er = F(ur) - kur
        e2 = e2 + er * er
    return e2 * F(inv)


def _reachable(target, inv):
    """is there a float32 e2 with float(e2 * inv) == target?  Above octave 0 the products lie further apart than the floats around 7.8"""
    return bool((ulps(float(target) / float(inv), 8) * F(inv) == F(target)).any())


def fuse_chi2(search):
    """e2 * mvInvLevelSigma2[kpLevel] against the DOUBLES 7.8 (stereo) and 5.99 (mono) at octaves 0 and 1.  float(7.8) lies above the double:
    a product of exactly float(7.8) is refused, the float below passes.  float(5.99) lies below the double: it passes, the float above is refused.
    The second octave is the first one at which float32 products reach both floats beside the limit (invSigma2 < 1 spreads the products wider
    than the floats lie).  The Scw variant runs the same scene with no gate: every one of these is fused."""
    gate = search == "fuse"
    s = Scene("chi_square", search, inv_sigma2=INV_SIGMA2 if gate else None)
    ox, oy = tile(2, 2)
    j = 0
    for stereo, limit in ((True, 7.8), (False, 5.99)):
        above = F(limit) if float(F(limit)) > limit else nxt(F(limit), UP)
        below = nxt(above, DOWN)
        assert float(below) <= limit < float(above)
        second = [o for o in range(1, 8) if _reachable(above, INV_SIGMA2[o]) and _reachable(below, INV_SIGMA2[o])][0]
        for lv in (0, second):
            for target in (above, below):
                u, v = ox + 16 + 32 * (j % 4), oy + 16 + 32 * (j // 4); ur = u - 32.0; j += 1
                e = float(target) / float(INV_SIGMA2[lv])
                got = None
                for ex0 in (2.0 - k / 16.0 for k in range(24)):                    # ex about ex0; stereo: ey = -1, er fills up e2; mono: ey does
                    if stereo:
                        fn = lambda kx, kur: chi2_v(u, v, ur, kx, F(v + 1), kur, INV_SIGMA2[lv], True)
                        got = hit(fn, target, ulps(u - ex0, 200), ulps(ur - np.sqrt(e - ex0 * ex0 - 1), 300))
                    else:
                        fn = lambda kx, ky: chi2_v(u, v, ur, kx, ky, None, INV_SIGMA2[lv], False)
                        got = hit(fn, target, ulps(u - ex0, 200), ulps(v - np.sqrt(e - ex0 * ex0), 300))
                    if got is not None:
                        break
                assert got is not None, "no float32 keypoint at chi2 == %r" % target
                kx, ky, kur = (got[0], F(v + 1), got[1]) if stereo else (got[0], got[1], F(-1))
                d = new_desc()
                kp = s.kp(kx, ky, lv, at_distance(d, 8), ur=kur)
                ok = not gate or target == below
                vals = dict(chi2=target, stereo=stereo) if gate else {}
                s.query(u, v, F(4) * SCALE[lv], lv, d, kp if ok else -1, R.ACCEPTED if ok else R.CHI2_FAILED, ur=ur, n_window=1, n_level=1,
                        best_dist=8 if ok else 256, **vals)
    # mvuRight[idx] >= 0 (:920): exactly 0 is stereo -- ex^2 + ey^2 = 1 would pass as mono, with er = 3 the stereo e2 = 10 does not
    u, v = ox + 16, oy + 80; d = new_desc()
    kp = s.kp(u - 1, v, 0, at_distance(d, 8), ur=0.0)
    s.query(u, v, 4, 0, d, -1 if gate else kp, R.CHI2_FAILED if gate else R.ACCEPTED, ur=3.0, **(dict(e2=F(10), stereo=True) if gate else {}))
    # bestDist <= TH_LOW (:958, :1088); best_dist is reported also when nothing passes
    for k, dist in enumerate((50, 51)):
        u, v = ox + 48 + 32 * k, oy + 80; d = new_desc()
        kp = s.kp(u, v, 0, at_distance(d, dist))
        s.query(u, v, 4, 0, d, kp if dist == 50 else -1, R.ACCEPTED if dist == 50 else R.OVER_TH, ur=u - 32.0, best_dist=dist)
    # a level whose invSigma2 decides: the same error passes at octave 1 and fails at octave 0
    for k, lv in enumerate((0, 1)):
        u, v = ox + 16 + 32 * k, oy + 104; d = new_desc()
        kp = s.kp(u - 2.5, v, lv, at_distance(d, 8))                                   # e2 = 6.25: > 5.99 at octave 0, 4.34 at octave 1
        ok = not gate or lv == 1
        s.query(u, v, F(4) * SCALE[lv], lv, d, kp if ok else -1, R.ACCEPTED if ok else R.CHI2_FAILED, ur=u - 32.0, **(dict(e2=F(6.25)) if gate else {}))
    _invalid(s, ox + 100, oy)
    return s.done()


def fuse_scenes(search):
    p = dict(inv_sigma2=LOOSE if search == "fuse" else None)
    return window_scenes(search, **p) + [fuse_chi2(search)]


# =================================================================================================================================
# SearchBySim3
# =================================================================================================================================
def sim3_gates():
    s = Scene("agreement_and_th", "sim3")
    ox, oy = tile(2, 2)

    def pair(j, d12, d21, v12=1, v21=1):
        """slot a of KF1 and keypoint b of KF2 at spot j; a's point is d12 bits from b's descriptor, b's point d21 bits from a's"""
        u, v = ox + 12 + 24 * (j % 6), oy + 12 + 24 * (j // 6)
        da, db = new_desc(), new_desc()
        a = s.k1.add(u, v, 0, da); b = s.kp(u, v, 0, db)
        s.q.append(dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=at_distance(db, d12), valid=v12))
        s.q21[b] = dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=at_distance(da, d21), valid=v21)
        return a, b
    # bestDist <= TH_HIGH in each direction (:1264, :1344)
    for j, (d12, d21) in enumerate(((100, 0), (101, 0), (0, 100), (0, 101))):
        a, b = pair(j, d12, d21)
        ok = max(d12, d21) == 100
        s.hold(a, b if ok else -1)
        s.want(a, R.ACCEPTED if ok else (R.OVER_TH if d12 == 101 else R.NO_AGREEMENT), best_dist=d12)
    # valid = 0 on either side
    a, b = pair(4, 0, 0, v12=0); s.hold(a, -1); s.want(a, R.INVALID)
    a, b = pair(5, 0, 0, v21=0); s.hold(a, -1); s.want(a, R.NO_AGREEMENT, best_idx=b)
    # 1->2 and 2->1 disagree: a0 -> b0, b0 -> a1 (a1's descriptor is nearer to b0's point), a1 -> nothing
    u, v = ox + 20, oy + 70
    da, db = new_desc(), new_desc()
    a0 = s.k1.add(u, v, 0, at_distance(da, 30)); a1 = s.k1.add(u + 1, v, 0, da); b0 = s.kp(u, v, 0, db)
    s.q.append(dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=db, valid=1))
    s.q.append(dict(NO_QUERY))
    s.q21[b0] = dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=da, valid=1)
    s.hold(a0, -1); s.hold(a1, -1); s.want(a0, R.NO_AGREEMENT, best_idx=b0); s.want(a1, R.INVALID)
    # no occupancy: a2 and a3 both choose b1; b1 chooses a3: only a3 is kept
    u, v = ox + 70, oy + 70
    da, db = new_desc(), new_desc()
    a2 = s.k1.add(u, v, 0, at_distance(da, 25)); a3 = s.k1.add(u + 1, v, 0, da); b1 = s.kp(u, v, 0, db)
    s.q.append(dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=at_distance(db, 3), valid=1))
    s.q.append(dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=at_distance(db, 9), valid=1))
    s.q21[b1] = dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=da, valid=1)
    s.hold(a2, -1); s.hold(a3, b1); s.want(a2, R.NO_AGREEMENT, best_idx=b1, best_dist=3); s.want(a3, R.ACCEPTED, best_idx=b1, best_dist=9)
    # a tie takes the first minimum, in both directions
    u, v = ox + 120, oy + 70
    da, db = new_desc(), new_desc()
    a4 = s.k1.add(u, v, 0, at_distance(da, 11)); a5 = s.k1.add(u + 1, v, 0, at_distance(da, 11, 90))
    b2 = s.kp(u, v, 0, at_distance(db, 6)); b3 = s.kp(u, v + 1, 0, at_distance(db, 6, 90))
    s.q.append(dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=db, valid=1))
    s.q.append(dict(NO_QUERY))
    s.q21[b2] = dict(u=F(u), v=F(v), ur=F(0), radius=F(4), level=0, desc=da, valid=1)
    s.hold(a4, b2); s.hold(a5, -1); s.want(a4, R.ACCEPTED, n_compared=2, best_idx=b2, best_dist=6)
    assert len(s.q) == len(s.k1.rows)
    return s.done()


def sim3_scenes():
    return window_scenes("sim3") + [sim3_gates()]


# =================================================================================================================================
# SearchForInitialization
# =================================================================================================================================
def _init_scene(name, nn_ratio=0.9, window=10):
    return Scene(name, "init", nn_ratio=nn_ratio, window=window)


def _i1(s, x, y, desc, octave=0, prev=None, angle=0.0):
    i = s.k1.add(x, y, octave, desc, angle=angle)
    s.prev.append((F(x), F(y)) if prev is None else (F(prev[0]), F(prev[1])))
    return i


def _twins(s, ox, oy, n):
    """n certain matches in bin 0"""
    for j in range(n):
        x, y = ox + 8 + 24 * (j % 6), oy + 8 + 24 * (j // 6)
        d = new_desc()
        a = _i1(s, x, y, d); b = s.kp(x + 1, y + 1, 0, d)
        s.hold(a, b)


def init_window():
    """the window is Frame::GetFeaturesInArea(vbPrevMatched[i1], windowSize, 0, 0): strict at r = 10, clamped at the image sides, octave 0 only,
    centred on vbPrevMatched and not on the keypoint"""
    s = _init_scene("window")
    ox, oy = tile(1, 1)
    for j, (sx, sy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        for k, inside in enumerate((False, True)):
            u, v = ox + 20 + 40 * j, oy + 30 + 60 * k
            x, y = F(u + 10 * sx), F(v + 10 * sy)
            if inside:
                x, y = nxt(x, F(u)) if sx else x, nxt(y, F(v)) if sy else y
            d = new_desc()
            a = _i1(s, u, v, d); b = s.kp(x, y, 0, at_distance(d, 10))
            s.want(a, R.ACCEPTED if inside else R.EMPTY_WINDOW, n_window=1 if inside else 0)
            if inside:
                s.hold(a, b)
    for (u, v), (kx, ky) in (((3, 60), (1, 62)), ((80, 3), (83, 1)), ((637, 420), (634, 421)), ((500, 477), (502, 474))):
        d = new_desc()
        a = _i1(s, u, v, d); b = s.kp(kx, ky, 0, at_distance(d, 20))
        s.want(a, R.ACCEPTED, n_window=1); s.hold(a, b)
    ox, oy = tile(2, 1)
    # an octave-1 keypoint of F1 is skipped (:428); one of F2 is no candidate although it is the nearest
    d = new_desc()
    a = _i1(s, ox + 20, oy + 20, d, octave=1); s.kp(ox + 20, oy + 21, 0, d)
    s.want(a, R.SKIPPED_LEVEL)
    d = new_desc()
    a = _i1(s, ox + 60, oy + 20, d); s.kp(ox + 60, oy + 21, 1, d); b = s.kp(ox + 61, oy + 20, 0, at_distance(d, 20))
    s.want(a, R.ACCEPTED, n_window=1, best_dist=20); s.hold(a, b)
    # centred on vbPrevMatched: the keypoint's own neighbour (distance 0) is not seen, the one at the previous match is
    d = new_desc()
    a = _i1(s, ox + 20, oy + 60, d, prev=(ox + 70, oy + 60)); s.kp(ox + 21, oy + 60, 0, d); b = s.kp(ox + 71, oy + 61, 0, at_distance(d, 30))
    s.want(a, R.ACCEPTED, n_window=1, best_dist=30); s.hold(a, b)
    # a window over four cells, the tie going to the first in window order
    u, v = ox + 105, oy + 95; d = new_desc()
    a = _i1(s, u, v, d)
    s.kp(u + 3, v - 3, 0, at_distance(d, 40)); b = s.kp(u - 3, v + 3, 0, at_distance(d, 12)); s.kp(u - 3, v - 3, 0, at_distance(d, 45))
    s.want(a, R.ACCEPTED, n_window=3, best_dist=12, best_dist2=40); s.hold(a, b)
    return s.done()


def init_gates():
    """TH_LOW (:465), the ratio (:467) with mfNNratio = 0.9f: (float)50 * 0.9f rounds to 45.0f, so 45 against 50 fails and 44 passes"""
    s = _init_scene("th_and_ratio")
    ox, oy = tile(2, 2)
    assert F(F(50) * F(0.9)) == F(45)
    cases = (("th_50", 50, None, R.ACCEPTED), ("th_51", 51, None, R.OVER_TH), ("ratio_45_50", 45, 50, R.RATIO_FAILED), ("ratio_44_50", 44, 50, R.ACCEPTED),
             ("equal_best", 10, 10, R.RATIO_FAILED), ("single", 30, None, R.ACCEPTED))
    for j, (name, d1, d2, oc) in enumerate(cases):
        u, v = ox + 16 + 48 * (j % 3), oy + 16 + 48 * (j // 3); d = new_desc()
        a = _i1(s, u, v, d); b = s.kp(u + 1, v, 0, at_distance(d, d1))
        if d2 is not None:
            s.kp(u + 1, v + 1, 0, at_distance(d, d2, 128))
        s.want(a, oc, best_dist=d1, best_dist2=R.INT_MAX if d2 is None else d2, best_idx=b)
        if oc == R.ACCEPTED:
            s.hold(a, b)
    return s.done()


def init_steals():
    """vMatchedDistance[i2] <= dist (:450) with a lower distance (steals), an equal and a higher one (both skipped); the stolen match sits in a
    rotation bin that is rejected afterwards: nmatches went down when it was stolen (:472) and not again (:510); a plain rejected bin;
    vbPrevMatched moves for the survivors only (:521-523)"""
    s = _init_scene("steals")
    ox, oy = tile(3, 1)
    _twins(s, ox, oy, 12)                                                               # bin 0 holds 12 (+ 1 below): a bin of one is rejected
    u, v = ox + 20, oy + 100; d = new_desc()
    k = s.kp(u, v, 0, d, angle=0.0)
    a = _i1(s, u + 1, v, at_distance(d, 20), angle=150.0)                               # takes k at 20, bin 5 ...
    b = _i1(s, u - 1, v, at_distance(d, 20, 60))                                        # equal: skipped
    c = _i1(s, u, v + 1, at_distance(d, 30, 120))                                       # higher: skipped
    e = _i1(s, u, v - 1, at_distance(d, 10, 180))                                       # lower: steals, bin 0
    s.want(a, R.ACCEPTED_THEN_STOLEN, best_dist=20, bin=5); s.want(b, R.OCCUPIED, n_window=1, n_compared=0); s.want(c, R.OCCUPIED, n_compared=0)
    s.want(e, R.ACCEPTED, best_dist=10, bin=0); s.hold(e, k)
    u, v = ox + 80, oy + 100; d = new_desc()
    r = _i1(s, u, v, d, angle=210.0); s.kp(u + 1, v, 0, d)                              # bin 7 alone: removed
    s.want(r, R.ROT_REMOVED, bin=7)
    s.nmatches = {True: 13, False: 14}
    return s.done()


def init_scenes():
    return [init_window(), init_gates(), init_steals()]


# =================================================================================================================================
# SearchByBoW(KeyFrame*, KeyFrame*)
# =================================================================================================================================
def _bin0(s, node, n):
    for _ in range(n):
        d = new_desc()
        a = s.f1(node, d); b = s.f2(node, d)
        s.hold(a, b)


def bow_gates():
    """nodes 3 10 20 40 41 50 on side 1 against 5 10 15 20 30 41 50 on side 2: both lower_bound jumps happen, 3 and 40 (5, 15, 30) are on one
    side only"""
    s = Scene("nodes_and_gates", "bow", nn_ratio=0.75)
    lone1 = s.f1(3, new_desc()); lone2 = s.f1(40, new_desc())
    for nd in (5, 15, 30):
        s.f2(nd, new_desc())
    s.want(lone1, R.NODE_NOT_SHARED); s.want(lone2, R.NODE_NOT_SHARED)
    # node 10: bestDist1 < TH_LOW is strict (:604)
    for dist in (49, 50):
        d = new_desc()
        a = s.f1(10, d); b = s.f2(10, at_distance(d, dist))
        s.want(a, R.ACCEPTED if dist == 49 else R.OVER_TH, best_dist=dist)
        if dist == 49:
            s.hold(a, b)
    # node 20: vbMatched2 (:582, :609)
    d = new_desc()
    p0 = s.f2(20, d); p1 = s.f2(20, at_distance(d, 20, 40)); p2 = s.f2(20, at_distance(d, 30, 100)); p3 = s.f2(20, at_distance(d, 32, 160))
    x1 = s.f1(20, at_distance(d, 5, 200)); x2 = s.f1(20, at_distance(d, 3, 220)); x3 = s.f1(20, at_distance(d, 2, 240))
    s.want(x1, R.ACCEPTED, best_idx=p0, best_dist=5, n_compared=4); s.hold(x1, p0)
    s.want(x2, R.ACCEPTED, best_idx=p1, best_dist=23, n_compared=3); s.hold(x2, p1)            # its best is taken: the next best
    s.want(x3, R.RATIO_FAILED, best_idx=p2, best_dist=32, best_dist2=34, n_compared=2)           # 32 against 0.75f * 34
    # node 41: a KF2 feature without a map point is skipped inside the loop; a KF1 feature without one is skipped outright;
    # a feature whose candidates are all taken or without a point
    d = new_desc()
    a = s.f1(41, d); s.f2(41, at_distance(d, 2), has=0); b = s.f2(41, at_distance(d, 25, 50))
    s.want(a, R.ACCEPTED, best_idx=b, best_dist=25, n_compared=1); s.hold(a, b)
    n = s.f1(41, at_distance(d, 25, 50), has=0); s.want(n, R.MAP_POINT)
    o = s.f1(10, new_desc()); s.want(o, R.OVER_TH, n_compared=1)                                # node 10: the feature at 49 is taken, the other is far
    # node 50: the rotation histogram: 12 in bin 0, one in bin 9
    _bin0(s, 50, 12)
    d = new_desc()
    r = s.f1(50, d, angle=270.0); s.f2(50, d)
    s.want(r, R.ROT_REMOVED, bin=9)
    d = new_desc()
    occ = s.f1(60, d); s.f2(60, d, has=0)
    s.want(occ, R.OCCUPIED, n_compared=0)
    s.walk = dict(jumps1=2, jumps2=3, nodes=[10, 20, 41, 50, 60])
    return s.done()


def bow_scenes():
    return [bow_gates()]


# =================================================================================================================================
# SearchForTriangulation
# =================================================================================================================================
F12_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F)                       # a = 0, b = 1, c = -y1: the line is the row y2 = y1
F12_TILTED = np.array([[0, 0, 0], [2.0 ** -7, 2.0 ** -6, -1], [0, 1, 0]], F)     # a = y1 / 128, b = 1 + y1 / 64, c = -y1
F12_NULL = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], F)                        # a = b = 0: den == 0 for every pair
EPIPOLE = (24.0, 16.0)                                                          # small coordinates: float32 steps fine enough to land beside the gate
FAR_EPIPOLE = (1.0e6, 240.0)


def _tri(name, F12, epipole, only_stereo=False):
    return Scene(name, "triangulation", F12=F12, ex=epipole[0], ey=epipole[1], only_stereo=only_stereo)


def epi_v(x1, y1, x2, y2, F12):
    """dsqr of CheckDistEpipolarLine (:149-160) on float32 arrays"""
    f = np.asarray(F12, F)
    a = x1 * f[0, 0] + y1 * f[1, 0] + f[2, 0]; b = x1 * f[0, 1] + y1 * f[1, 1] + f[2, 1]; c = x1 * f[0, 2] + y1 * f[1, 2] + f[2, 2]
    num = a * x2 + b * y2 + c
    return (num * num) / (a * a + b * b)


def tri_gates(only_stereo=False):
    s = _tri("gates" + ("_only_stereo" if only_stereo else ""), F12_ROWS, EPIPOLE, only_stereo)
    st = int(only_stereo)
    node = 7
    lone = s.f1(2, new_desc(), stereo=1); s.f2(4, new_desc(), stereo=1); s.want(lone, R.NODE_NOT_SHARED)
    # dist > TH_LOW (:744): 50 is taken (bestDist starts AT TH_LOW), 51 is not
    for dist in (50, 51):
        d = new_desc(); node += 1
        a = s.f1(node, d, stereo=st, x=100, y=50); b = s.f2(node, at_distance(d, dist), stereo=st, x=90, y=50)
        s.want(a, R.ACCEPTED if dist == 50 else R.OVER_TH, best_dist=50)
        if dist == 50:
            s.hold(a, b)
    # dist > bestDist: a later EQUAL distance replaces the earlier one
    d = new_desc(); node += 1
    a = s.f1(node, d, stereo=st, x=100, y=60); s.f2(node, at_distance(d, 20), stereo=st, x=90, y=60); b = s.f2(node, at_distance(d, 20, 70), stereo=st, x=91, y=60)
    s.want(a, R.ACCEPTED, n_taken=2, best_idx=b); s.hold(a, b)
    # vbMatched2 is never set: two KF1 features end on the same KF2 feature
    d = new_desc(); node += 1
    a = s.f1(node, at_distance(d, 4), stereo=st, x=100, y=70); a2 = s.f1(node, at_distance(d, 6, 30), stereo=st, x=101, y=70)
    b = s.f2(node, d, stereo=st, x=90, y=70); s.f2(node, at_distance(d, 40, 100), stereo=st, x=91, y=70)
    s.want(a, R.ACCEPTED, best_idx=b); s.want(a2, R.ACCEPTED, best_idx=b); s.hold(a, b); s.hold(a2, b)
    # features that own a map point: on side 1 skipped (:708), on side 2 no candidate (:731)
    d = new_desc(); node += 1
    a = s.f1(node, d, has=1, stereo=st, x=100, y=80); s.f2(node, d, stereo=st, x=90, y=80)
    s.want(a, R.MAP_POINT)
    d = new_desc(); node += 1
    a = s.f1(node, d, stereo=st, x=100, y=90); s.f2(node, d, has=1, stereo=st, x=90, y=90); b = s.f2(node, at_distance(d, 30), stereo=st, x=91, y=90)
    s.want(a, R.ACCEPTED, best_idx=b, best_dist=30); s.hold(a, b)
    d = new_desc(); node += 1
    a = s.f1(node, d, stereo=st, x=100, y=95); s.f2(node, d, has=1, stereo=st, x=90, y=95)
    s.want(a, R.OCCUPIED)
    # the row-aligned line: dsqr = (y2 - y1)^2 against 3.84: one row off passes, two rows off (4 > 3.84) do not
    for off, ok in ((1, True), (2, False)):
        d = new_desc(); node += 1
        a = s.f1(node, d, stereo=st, x=100, y=100); b = s.f2(node, d, stereo=st, x=90, y=100 + off)
        s.want(a, R.ACCEPTED if ok else R.OFF_EPIPOLAR_LINE, dsqr=F(off * off), den=F(1))
        if ok:
            s.hold(a, b)
    # the epipole gate (:749-754): only when BOTH are mono; e2 < 100 * mvScaleFactors[octave], a float
    for o in (0, 1):
        T = F(F(100) * SCALE[o])
        fn = lambda x2, y2: (F(EPIPOLE[0]) - x2) * (F(EPIPOLE[0]) - x2) + (F(EPIPOLE[1]) - y2) * (F(EPIPOLE[1]) - y2)
        for target, close in ((T, False), (nxt(T, DOWN), True)):
            got = hit(fn, target, ulps(EPIPOLE[0] - 8, 400), ulps(EPIPOLE[1] - np.sqrt(float(T) - 64.0), 400))      # dx = 8, dy^2 = T - 64
            assert got is not None, "no float32 keypoint at e2 == %r" % target
            for s1, s2 in ((0, 0), (1, 0), (0, 1)):
                if only_stereo and not (s1 and s2):
                    continue
                d = new_desc(); node += 1
                a = s.f1(node, d, stereo=s1, x=100, y=got[1]); b = s.f2(node, d, stereo=s2, x=got[0], y=got[1], octave=o)
                gated = close and not s1 and not s2
                s.want(a, R.EPIPOLE_TOO_CLOSE if gated else R.ACCEPTED, **(dict(epipole_d2=target) if not (s1 or s2) else {}))
                if not gated:
                    s.hold(a, b)
    # bOnlyStereo (:713, :736)
    d = new_desc(); node += 1
    a = s.f1(node, d, stereo=0, x=100, y=110); b = s.f2(node, d, stereo=1, x=90, y=110)
    s.want(a, R.NOT_STEREO if only_stereo else R.ACCEPTED)
    if not only_stereo:
        s.hold(a, b)
    d = new_desc(); node += 1
    a = s.f1(node, d, stereo=1, x=100, y=115); s.f2(node, d, stereo=0, x=90, y=115); b = s.f2(node, at_distance(d, 35), stereo=1, x=91, y=115)
    s.want(a, R.ACCEPTED, best_idx=b if only_stereo else b - 1); s.hold(a, b if only_stereo else b - 1)
    d = new_desc(); node += 1
    a = s.f1(node, d, stereo=1, x=100, y=118); b = s.f2(node, d, stereo=0, x=90, y=118)
    s.want(a, R.NOT_STEREO if only_stereo else R.ACCEPTED)
    if not only_stereo:
        s.hold(a, b)
    # the rotation histogram: 12 in bin 0, one in bin 4
    for _ in range(12):
        d = new_desc(); node += 1
        a = s.f1(node, d, stereo=1, x=100, y=130); b = s.f2(node, d, stereo=1, x=90, y=130)
        s.hold(a, b)
    d = new_desc(); node += 1
    r = s.f1(node, d, stereo=1, x=100, y=140, angle=120.0); s.f2(node, d, stereo=1, x=90, y=140)
    s.want(r, R.ROT_REMOVED, bin=4)
    return s.done()


def tri_tilted():
    """a general F12 (a, b, c all depend on the KF1 keypoint) and dsqr on either side of the DOUBLE 3.84 * mvLevelSigma2[octave] for octaves 0
    and 1: the last float below it is on the line, the first float not below it is off"""
    s = _tri("tilted_dsqr", F12_TILTED, FAR_EPIPOLE)
    node = 100
    for o in (0, 1):
        t = 3.84 * float(SIGMA2[o])
        lo = F(t) if float(F(t)) < t else nxt(F(t), DOWN)
        hi = nxt(lo, UP)
        assert float(lo) < t <= float(hi)
        for target, ok in ((lo, True), (hi, False)):
            got = None
            for y1, x2 in ((y1, x2) for y1 in range(1, 48) for x2 in (F(128), F(0), F(64))):
                a, b = y1 / 128.0, 1.0 + y1 / 64.0
                y0 = (np.sqrt(t * (a * a + b * b)) - a * float(x2) + y1) / b
                got = hit(lambda p, y2: epi_v(F(100), p, x2, y2, F12_TILTED), target, [F(y1)], ulps(y0, 200))
                if got is not None:
                    break
            assert got is not None, "no float32 pair at dsqr == %r" % target
            d = new_desc(); node += 1
            a1 = s.f1(node, d, x=100, y=got[0]); b2 = s.f2(node, d, x=x2, y=got[1], octave=o)
            s.want(a1, R.ACCEPTED if ok else R.OFF_EPIPOLAR_LINE, dsqr=target)
            if ok:
                s.hold(a1, b2)
    # on the line and far off it
    d = new_desc(); node += 1
    a1 = s.f1(node, d, x=100, y=32); b2 = s.f2(node, d, x=2, y=21)                  # a = 0.25, b = 1.5, c = -32: 0.5 + 31.5 - 32 = 0
    s.want(a1, R.ACCEPTED, a=F(0.25), b=F(1.5), c=F(-32), num=F(0), dsqr=F(0)); s.hold(a1, b2)
    d = new_desc(); node += 1
    a1 = s.f1(node, d, x=100, y=32); s.f2(node, d, x=2, y=30)                       # num = 13.5, den = 2.3125
    s.want(a1, R.OFF_EPIPOLAR_LINE, num=F(13.5), den=F(2.3125))
    return s.done()


def tri_null():
    s = _tri("den_zero", F12_NULL, FAR_EPIPOLE)
    d = new_desc()
    a = s.f1(5, d, x=100, y=50); s.f2(5, d, x=90, y=50)
    s.want(a, R.DEN_ZERO, den=F(0), a=F(0), b=F(0))
    return s.done()


def triangulation_scenes():
    return [tri_gates(False), tri_gates(True), tri_tilted(), tri_null()]


# =================================================================================================================================
# all of them; the concatenation of the scenes of one call; the restatement and the oracle on a scene
# =================================================================================================================================
def all_scenes():
    return dict(keyframe=keyframe_scenes(), fuse=fuse_scenes("fuse"), fuse_scw=fuse_scenes("fuse_scw"), sim3=sim3_scenes(), init=init_scenes(),
                bow=bow_scenes(), triangulation=triangulation_scenes())


def groups(scenes):
    out = {}
    for sc in scenes:
        out.setdefault(sc.group, []).append(sc)
    return list(out.values())


def _cat_rec(recs):
    return dict(kps=np.concatenate([r["kps"] for r in recs]), desc=np.concatenate([r["desc"] for r in recs]), uright=np.concatenate([r["uright"] for r in recs]))


def _cat_q(qs):
    return {k: np.concatenate([q[k] for q in qs]) for k in QKEYS}


def concat(scs):
    """the scenes of one group as ONE call: keypoints, queries and features appended, indices and node ids shifted.  Only inputs: what the
    call must give comes from the restatement on the whole."""
    c = Scene("+".join(s.name for s in scs), scs[0].search, **scs[0].params)
    c.rec1, c.rec2 = _cat_rec([s.rec1 for s in scs]), _cat_rec([s.rec2 for s in scs])
    o1 = np.cumsum([0] + [len(s.rec1["kps"]) for s in scs]); o2 = np.cumsum([0] + [len(s.rec2["kps"]) for s in scs])
    if c.search in ("keyframe", "fuse", "fuse_scw", "sim3"):
        c.Q = _cat_q([s.Q for s in scs])
    if c.search == "keyframe":
        c.matched = np.concatenate([s.matched for s in scs])
    if c.search == "sim3":
        c.Q21 = _cat_q([s.Q21 for s in scs])
    if c.search == "init":
        c.prev_xy = np.concatenate([s.prev_xy for s in scs])
    for a in ("has1", "has2", "st1", "st2"):
        setattr(c, a, np.concatenate([getattr(s, a) for s in scs]))
    for k, s in enumerate(scs):
        for nd, idx in s.fv1.items():
            c.fv1[1000 * k + nd] = [int(i + o1[k]) for i in idx]
        for nd, idx in s.fv2.items():
            c.fv2[1000 * k + nd] = [int(i + o2[k]) for i in idx]
    return c


def run_ref(sc, ori=True, fault=None):
    """-> (result arrays, count or None, outcome per item, infos)"""
    p, k1, k2 = sc.params, sc.rec1, sc.rec2
    if sc.search == "keyframe":
        m, nm, oc, inf = R.search_keyframe_points(k2["kps"], k2["desc"], BOUNDS, sc.Q, sc.matched, fault)
        return [m], nm, oc, inf
    if sc.search in ("fuse", "fuse_scw"):
        bi, bd, oc, inf = R.fuse_candidates(k2["kps"], k2["desc"], k2["uright"], BOUNDS, p["inv_sigma2"], sc.Q, fault)
        return [bi, bd], None, oc, inf
    if sc.search == "sim3":
        m, nf, oc, inf = R.search_by_sim3(k1["kps"], k1["desc"], BOUNDS, k2["kps"], k2["desc"], BOUNDS, sc.Q, sc.Q21, fault)
        return [m], nf, np.concatenate(oc), inf[0] + inf[1]
    if sc.search == "init":
        m, prev, nm, oc, inf = R.search_for_initialization(k1["kps"], k1["desc"], k2["kps"], k2["desc"], BOUNDS, sc.prev_xy, p["window"], p["nn_ratio"], ori, fault)
        return [m, prev], nm, oc, inf
    if sc.search == "bow":
        m, nm, oc, inf, walk = R.search_by_bow_keyframes(k1["kps"], k1["desc"], sc.has1, sc.fv1, k2["kps"], k2["desc"], sc.has2, sc.fv2, p["nn_ratio"], ori, fault)
        return [m], nm, oc, inf
    m, nm, oc, inf = R.search_for_triangulation(k1["kps"], k1["desc"], sc.has1, sc.st1, sc.fv1, k2["kps"], k2["desc"], sc.has2, sc.st2, sc.fv2, p["F12"], p["ex"], p["ey"],
                                                SCALE, SIGMA2, p["only_stereo"], ori, fault)
    return [m], nm, oc, inf


def run_entry(E, M, sc, ori=True):
    """the same call through an entry point with the oracle's (E = oracle_lib, M = None) or the device's (E = None, M = iv.ORBmatcher) signature"""
    p, k1, k2 = sc.params, sc.rec1, sc.rec2
    if sc.search == "keyframe":
        m, nm = E.search_keyframe_points(k2["kps"], k2["desc"], BOUNDS, sc.Q, sc.matched) if E else M(0.6, ori).SearchByProjectionKeyFrame(k2["kps"], k2["desc"], BOUNDS, sc.Q, sc.matched)
        return [m], nm
    if sc.search in ("fuse", "fuse_scw"):
        ur = k2["uright"] if p["inv_sigma2"] is not None else None
        bi, bd = E.fuse_candidates(k2["kps"], k2["desc"], ur, BOUNDS, p["inv_sigma2"], sc.Q) if E else M(0.6, ori).FuseCandidates(k2["kps"], k2["desc"], ur, BOUNDS, p["inv_sigma2"], sc.Q)
        return [bi, bd], None
    if sc.search == "sim3":
        a = (k1["kps"], k1["desc"], BOUNDS, k2["kps"], k2["desc"], BOUNDS, sc.Q, sc.Q21)
        m, nf = E.search_by_sim3(*a) if E else M(0.6, ori).SearchBySim3(*a)
        return [m], nf
    if sc.search == "init":
        a = (k1["kps"], k1["desc"], k2["kps"], k2["desc"], BOUNDS, sc.prev_xy, p["window"])
        m, prev, nm = E.search_for_initialization(*a, p["nn_ratio"], ori) if E else M(p["nn_ratio"], ori).SearchForInitialization(*a)
        return [m, prev], nm
    if sc.search == "bow":
        a = (k1["kps"], k1["desc"], sc.has1, sc.fv1, k2["kps"], k2["desc"], sc.has2, sc.fv2)
        m, nm = E.search_by_bow_keyframes(*a, p["nn_ratio"], ori) if E else M(p["nn_ratio"], ori).SearchByBoWKeyFrames(*a)
        return [m], nm
    a = (k1["kps"], k1["desc"], sc.has1, sc.st1, sc.fv1, k2["kps"], k2["desc"], sc.has2, sc.st2, sc.fv2, p["F12"], p["ex"], p["ey"], SCALE, SIGMA2, p["only_stereo"])
    m, nm = E.search_for_triangulation(*a, ori) if E else M(0.6, ori).SearchForTriangulation(*a)
    return [m], nm


def same_result(a, na, b, nb):
    return na == nb and len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def describe(outcome, infos, i):
    """what a failure message says about item i"""
    keys = ("n_window", "n_level", "n_compared", "best_dist", "best_dist2", "best_idx", "e2", "chi2", "epipole_d2", "den", "dsqr", "bin", "node")
    return "item %d: %s (%s)" % (i, R.NAMES[outcome[i]], ", ".join("%s %s" % (k, infos[i][k]) for k in keys if k in infos[i]))


def explain(sc, got, exp, outcome, infos):
    """the slots on which two results differ, with where the restatement says the items involved left the loop"""
    lines = []
    for g, e in zip(got, exp):
        g = np.asarray(g).reshape(len(g), -1); e = np.asarray(e).reshape(len(e), -1)
        for k in np.nonzero((g != e).any(axis=1))[0][:6]:
            if sc.search == "keyframe":
                items = sorted(set(int(q) for q in (g[k, 0], e[k, 0]) if 0 <= q < len(outcome)))
            else:
                items = [int(k)]
            lines.append("slot %d holds %s, expected %s; %s" % (k, g[k].tolist(), e[k].tolist(), "; ".join(describe(outcome, infos, i) for i in items)))
    return "scene %s (%s)\n%s" % (sc.name, sc.search, "\n".join(lines))
