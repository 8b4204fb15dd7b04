"""reloc_scenes.py -- hand-made scenes for ivf_tracker_search_reloc, the batched ORBmatcher::SearchByProjection(CurrentFrame, pKF,
sAlreadyFound, th, ORBdist) (ORB/src/ORBmatcher.cc:1520-1652): keyframe map points and current keypoints placed ON every comparison of the
loop and one step beside it, in the manner of tests/projection_scenes.py and with its exact camera (fx = fy = 256, cx = 320, cy = 120, a
640 x 240 image; a point at depth 4 projects to u = 320 + 64 x, v = 120 + 64 y).

A scene is one (keyframe, current) pair: keyframe keypoints with the map point each holds (the pool of the oracle holds one point per keyframe
keypoint, so map point ids ARE keyframe keypoint indices), current keypoints with the keyframe keypoint each holds on entry, and a list
of calls (th, orb_dist, found or None).  `expect` = (call, keyframe keypoint, gate), `holds` = (current keypoint, keyframe keypoint or -1
at the end).  walk() is a plain-Python restatement that names the gate at which every keyframe keypoint leaves the loop;
tests/test_reloc_scenes_cpu.py checks it and the expectations against oracle/projection_oracle.py:search_reloc,
tests/test_gpu_track_reloc.py runs the device on the same scenes."""
import math

import numpy as np

import projection_scenes as PS
from projection_scenes import F, UP, DOWN, nxt, new_desc, at_distance, world, spot, SCALE, KP_DTYPE, _first

NF = 256
D = np.float64
(NO_POINT, BAD, FOUND, OUT_OF_IMAGE, TOO_NEAR, TOO_FAR, EMPTY_WINDOW, ALL_OCCUPIED, TOO_DISTANT, MATCHED, ROTATED_OUT) = range(11)
NAMES = ("no point", "bad point", "already found", "out of the image", "too near", "too far", "empty window", "every candidate occupied",
         "best distance above ORBdist", "matched", "matched, taken back by the rotation filter")
I4 = np.eye(4, dtype=F)
FAR = 64.0                                      # default maxDist: PredictScale's quotient clamps at level 7 unless a scene sets it


def cam(bounds=(0.0, 0.0, 640.0, 240.0), nf=NF):
    return dict(PS.CAM, nf=nf, bounds=bounds)


class Scene:
    def __init__(self, name, calls=((10.0, 100, "given"),), ori=True, T=I4, bounds=(0.0, 0.0, 640.0, 240.0), nf=NF):
        self.name, self.ori, self.T, self.cam = name, ori, np.array(T, F), cam(bounds, nf)
        self.calls = [dict(th=F(c[0]), orb_dist=int(c[1]), given=(c[2] == "given")) for c in calls]
        self.kf, self.cur = PS._Keys(), PS._Keys()
        self.points, self.found, self.assign_in, self.expect, self.holds = [], set(), [], [], []

    @property
    def group(self):
        return (self.cam["nf"], self.cam["bounds"], self.ori, tuple((float(c["th"]), c["orb_dist"], c["given"]) for c in self.calls))

    def pt(self, pos, desc, lv=None, minDist=1.0, maxDist=None, angle=0.0, bad=False, none=False, found=False, kxy=(1.0, 1.0)):
        """a keyframe keypoint and the map point it holds; lv: the level PredictScale is to give (maxDist in the middle of its interval)"""
        pos = np.asarray(pos, F)
        dist = float(np.sqrt((pos.astype(D) ** 2).sum()))
        if maxDist is None:
            maxDist = FAR if lv is None else dist * 1.2 ** (lv - 0.5)
        i = self.kf.add(kxy[0], kxy[1], 0, new_desc(), angle=angle)
        self.points.append(None if none else dict(pos=pos, minDist=F(minDist), maxDist=F(maxDist), desc=np.array(desc, np.uint8), bad=bool(bad)))
        if found:
            self.found.add(i)
        return i

    def kp(self, x, y, octave, desc, angle=0.0, holds=-1):
        self.assign_in.append(int(holds))
        return self.cur.add(x, y, octave, desc, angle=angle)

    def want(self, i, gate, call=0, **vals):
        self.expect.append((call, i, gate, vals))

    def hold(self, k, i):
        self.holds.append((k, i))

    def simple(self, j, gate, d=0, lv=0, octave=None, **kw):
        """one point on spot j with one keypoint at its projection, descriptor distance d"""
        u, v = spot(j)
        desc = new_desc()
        i = self.pt(world(u, v), desc, lv=lv, **kw)
        k = self.kp(u, v, lv if octave is None else octave, at_distance(desc, d))
        self.want(i, gate); self.hold(k, i if gate == MATCHED else -1)
        return i, k

    def done(self):
        assert len(self.kf.kx) <= self.cam["nf"] and len(self.cur.kx) <= self.cam["nf"]
        self.rec_kf, self.rec_cur = self.kf.record(), self.cur.record()
        self.assign0 = np.array(self.assign_in, np.int32)
        return self


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def window(sc, u, v, r, lo, hi):
    """Frame::GetFeaturesInArea (Frame.cc:615-668) on the current record: indices in the reference's order (grid column, grid row,
    insertion order)"""
    b = sc.cam["bounds"]
    invW = F(F(64.0) / F(F(b[2]) - F(b[0]))); invH = F(F(48.0) / F(F(b[3]) - F(b[1])))
    k = sc.rec_cur["kps"]
    x0 = max(0, int(math.floor(F(F(F(u - F(b[0])) - r) * invW)))); x1 = min(63, int(math.ceil(F(F(F(u - F(b[0])) + r) * invW))))
    y0 = max(0, int(math.floor(F(F(F(v - F(b[1])) - r) * invH)))); y1 = min(47, int(math.ceil(F(F(F(v - F(b[1])) + r) * invH))))
    px = np.round(((k["x"] - F(b[0])).astype(F) * invW).astype(F)).astype(np.int64); py = np.round(((k["y"] - F(b[1])).astype(F) * invH).astype(F)).astype(np.int64)
    ok = (px >= 0) & (px < 64) & (py >= 0) & (py < 48) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)      # np.round ties to even; no scene sits on a tie
    if lo > 0 or hi >= 0:
        ok &= ~(k["octave"] < lo)
        if hi >= 0:
            ok &= ~(k["octave"] > hi)
    ok &= (np.abs((k["x"] - F(u)).astype(F)) < F(r)) & (np.abs((k["y"] - F(v)).astype(F)) < F(r))
    idx = np.nonzero(ok)[0]
    return [int(i) for i in idx[np.lexsort((idx, py[idx], px[idx]))]]


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def walk(O, PO, sc, assign, call):
    """one call on `assign` (current keypoint -> keyframe keypoint or -1): (nmatches, assign after, gate per keyframe keypoint, infos)"""
    c = sc.calls[call]
    found = set(sc.found) if c["given"] else set(int(a) for a in assign if a >= 0)
    cm = sc.cam
    Rcw, tcw = sc.T[:3, :3], sc.T[:3, 3]
    Ow = PO.neg_rt_mul(Rcw, tcw)
    logscale = F(O.lib.orc_logf(float(SCALE[1])))
    assign = np.array(assign, np.int32)
    gates, infos, made = [], [], []
    hist = [0] * 30
    kc = sc.rec_cur["kps"]
    for i, p in enumerate(sc.points):
        info = {}
        infos.append(info)
        if p is None or p["bad"] or i in found:
            gates.append(NO_POINT if p is None else BAD if p["bad"] else FOUND)
            continue
        x = PO.mul_add(Rcw, p["pos"], tcw)
        with np.errstate(all="ignore"):
            invz = F(D(1.0) / D(x[2]))
            u = F(F(F(cm["fx"] * x[0]) * invz) + cm["cx"]); v = F(F(F(cm["fy"] * x[1]) * invz) + cm["cy"])
        info.update(u=u, v=v, zc=x[2])
        b = cm["bounds"]
        if u < F(b[0]) or u > F(b[2]) or v < F(b[1]) or v > F(b[3]):
            gates.append(OUT_OF_IMAGE)
            continue
        dist = F(PO.norm((p["pos"] - Ow).astype(F)))
        info.update(dist=dist)
        if dist < F(F(0.8) * p["minDist"]):
            gates.append(TOO_NEAR)
            continue
        if dist > F(F(1.2) * p["maxDist"]):
            gates.append(TOO_FAR)
            continue
        quot = F(F(O.lib.orc_logf(float(F(p["maxDist"] / dist)))) / logscale)
        lv = min(max(int(math.ceil(float(quot))), 0), 7)
        r = F(c["th"] * SCALE[lv])
        cand = window(sc, u, v, r, lv - 1, lv + 1)
        info.update(quotient=quot, level=lv, radius=r, n_window=len(cand), window=cand)
        if not cand:
            gates.append(EMPTY_WINDOW)
            continue
        best, bi = 256, -1
        for k in cand:
            if assign[k] != -1:
                continue
            d = hamming(p["desc"], sc.rec_cur["desc"][k])
            if d < best:
                best, bi = d, k
        info.update(best_dist=best, best_idx=bi)
        if bi < 0:
            gates.append(ALL_OCCUPIED)
            continue
        if best > c["orb_dist"]:
            gates.append(TOO_DISTANT)
            continue
        assign[bi] = i
        gates.append(MATCHED)
        bn = 0
        if sc.ori:
            rot = F(sc.rec_kf["kps"]["angle"][i] - kc["angle"][bi])
            if rot < 0:
                rot = F(rot + F(360.0))
            raw = int(np.floor(D(F(rot * F(F(1.0) / F(30.0)))) + 0.5))
            bn = 0 if raw == 30 else raw
            info.update(bin=bn, raw_bin=raw)
            hist[bn] += 1
        made.append((i, bi, bn))
    nm = len(made)
    if sc.ori:
        ind = [-1, -1, -1]; mx = [0, 0, 0]
        for bnum, s in enumerate(hist):
            if s > mx[0]:
                mx = [s, mx[0], mx[1]]; ind = [bnum, ind[0], ind[1]]
            elif s > mx[1]:
                mx = [mx[0], s, mx[1]]; ind = [ind[0], bnum, ind[1]]
            elif s > mx[2]:
                mx[2] = s; ind[2] = bnum
        if mx[1] < F(0.1) * F(mx[0]):
            ind[1] = ind[2] = -1
        elif mx[2] < F(0.1) * F(mx[0]):
            ind[2] = -1
        for i, bi, bn in made:
            if bn not in ind:
                assign[bi] = -1; gates[i] = ROTATED_OUT; nm -= 1
    return nm, assign, gates, infos


def oracle_search(O, PO, sc, assign, T, found, th, orb_dist):
    """one search through oracle/projection_oracle.py:search_reloc around the C oracle: (nmatches, assign after)"""
    import types
    T4 = np.eye(4, dtype=F); T4[:3, :4] = np.asarray(T, F).reshape(-1, 4)[:3]
    cur = dict(kps=sc.rec_cur["kps"], desc=sc.rec_cur["desc"], T=T4, scale=SCALE, logScale=F(O.lib.orc_logf(float(SCALE[1]))), fx=sc.cam["fx"],
               fy=sc.cam["fy"], cx=sc.cam["cx"], cy=sc.cam["cy"], bounds=sc.cam["bounds"])
    pool = [dict(pos=np.zeros(3, F), minDist=F(1), maxDist=F(1), desc=np.zeros(32, np.uint8), bad=True) if p is None else p for p in sc.points]
    kf = dict(kps=sc.rec_kf["kps"], mps=[-1 if p is None else i for i, p in enumerate(sc.points)])
    oo = O if sc.ori else types.SimpleNamespace(search_by_projection_reloc=lambda k, d, b, q, od, chk, occ: O.search_by_projection_reloc(k, d, b, q, od, False, occ))
    with np.errstate(all="ignore"):
        nm, out = PO.search_reloc(oo, cur, kf, pool, [int(a) for a in assign], set(int(f) for f in found), F(th), int(orb_dist))
    return nm, np.array(out, np.int32)


def oracle_call(O, PO, sc, assign, call):
    c = sc.calls[call]
    found = set(sc.found) if c["given"] else set(int(a) for a in assign if a >= 0)
    return oracle_search(O, PO, sc, assign, sc.T, found, c["th"], c["orb_dist"])


def kf_points(sc, nf, dtype):
    """the scene's d_kf_points row: one LOCAL_POINT_DTYPE record per keyframe keypoint, flags bit 0 on everything that holds no live point"""
    a = np.zeros(nf, dtype)
    a["flags"] = 1
    for i, p in enumerate(sc.points):
        if p is not None:
            a["pos"][i] = p["pos"]; a["min_distance"][i] = p["minDist"]; a["max_distance"][i] = p["maxDist"]; a["desc"][i] = p["desc"]
            a["flags"][i] = 1 if p["bad"] else 0
            a["normal"][i] = (np.nan, np.nan, np.nan)                       # ignored by this search
    return a


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------
def skip_rules():
    s = Scene("skip_rules")
    s.simple(0, MATCHED)
    for j, (gate, kw) in enumerate(((NO_POINT, dict(none=True)), (BAD, dict(bad=True)), (FOUND, dict(found=True))), 1):
        s.simple(j, gate, **kw)
    return s.done()


def image_bounds():
    """u = 64 x + 320: x = 5 is u = 640 exactly, two floats above 5 give the float after 640; x one float below -5 gives u = -2^-15.  v
    likewise with y = +-1.875.  Each point's keypoint lies 8 px inside the image, within the radius of 10."""
    s = Scene("image_bounds")
    for pin, pout, wit, uv_in, uv_out in (
            ([5, 0, 4], [nxt(5, UP, 2), 0, 4], (632, 120), (640, 120), (nxt(640), 120)),
            ([-5, 0, 4], [nxt(-5, DOWN), 0, 4], (8, 120), (0, 120), (F(-2.0 ** -15), 120)),
            ([0, 1.875, 4], [0, nxt(1.875, UP, 2), 4], (320, 234), (320, 240), (320, nxt(240))),
            ([0, -1.875, 4], [0, nxt(-1.875, DOWN), 4], (320, 6), (320, 0), (320, F(-2.0 ** -17)))):
        di, do = new_desc(), new_desc()
        a = s.pt(pin, di, lv=0); b = s.pt(pout, do, lv=0)
        ka = s.kp(wit[0], wit[1], 0, di); kb = s.kp(wit[0], wit[1], 0, do)
        s.want(a, MATCHED, u=F(uv_in[0]), v=F(uv_in[1]), radius=F(10)); s.want(b, OUT_OF_IMAGE, u=F(uv_out[0]), v=F(uv_out[1]))
        s.hold(ka, a); s.hold(kb, -1)
    return s.done()


def negative_bounds():
    """an undistorted image whose bounds start below zero: u = -8 (x = -5.125) and v = -4 are inside (-16, -8, 640, 240); u one float below
    -16 is outside"""
    s = Scene("negative_bounds", bounds=(-16.0, -8.0, 640.0, 240.0))
    da, db, dc = new_desc(), new_desc(), new_desc()
    a = s.pt([-5.125, 0, 4], da, lv=0); b = s.pt([0, -1.9375, 4], db, lv=0); c = s.pt([nxt(-5.25, DOWN), 0, 4], dc, lv=0)
    ka = s.kp(-12, 118, 0, da); kb = s.kp(322, -6, 0, db); kc = s.kp(-14, 124, 0, dc)
    s.want(a, MATCHED, u=F(-8), v=F(120)); s.want(b, MATCHED, u=F(320), v=F(-4)); s.want(c, OUT_OF_IMAGE)
    s.hold(ka, a); s.hold(kb, b); s.hold(kc, -1)
    return s.done()


def behind_the_camera():
    """zc = -4: invzc = -0.25, u = 320 - 64 x lands inside the image; the reference has no test on the sign and searches for the point"""
    s = Scene("behind_the_camera")
    d = new_desc()
    a = s.pt([1.0, 0.5, -4.0], d, lv=0)
    k = s.kp(256 + 3, 88 - 2, 0, at_distance(d, 7))
    s.want(a, MATCHED, u=F(256), v=F(88), zc=F(-4)); s.hold(k, a)
    return s.done()


def dist_range():
    """on the axis at depth 4: dist3D == 4.  0.8f * 5 rounds to 4 (inside); the first minDist above 5 whose product exceeds 4 is outside.
    Likewise a maxDist with 1.2f * maxDist == 4 and the one below it."""
    s = Scene("dist_range")
    near_out = _first(lambda m: F(F(0.8) * m) > F(4), F(5), UP)
    far_in = _first(lambda m: F(F(1.2) * m) == F(4), nxt(F(4.0 / 1.2), DOWN, 8), UP)
    far_out = _first(lambda m: F(F(1.2) * m) < F(4), far_in, DOWN)
    assert F(F(0.8) * F(5)) == F(4)
    for n, (mind, maxd, lv, gate) in enumerate(((5, 8, 4, MATCHED), (near_out, 8, 4, TOO_NEAR), (1, far_in, 0, MATCHED), (1, far_out, 0, TOO_FAR))):
        d = new_desc()
        p = s.pt([0, 0, 4], d, minDist=mind, maxDist=maxd)
        k = s.kp(318 + n, 120, lv, d)
        s.want(p, gate, dist=F(4), **(dict(level=lv) if gate == MATCHED else {})); s.hold(k, p if gate == MATCHED else -1)
    return s.done()


def scale_clamps():
    """PredictScale's clamp: maxDist / dist == 1 (logf gives 0), 0.9 (a negative quotient) and 16 (quotient 15.2) at both ends; the
    witnesses two octaves away from the clamped level carry the smaller distance and are outside [level - 1, level + 1]"""
    s = Scene("scale_clamps")
    for n, (ratio, lv, wrong) in enumerate(((1.0, 0, 2), (0.9, 0, 2), (16.0, 7, 5))):
        d = new_desc()
        u, v = (320.0, 120.0) if n == 0 else spot(n)
        pos = world(u, v)
        p = s.pt(pos, d, maxDist=F(ratio * float(np.sqrt((pos.astype(D) ** 2).sum()))))
        k = s.kp(u + 1, v, lv, at_distance(d, 9)); kw = s.kp(u, v + 1, wrong, at_distance(d, 1))
        s.want(p, MATCHED, level=lv, n_window=1, best_dist=9); s.hold(k, p); s.hold(kw, -1)
    return s.done()


def window_levels():
    """candidates on octaves lv - 2 .. lv + 2 around one projection: the two outside [lv - 1, lv + 1] carry the smallest distances.  One query
    per admitted octave, which holds that query's best; then lv = 0, whose lower bound -1 still keeps octave 2 out (Frame.cc:615-668)"""
    s = Scene("window_levels")
    for n, win in enumerate((1, 2, 3)):
        u, v = spot(n)
        d = new_desc()
        p = s.pt(world(u, v), d, lv=2)
        ks = {}
        for j, o in enumerate((0, 1, 2, 3, 4)):
            dd = 1 if o == 0 else 2 if o == 4 else 5 if o == win else 8 + o
            ks[o] = s.kp(u - 2 + j, v + (j % 2), o, at_distance(d, dd, shift=16 * j))
        s.want(p, MATCHED, level=2, n_window=3, best_dist=5)
        for o, k in ks.items():
            s.hold(k, p if o == win else -1)
    u, v = spot(5)
    d = new_desc()
    p = s.pt(world(u, v), d, lv=0)
    k0 = s.kp(u - 1, v, 0, at_distance(d, 9)); k1 = s.kp(u, v, 1, at_distance(d, 6)); k2 = s.kp(u + 1, v, 2, at_distance(d, 1))
    s.want(p, MATCHED, level=0, n_window=2, best_dist=6); s.hold(k0, -1); s.hold(k1, p); s.hold(k2, -1)
    return s.done()


def windows_empty_and_occupied():
    s = Scene("windows_empty_and_occupied")
    u, v = spot(0)
    d = new_desc()
    p = s.pt(world(u, v), d, lv=0)
    k = s.kp(u + 10, v, 0, d)                                                # |dx| < radius is strict: 10 px away is outside
    s.want(p, EMPTY_WINDOW, radius=F(10), n_window=0); s.hold(k, -1)
    u, v = spot(1)
    d = new_desc()
    h1 = s.pt(world(600, 200), new_desc(), found=True); h2 = s.pt(world(600, 200), new_desc(), found=True)
    p = s.pt(world(u, v), d, lv=0)
    ka = s.kp(u + 1, v, 0, d, holds=h1); kb = s.kp(u, v + 1, 0, at_distance(d, 3), holds=h2)
    s.want(p, ALL_OCCUPIED, n_window=2); s.hold(ka, h1); s.hold(kb, h2)
    return s.done()


def overflow(nf=NF, name="overflow"):
    """a window of 100 candidates (a 10 x 10 lattice of 2 px inside the 20 px box) for two queries with the same projection and
    descriptor.  By window position: 3 and 70 lie at distance 5, 10 and 20 at distance 2 but occupied on entry, the rest at 30.  The first
    query takes position 3, the second finds it taken and must reach position 70, past the 64 listed candidates."""
    s = Scene(name, nf=nf)
    u, v = 325.0, 122.5
    d = new_desc()
    holder = {10: s.pt(world(600, 200), new_desc(), found=True), 20: s.pt(world(600, 200), new_desc(), found=True)}
    q1 = s.pt(world(u, v), d, lv=0); q2 = s.pt(world(u, v), d, lv=0)
    pos = [(u - 9 + 2 * a, v - 9 + 2 * b) for a in range(10) for b in range(10)]
    tmp = Scene("tmp", nf=nf)
    for x, y in pos:
        tmp.kp(x, y, 0, d)
    tmp.rec_cur = tmp.cur.record()
    order = window(tmp, F(u), F(v), F(10), -1, 1)
    assert len(order) == 100
    rank = {k: r for r, k in enumerate(order)}
    ks = []
    for n, (x, y) in enumerate(pos):
        r = rank[n]
        dd = 5 if r in (3, 70) else 2 if r in (10, 20) else 30
        ks.append(s.kp(x, y, 0, at_distance(d, dd, shift=r), holds=holder.get(r, -1)))
    s.want(q1, MATCHED, n_window=100, best_dist=5, best_idx=order[3]); s.want(q2, MATCHED, n_window=100, best_dist=5, best_idx=order[70])
    s.hold(ks[order[3]], q1); s.hold(ks[order[70]], q2); s.hold(ks[order[10]], holder[10]); s.hold(ks[order[20]], holder[20])
    s.positions = dict(first=3, second=70, occupied=(10, 20))
    return s.done()


def acceptance_and_ties():
    s = Scene("acceptance_and_ties", calls=((10.0, 64, "given"),))
    s.simple(0, MATCHED, d=64, lv=0); s.simple(1, TOO_DISTANT, d=65, lv=0)
    # two candidates at the same distance: the one in the lower grid column is listed first
    u, v = spot(2)
    d = new_desc()
    p = s.pt(world(u, v), d, lv=0)
    kb = s.kp(u + 7, v, 0, at_distance(d, 11, shift=40)); ka = s.kp(u - 7, v, 0, at_distance(d, 11))
    s.want(p, MATCHED, n_window=2, best_dist=11, best_idx=ka); s.hold(ka, p); s.hold(kb, -1)
    # two queries whose best is the same keypoint: the second takes its next best
    u, v = spot(3)
    d = new_desc()
    p1 = s.pt(world(u, v), d, lv=0); p2 = s.pt(world(u + 1, v), d, lv=0)
    k1 = s.kp(u, v + 2, 0, at_distance(d, 4)); k2 = s.kp(u + 3, v - 2, 0, at_distance(d, 20))
    s.want(p1, MATCHED, best_dist=4, best_idx=k1); s.want(p2, MATCHED, best_dist=20, best_idx=k2); s.hold(k1, p1); s.hold(k2, p2)
    return s.done()


def rotation(nf=NF, name="rotation", ori=True):
    """matches in five bins of the rotation histogram (rot = 0, 60, 120, 180, 240 degrees -> bins 0, 2, 4, 6, 8 with 2, 3, 3, 1, 1 matches):
    ComputeThreeMaxima keeps bins 0, 2 and 4, the others are taken back, and a later query whose only candidate is one of the freed
    keypoints found it occupied while the walk ran.  359.9 degrees is bin 12 (factor = 1 / 30 maps [0, 360) onto bins 0..12), and so is a
    difference just below zero; a keyframe angle of 899.9 reaches bin 30, which becomes 0 and is bin 0's third match."""
    s = Scene(name, nf=nf, ori=ori)
    j = 0
    lost = []
    for rot, n in ((0.0, 2), (60.0, 3), (120.0, 3), (180.0, 1), (240.0, 1)):
        for _ in range(n):
            u, v = spot(j); j += 1
            d = new_desc()
            keep = rot < 150 or not ori
            p = s.pt(world(u, v), d, lv=0, angle=rot + 10.0)
            k = s.kp(u, v, 0, at_distance(d, 3), angle=10.0)
            s.want(p, MATCHED if keep else ROTATED_OUT, **(dict(bin=int(rot // 30)) if ori else {})); s.hold(k, p if keep else -1)
            if not keep:
                lost.append((u, v, k))
    for u, v, k in lost:                                                        # later queries on the keypoints that will be freed
        p = s.pt(world(u + 1, v), s.cur.kd[k], lv=0)
        s.want(p, ALL_OCCUPIED)
    for ang_kf, ang_cur, raw, bn in ((359.9, 0.0, 12, 12), (899.9, 0.0, 30, 0), (5.0, 5.0 + 1e-3, 12, 12)):
        u, v = spot(j); j += 1
        d = new_desc()
        p = s.pt(world(u, v), d, lv=0, angle=ang_kf)
        k = s.kp(u, v, 0, d, angle=ang_cur)
        keep = bn == 0 or not ori
        s.want(p, MATCHED if keep else ROTATED_OUT, **(dict(bin=bn, raw_bin=raw) if ori else {})); s.hold(k, p if keep else -1)
    return s.done()


def two_calls():
    """Tracking.cc:2375 and :2391: (10, 100) with sFound given, then (3, 64) with the set rebuilt from what the frame holds.  Point a is 6 px
    and 80 bits from its keypoint: the first call takes it.  Point b is 2 px and 70 bits away: inside both windows, accepted by the first
    call only -- it is held out of the first call by sFound, and the second call, which no longer has it in the set, rejects it at 64.
    Point c (2 px, 60 bits) is in sFound too and matches in the second call.  Point a is not searched again: the frame holds it."""
    s = Scene("two_calls", calls=((10.0, 100, "given"), (3.0, 64, "rebuilt")))
    rows = []
    for n, (off, dd, found) in enumerate(((6, 80, False), (2, 70, True), (2, 60, True))):
        u, v = spot(n)
        d = new_desc()
        p = s.pt(world(u, v), d, lv=0, found=found)
        k = s.kp(u + off, v, 0, at_distance(d, dd))
        rows.append((p, k))
    (a, ka), (b, kb), (c, kc) = rows
    s.want(a, MATCHED, 0); s.want(b, FOUND, 0); s.want(c, FOUND, 0)
    s.want(a, FOUND, 1); s.want(b, TOO_DISTANT, 1, radius=F(3), best_dist=70); s.want(c, MATCHED, 1, best_dist=60)
    s.hold(ka, a); s.hold(kb, -1); s.hold(kc, c)
    return s.done()


def scenes():
    return [skip_rules(), image_bounds(), negative_bounds(), behind_the_camera(), dist_range(), scale_clamps(), window_levels(),
            windows_empty_and_occupied(), overflow(), acceptance_and_ties(), rotation(), rotation(name="rotation_unchecked", ori=False), two_calls(),
            overflow(nf=4096, name="overflow_at_4096"), rotation(nf=4096, name="rotation_at_4096")]


def run_calls(O, PO, sc, fn):
    """every call of the scene in turn through fn (walk or oracle_call): list of results, the assignment carried from call to call"""
    a = sc.assign0.copy()
    out = []
    for c in range(len(sc.calls)):
        r = fn(O, PO, sc, a, c)
        a = r[1]
        out.append(r)
    return out


def describe(gates, infos, i):
    keys = ("u", "v", "dist", "quotient", "level", "radius", "n_window", "best_dist", "best_idx", "bin")
    return "keyframe keypoint %d: %s (%s)" % (i, NAMES[gates[i]], ", ".join("%s %s" % (k, infos[i][k]) for k in keys if k in infos[i]))


def explain(got, exp, gates, infos):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    return "\n".join("keypoint %d holds %d, expected %d; %s" % (k, got[k], exp[k], "; ".join(
        describe(gates, infos, int(i)) for i in sorted(set((int(got[k]), int(exp[k])))) if 0 <= i < len(gates))) for k in bad[:6])


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
CHAIN_SEED = 3
CHAIN_NF = 256


class Chain:
    """Tracking::Relocalization from its first pose on (Tracking.cc:2351-2404) on one lost frame (tests/pose_opt_scenes.py:make_frame: 200
    keypoints that observe known world points, 0.5 px noise) and a keyframe that holds some of those points in shuffled order:
      A  30 points the frame holds on entry (PnP's inliers), plus 3 wrong ones the first optimisation is to flag;
      B   8 points whose keypoint is 5 bits away: the first search (10, 100) finds them;
      W  25 points whose true keypoint is 40 bits away and that have a decoy keypoint 7 px x scale beside it at 10 bits: the first search
         takes the decoy, the optimisation flags it, and the second search (3, 64), whose window no longer reaches the decoy, takes the
         true keypoint.
    So nGood is about 30 after the first optimisation, nadditional + nGood >= 50, nGood lies in (30, 50) after the second one, which is
    what Tracking.cc:2385 asks of a second search, and the last optimisation ends with >= 50 inliers."""

    def __init__(self, seed=CHAIN_SEED, n_entry=30):
        import pose_opt_scenes as PSC
        fr = PSC.make_frame(seed, 200, 200, "mixed", noise=0.5)
        rng = np.random.default_rng(seed + 1000)
        n, nA, nB, nW, nX = fr["n"], 30, 8, 25, 3
        self.fr, self.ori, self.name = fr, True, "chain"
        self.cam = dict(PSC.CAM, nf=CHAIN_NF, scale=PSC.SCALE, bounds=PSC.BOUNDS, b=F(PSC.CAM["bf"] / PSC.CAM["fx"]))
        assert np.array_equal(PSC.SCALE, SCALE)
        perm = rng.permutation(n)
        desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
        Tg = fr["pose_gt"].reshape(3, 4)
        Ow = -Tg[:, :3].T @ Tg[:, 3]
        kps, ur, dep = [fr["kps"]], [fr["uright"]], [fr["depth"]]
        self.points = [None] * n
        self.kf_xw = np.zeros((CHAIN_NF, 3), F)
        dk, dd = np.zeros(nW, KP_DTYPE), []

        def hold(i, pdesc):
            o = int(fr["kps"]["octave"][i])
            maxd = float(np.linalg.norm(fr["xw"][i].astype(D) - Ow)) * 1.2 ** (o - 0.5)
            self.points[perm[i]] = dict(pos=fr["xw"][i], minDist=F(maxd / 3.6), maxDist=F(maxd), desc=pdesc, bad=False)
            self.kf_xw[perm[i]] = fr["xw"][i]
        for i in range(nA + nB):
            hold(i, at_distance(desc[i], 5, shift=int(rng.integers(0, 256))))
        for w, i in enumerate(range(nA + nB, nA + nB + nW)):
            pdesc = rng.integers(0, 256, 32).astype(np.uint8)
            hold(i, pdesc)
            desc[i] = at_distance(pdesc, 40, shift=100)
            dk[w] = fr["kps"][i]
            dk[w]["x"] = fr["kps"]["x"][i] + F(7.0) * SCALE[fr["kps"]["octave"][i]] * (1 if fr["kps"]["x"][i] < 600 else -1)
            dd.append(at_distance(pdesc, 10))
        first_x = nA + nB + nW
        for i in range(first_x, first_x + nX):
            hold(i, rng.integers(0, 256, 32).astype(np.uint8))
        self.rec_cur = dict(kps=np.concatenate(kps + [dk]), desc=np.concatenate([desc, np.array(dd, np.uint8)]),
                            uright=np.concatenate(ur + [np.full(nW, -1, F)]), depth=np.concatenate(dep + [np.full(nW, -1, F)]))
        kk = np.zeros(n, KP_DTYPE); kk["size"] = 31
        self.rec_kf = dict(kps=kk, desc=rng.integers(0, 256, (n, 32)).astype(np.uint8), uright=np.full(n, -1, F), depth=np.full(n, -1, F))
        self.nC = n + nW
        a = np.full(self.nC, -1, np.int32)
        a[:n_entry] = perm[:n_entry]
        for j in range(nX):                                                   # wrong on entry: the point of the next keypoint
            a[first_x + j] = perm[first_x + (j + 1) % nX]
        self.assign0 = a
        self.pose_in = fr["pose_in"].copy()
        self.INV_SIGMA2 = PSC.INV_SIGMA2

    def optimise(self, PR, assign, pose):
        """Optimizer::PoseOptimization on what the frame holds (tests/pose_opt_ref.py): (result, xw, has_point)"""
        has = (assign >= 0).astype(np.uint8)
        xw = np.where(has[:, None] != 0, self.kf_xw[np.maximum(assign, 0)], 0).astype(F)
        c = self.cam
        r = PR.pose_optimization(self.rec_cur["kps"], self.nC, self.rec_cur["uright"], self.INV_SIGMA2, c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], xw, has,
                                 None, 4, np.asarray(pose, F).reshape(12))
        return r, xw, has


def chain_reference(O, PO, PR, ch):
    """the steps of Tracking.cc:2351-2404 through the oracle and tests/pose_opt_ref.py alone: a dict of every intermediate"""
    out = {}
    a = ch.assign0.copy()
    found = set(int(v) for v in a if v >= 0)                                    # :2351-2361
    r1, _, _ = ch.optimise(PR, a, ch.pose_in)                                   # :2363
    a[r1["outlier"][:ch.nC] != 0] = -1                                          # :2368-2370
    out.update(nGood1=int(r1["ninliers"]), pose1=r1["pose"], assign1=a.copy())
    nadd, a = oracle_search(O, PO, ch, a, r1["pose"], found, 10.0, 100)         # :2375
    out.update(nadd1=nadd, search1=a.copy())
    r2, _, _ = ch.optimise(PR, a, r1["pose"])                                   # :2379
    a[r2["outlier"][:ch.nC] != 0] = -1
    out.update(nGood2=int(r2["ninliers"]), pose2=r2["pose"], assign2=a.copy())
    nadd, a = oracle_search(O, PO, ch, a, r2["pose"], set(int(v) for v in a if v >= 0), 3.0, 64)   # :2386-2391
    out.update(nadd2=nadd, search2=a.copy())
    r3, _, _ = ch.optimise(PR, a, r2["pose"])                                   # :2395
    a[r3["outlier"][:ch.nC] != 0] = -1                                          # :2398-2400
    out.update(nGood3=int(r3["ninliers"]), pose3=r3["pose"], assign3=a)
    return out
