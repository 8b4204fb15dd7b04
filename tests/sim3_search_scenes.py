"""sim3_search_scenes.py -- the hand-made scenes of the two batched loop-closing searches (test infrastructure only), shared by
tests/test_sim3_search_cpu.py (the restatement tests/sim3_search_ref.py against these expectations) and tests/test_gpu_sim3_search.py
(ivf_tracker_search_by_sim3 / ivf_tracker_search_by_bow_keyframes against the restatement).

EXACT scenes: identity poses, s = 1, R = I, t = 0, a camera with fx = fy = 512 and integral cx, cy, every point at z = 1 or on the optical
axis, so the restatement's u, v and dist3D are the intended floats bit for bit (`exact` lists them; the CPU module asserts it) and every
comparison of the search sits ON its boundary, with a neighbour one step on the other side.  Each states by hand what must come out
(`expect`: vnMatch1, vnMatch2, vpMatches12, nFound; everything not named is -1).
GENERIC scenes: the planted similarity of the chain test of tests/test_gpu_sim3.py on the camera and poses of tests/sim3_scenes.py; the CPU
module keeps every gate quantity of them away from its threshold.
BOW scenes: built with the Builder of tests/track_bow_scenes.py on its depth-3 tree, with points on both sides.

A sim3 scene is dict(name, cam, nf, kf1, kf2, sim3 [16], match12 [nf], inlier [nf] or None, th); nf = sim3_scenes.NF = 128, except for the
window of 130 candidates, which needs a record of more than 128 keypoints (256)."""
import numpy as np

import sim3_scenes as S
import track_bow_scenes as TB
from create_points_ref import LOCAL_POINT_DTYPE

F, D = np.float32, np.float64
NF = S.NF
KP_DTYPE = S.KP_DTYPE
EXACT_CAM = dict(fx=F(512.0), fy=F(512.0), cx=F(600.0), cy=F(180.0), bf=F(386.1448), bounds=S.BOUNDS, scale=S.SCALE)
GENERIC_CAM = dict(S.CAM, bounds=S.BOUNDS, scale=S.SCALE)
IDENT_POSE = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
IDENT_SIM3 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)
TH = 7.5


def flip(d, bits):
    d = np.array(d, np.uint8)
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


class Exact:
    """two keyframes of one exact scene; side 0 = KF1, side 1 = KF2"""

    def __init__(self, name, seed, nf=NF):
        self.name, self.nf, self.rng = name, nf, np.random.default_rng(seed)
        self.kps = ([], []); self.pts = ([], [])
        self.match12 = {}; self.inlier = {}
        self.expect = dict(match1={}, match2={}, matches={}, nfound=0)
        self.exact = []                                                       # (side, keypoint, field, intended float)
        self.stage = []                                                       # (side, keypoint, stage name of sim3_search_ref)

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def kp(self, side, x, y, octave=0, desc=None):
        self.kps[side].append((F(x), F(y), int(octave), self.desc() if desc is None else np.array(desc, np.uint8)))
        self.pts[side].append(None)
        return len(self.kps[side]) - 1

    def point(self, side, i, u=None, v=None, level=0, desc=None, pos=None, min_d=None, max_d=None, bad=False):
        """the point keypoint i of `side` holds: at z = 1 behind pixel (u, v) of the OTHER keyframe (or at pos), its max_distance chosen so
        that PredictScale gives `level` with half a level to spare (level 0: ratio 1 exactly)"""
        c = EXACT_CAM
        if pos is None:
            pos = ((D(u) - D(c["cx"])) / D(c["fx"]), (D(v) - D(c["cy"])) / D(c["fy"]), 1.0)
            assert all(D(F(x)) == x for x in pos), "%s: (%r, %r) is no exact pixel of this camera" % (self.name, u, v)
            self.exact += [(side, i, "u", F(u)), (side, i, "v", F(v))]
        pos = np.array(pos, F)
        dist = F(np.sqrt(D(pos[0]) ** 2 + D(pos[1]) ** 2 + D(pos[2]) ** 2))
        if max_d is None:
            max_d = dist if level == 0 else F(D(dist) * 1.2 ** (level - 0.5))
        if min_d is None:
            min_d = F(0.5) * dist
        self.pts[side][i] = dict(pos=pos, min_d=F(min_d), max_d=F(max_d), desc=self.desc() if desc is None else np.array(desc, np.uint8), bad=bad)
        return dist

    def pair(self, at1, at2, proj12=None, proj21=None, d12=0, d21=0, oct1=0, oct2=0, level12=0, level21=0, **kw12):
        """keypoint i of KF1 at at1 whose point projects to proj12 (default: at2) in KF2, keypoint j of KF2 at at2 whose point projects to
        proj21 (default: at1) in KF1; the point's descriptor is d12 / d21 bits from the keypoint's it is meant to find -> (i, j)"""
        d, e = self.desc(), self.desc()
        i = self.kp(0, at1[0], at1[1], oct1, flip(e, range(d21)))
        j = self.kp(1, at2[0], at2[1], oct2, flip(d, range(d12)))
        p12 = at2 if proj12 is None else proj12; p21 = at1 if proj21 is None else proj21
        self.point(0, i, p12[0], p12[1], level12, d, **kw12)
        self.point(1, j, p21[0], p21[1], level21, e)
        return i, j

    def agreed(self, i, j):
        self.expect["match1"][i] = j; self.expect["match2"][j] = i; self.expect["matches"][i] = j; self.expect["nfound"] += 1

    def side(self, s):
        n = len(self.kps[s])
        assert n <= self.nf, (self.name, n)
        kp = np.zeros(n, KP_DTYPE); desc = np.zeros((n, 32), np.uint8); pts = np.zeros(n, LOCAL_POINT_DTYPE)
        kp["size"] = 31
        for i, (x, y, o, d) in enumerate(self.kps[s]):
            kp["x"][i], kp["y"][i], kp["octave"][i] = x, y, o
            desc[i] = d
            p = self.pts[s][i]
            if p is None:
                pts["flags"][i] = 1; pts["max_distance"][i] = 1.0; pts["min_distance"][i] = 1.0
            else:
                pts["pos"][i] = p["pos"]; pts["min_distance"][i] = p["min_d"]; pts["max_distance"][i] = p["max_d"]; pts["desc"][i] = p["desc"]
                pts["flags"][i] = 1 if p["bad"] else 0
        return dict(n=n, kps=kp, desc=desc, pose=IDENT_POSE.copy(), points=pts)

    def scene(self):
        m12 = np.full(self.nf, -1, np.int32); inl = np.ones(self.nf, np.uint8)
        for i, m in self.match12.items():
            m12[i] = m
        for i, f in self.inlier.items():
            inl[i] = f
        ex = dict(self.expect)
        for i, m in self.match12.items():                                     # a kept input entry stays in vpMatches12
            if inl[i] and m >= 0:
                ex["matches"].setdefault(i, m)
        return dict(name=self.name, cam=EXACT_CAM, nf=self.nf, kf1=self.side(0), kf2=self.side(1), sim3=IDENT_SIM3.copy(), match12=m12,
                    inlier=inl if self.inlier else None, th=TH, expect=ex, exact=self.exact, stage=self.stage, kind="exact")


def exact_scenes():
    out = []
    W, H = S.W, S.H
    # ---- KeyFrame::IsInImage: u == minX is kept, u == maxX is dropped; the same for v
    b = Exact("image_edges", 1)
    i, j = b.pair((100, 100), (2, 50), proj12=(0, 50)); b.agreed(i, j)
    i, j = b.pair((200, 100), (W - 2, 60), proj12=(W, 60)); b.expect["match2"][j] = i; b.stage.append((0, i, "outside the image"))
    i, j = b.pair((300, 100), (700, 2), proj12=(700, 0)); b.agreed(i, j)
    i, j = b.pair((400, 100), (800, H - 2), proj12=(800, H)); b.expect["match2"][j] = i; b.stage.append((0, i, "outside the image"))
    i, j = b.pair((2, 200), (500, 200), proj21=(0, 200)); b.agreed(i, j)                                 # the mirror image: KF2's point into KF1
    i, j = b.pair((W - 2, 250), (600, 250), proj21=(W, 250)); b.expect["match1"][i] = j; b.stage.append((1, j, "outside the image"))
    out.append(b.scene())
    # ---- z == 0 and z == -0.0 go on and fail the image test, a small negative z is skipped
    b = Exact("depth_sign", 2)
    for k, (xy, z, st) in enumerate(((0.125, 0.0, "outside the image"), (-0.125, -0.0, "outside the image"), (0.125, -1e-3, "z < 0"))):
        i, j = b.pair((100 + 50 * k, 100), (600 + 50 * k, 180), pos=(xy, xy, z), min_d=0.01, max_d=10.0)
        b.expect["match2"][j] = i; b.stage.append((0, i, st))
    i, j = b.pair((400, 100), (600, 300)); b.agreed(i, j)
    sc = b.scene()
    sc["kf1"]["pose"][11] = -0.0                                              # a sum keeps -0.0 only when every addend is -0.0: t1w and t21 = -(0) are
    out.append(sc)
    # ---- dist3D == each end of [0.8f min_distance, 1.2f max_distance] is kept, one float outside is dropped; points on the optical axis
    b = Exact("range_ends", 3)
    near = F(F(0.8) * F(2.5)); far = F(F(1.2) * F(2.5))
    cases = ((near, 2.5, near, None), (np.nextafter(near, F(0)), 2.5, near, "too near"), (far, 1.0, 2.5, None), (np.nextafter(far, F(10)), 1.0, 2.5, "too far"))
    for k, (z, mn, mx, st) in enumerate(cases):
        i, j = b.pair((100 + 60 * k, 300), (600, 180), pos=(0.0, 0.0, z), min_d=mn, max_d=mx)
        # the four keypoints of KF2 share one pixel: each query finds its own descriptor at distance 0, the first minimum
        b.exact += [(0, i, "u", F(600)), (0, i, "v", F(180)), (0, i, "dist", F(z))]
        if st is None:
            b.agreed(i, j)
        else:
            b.expect["match2"][j] = i; b.stage.append((0, i, st))
    out.append(b.scene())
    # ---- the window: a keypoint at exactly r = 7.5 from the projection is excluded, one at 7.25 is not; both axes
    b = Exact("radius_edge", 4)
    i, j = b.pair((100, 100), (307.5, 100), proj12=(300, 100)); b.expect["match2"][j] = i; b.stage.append((0, i, "searched"))
    i, j = b.pair((200, 100), (407.25, 100), proj12=(400, 100)); b.agreed(i, j)
    i, j = b.pair((300, 100), (500, 207.5), proj12=(500, 200)); b.expect["match2"][j] = i
    i, j = b.pair((400, 100), (700, 192.75), proj12=(700, 200)); b.agreed(i, j)
    out.append(b.scene())
    # ---- octaves level - 2 .. level + 1 at level 2: only level - 1 and level are compared, whatever the others' distances
    b = Exact("octaves", 5)
    d, e = b.desc(), b.desc()
    i = b.kp(0, 100, 100, 0, e)
    b.point(0, i, 600, 100, level=2, desc=d)
    js = [b.kp(1, 598 + 1.5 * k, 100, o, flip(d, range(nb))) for k, (o, nb) in enumerate(((0, 0), (3, 1), (2, 6), (1, 5)))]
    b.point(1, js[3], 100, 100, desc=e)
    b.agreed(i, js[3])
    out.append(b.scene())
    # ---- TH_HIGH: 100 is accepted, 101 is not; in both directions
    b = Exact("th_high", 6)
    i, j = b.pair((100, 100), (600, 100), d12=100, d21=100); b.agreed(i, j)
    i, j = b.pair((200, 100), (700, 100), d12=101); b.expect["match2"][j] = i
    i, j = b.pair((300, 100), (800, 100), d21=101); b.expect["match1"][i] = j
    out.append(b.scene())
    # ---- equal distances: the first in WINDOW order wins (grid column 25 before 26), not the lower index
    b = Exact("equal_distances", 7)
    d, e = b.desc(), b.desc()
    i = b.kp(0, 100, 100, 0, e)
    b.point(0, i, 497, 300, desc=d)
    j_late = b.kp(1, 500.5, 300, 0, flip(d, range(10)))                       # column 26, the lower index
    j_first = b.kp(1, 494, 300, 0, flip(d, range(10, 20)))                    # column 25
    b.point(1, j_first, 100, 100, desc=e)
    b.agreed(i, j_first)
    out.append(b.scene())
    # ---- the agreement check, the already-matched sets, the inlier filter, a bad point, a match past KF2's count
    b = Exact("bookkeeping", 8)
    i, j = b.pair((100, 100), (600, 100), proj21=(900, 300)); b.expect["match1"][i] = j        # 2 -> 1 finds nothing: no agreement
    i, j = b.pair((150, 100), (650, 100)); b.match12[i] = j                                    # already matched on both sides: neither is searched
    b.stage += [(0, i, "already matched"), (1, j, "already matched")]
    i, j = b.pair((200, 100), (700, 100)); b.match12[i] = 0; b.inlier[i] = 0; b.agreed(i, j)   # dropped by its flag: both keypoints are free
    i, j = b.pair((250, 100), (750, 100)); b.pts[0][i]["bad"] = True; b.expect["match2"][j] = i
    b.stage.append((0, i, "no point / bad"))
    past = b.pair((300, 100), (800, 100))
    far_past = b.pair((350, 100), (850, 100))
    sc_n2 = len(b.kps[1])
    b.match12[past[0]] = sc_n2; b.expect["match2"][past[1]] = past[0]                          # one past KF2's count: KF1's side is matched, nothing in KF2
    b.match12[far_past[0]] = 100000; b.expect["match2"][far_past[1]] = far_past[0]
    out.append(b.scene())
    # ---- a window of 65 and of 130 candidates in one grid column: more than one, more than two steps of the wave
    for name, nc, nf in (("window_65", 65, NF), ("window_130", 130, 256)):
        b = Exact(name, 9 + nc, nf)
        d, e = b.desc(), b.desc()
        i = b.kp(0, 100, 100, 0, e)
        b.point(0, i, 620, 188, desc=d)
        js = []
        for k in range(nc):                                                   # rows ascend with the index: window order is index order
            nb = 40 + k % 7
            o = 0
            if k == 5:
                nb, o = 0, 1                                                  # the best descriptor, at an octave the level excludes
            if k in (nc - 1, nc - 3):
                nb = 3                                                        # two equal minima behind the first step(s): the earlier wins
            js.append(b.kp(1, 616 + (k % 8), 184 + 0.0625 * (k // 8) * 8, o, flip(d, range(k % 5, k % 5 + nb))))
        b.point(1, js[nc - 3], 100, 100, desc=e)
        b.agreed(i, js[nc - 3])
        out.append(b.scene())
    # ---- a record with no keypoints on either side, and one with exactly nfeatures
    for name, empty in (("empty_kf1", 0), ("empty_kf2", 1)):
        b = Exact(name, 20 + empty)
        i, j = b.pair((100, 100), (600, 100))
        b.kps[empty].clear(); b.pts[empty].clear()
        b.exact = [x for x in b.exact if x[0] != empty]
        out.append(b.scene())
    b = Exact("full_records", 22)
    for k in range(NF):
        i, j = b.pair((20 + 9 * k, 40 + 17 * (k % 16)), (1200 - 9 * k, 330 - 17 * (k % 16)))
        b.agreed(i, j)
    out.append(b.scene())
    return out


def generic_scene(name, seed, n=60, s12=1.2, prematch=None, outlier_every=0):
    """the planted similarity of the chain test: n points seen by both keyframes, KF1 keypoint i1 <-> KF2 keypoint perm[i1]; prematch:
    keep every prematch-th correspondence out of match12 (None: match12 is empty); outlier_every: the inlier flag of every such match is 0"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (D(S.CAM[k]) for k in ("fx", "fy", "cx", "cy"))
    R12 = S.PS.rot((0.1, 1.0, 0.3), 2.0); t12 = np.array([0.3, 0.1, -0.4])
    u = rng.uniform(80, S.W - 80, n); v = rng.uniform(60, S.H - 60, n); z = rng.uniform(5, 18, n)
    X1 = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    X2 = (X1 - t12) @ R12 / s12
    perm = rng.permutation(n)
    proj = lambda X: np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    lv = rng.integers(0, 4, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    (R1, t1), (R2, t2) = S.POSE1, S.POSE2
    kfs = []
    for side, (X, Xother, Rw, tw, slot) in enumerate(((X1, X2, R1, t1, np.arange(n)), (X2, X1, R2, t2, perm))):
        kp = np.zeros(n, KP_DTYPE); kp["size"] = 31
        p = proj(X).astype(F)
        kp["x"][slot] = p[:, 0]; kp["y"][slot] = p[:, 1]; kp["octave"][slot] = lv
        pts = np.zeros(n, LOCAL_POINT_DTYPE)
        pts["pos"][slot] = ((X - tw) @ Rw).astype(F)
        dist = np.linalg.norm(Xother, axis=1)                                 # what the search measures: the norm in the OTHER camera
        pts["max_distance"][slot] = (dist * 1.2 ** (lv - 0.5)).astype(F)       # level lv with half a level to spare
        pts["min_distance"][slot] = (0.5 * dist).astype(F)
        d = np.zeros((n, 32), np.uint8); d[slot] = desc
        pts["desc"] = d
        kfs.append(dict(n=n, kps=kp, desc=d, pose=S.pose12(Rw, tw), points=pts))
    sim3 = np.zeros(16, F); sim3[:9] = R12.reshape(9); sim3[9:12] = t12; sim3[12] = s12
    m12 = np.full(NF, -1, np.int32); inl = None
    if prematch:
        known = np.arange(n) % prematch != 0
        m12[:n][known] = perm[known]
        if outlier_every:
            inl = np.ones(NF, np.uint8); inl[np.nonzero(known)[0][::outlier_every]] = 0
    want = np.full(NF, -1, np.int32); want[:n] = perm
    return dict(name=name, cam=GENERIC_CAM, nf=NF, kf1=kfs[0], kf2=kfs[1], sim3=sim3, match12=m12, inlier=inl, th=TH, kind="generic", perm=perm,
                expect_matches=want)


def generic_scenes():
    # the seeds: the first from 31 on at which every gate of the scene stands 0.02 px / 0.1 m or more from its threshold (the CPU module's
    # bound, 64 x the f32 - f64 spread, is 0.009 px and 2e-4 m)
    return [generic_scene("planted", 73), generic_scene("planted_prematched", 34, prematch=3), generic_scene("planted_filtered", 53, prematch=3, outlier_every=4),
            generic_scene("planted_s1", 73, s12=1.0)]


def sim3_scenes():
    return {s["name"]: s for s in exact_scenes() + generic_scenes()}


# ---- SearchByBoW(KF, KF) --------------------------------------------------------------------------------------------------------------
NF_BOW = TB.NF                                                               # 256: a node of 130 features needs more than 128 keypoints
NN_RATIO = 0.75


def _bow_scene(b, name, no_point2=()):
    sc = b.scene(name, b.tree["depth"] - 2)
    has2 = np.ones(len(sc["f"]["kps"]), np.uint8); has2[list(no_point2)] = 0
    kf = lambda s, has: dict(n=len(s["kps"]), kps=s["kps"], desc=s["desc"], has=has)
    return dict(name=name, tree=b.tree, levelsup=sc["levelsup"], kf1=kf(sc["kf"], sc["kf"]["has"]), kf2=kf(sc["f"], has2), nf=NF_BOW)


def bow_scenes():
    tree = TB.TREES[3]
    out = []
    b = TB.Builder(tree, 41)
    b.add_kf([2], b.payload())                                                # node 0 on KF1's side only
    b.good(b.node(), 12)
    nd = b.node(); b.add_f(nd, b.payload())                                   # a node on KF2's side only
    nd = b.node(); p = b.payload(); b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(49)))      # bestDist1 = 49: accepted
    nd = b.node(); p = b.payload(); b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(50)))      # 50: not < TH_LOW
    nd = b.node(); p = b.payload()                                            # the ratio on its edge: 21 < 0.75 * 29 = 21.75
    b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(29))); b.add_f(nd, b.flipped(p, b.pick(21)))
    nd = b.node(); p = b.payload()                                            # 21 < 0.75 * 28 = 21 is false
    b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(21))); b.add_f(nd, b.flipped(p, b.pick(28)))
    nd = b.node(); p = b.payload()                                            # the twin in KF2 holds no point: the other candidate is taken
    b.add_kf(nd, p); dead = b.add_f(nd, b.flipped(p, b.pick(2))); b.add_f(nd, b.flipped(p, b.pick(10)))
    nd = b.node(); p = b.payload()                                            # two KF1 features want one KF2 feature: the second takes its next best
    x = b.pick(2); y = b.pick(1, avoid=x); z = b.pick(30, avoid=x + y)
    b.add_kf(nd, p); b.add_kf(nd, b.flipped(p, x)); b.add_f(nd, b.flipped(p, x + z)); b.add_f(nd, b.flipped(p, y))
    nd = b.node(); p = b.payload()                                            # ... or finds every candidate matched
    b.add_kf(nd, p); b.add_kf(nd, b.flipped(p, b.pick(2))); b.add_f(nd, b.flipped(p, b.pick(1)))
    nd = b.node(); p = b.payload(); q = b.payload()                           # a KF1 feature without a point: its twin stays free
    b.add_kf(nd, p, has=0); b.add_kf(nd, q); b.add_f(nd, p); b.add_f(nd, b.flipped(q, b.pick(4)))
    nd = b.node(); p = b.payload()                                            # a match alone in its rotation bin (rot = 150): removed
    b.add_kf(nd, p, angle=200.0); b.add_f(nd, b.flipped(p, b.pick(2)), angle=50.0)
    b.add_kf(b.nodes[-1], b.payload())
    out.append(_bow_scene(b, "bow_gates", no_point2=[dead]))
    # nodes of 1, 64, 65 and 130 features on either side
    for name, sizes, seed in (("bow_wide_kf2", ((1, 64), (65, 130)), 42), ("bow_wide_kf1", ((64, 1), (130, 65)), 43)):
        b = TB.Builder(tree, seed)
        dead = []
        for n1, n2 in sizes:
            nd = b.node()
            ps = [b.payload() for _ in range(n1)]
            fill = [b.payload() for _ in range(n2)]
            for k, j in enumerate(sorted(set((0, n1 - 1, n1 // 2, min(63, n1 - 1), min(64, n1 - 1))))):   # twins at both ends of KF2's run
                fill[(n2 - 1 - 37 * k) % n2] = b.flipped(ps[j], b.pick(3 + k))
            for p in ps:
                b.add_kf(nd, p)
            base = len(b.f)
            for p in fill:
                b.add_f(nd, p)
            if n2 > 2:
                dead.append(base + 1)
        out.append(_bow_scene(b, name, no_point2=dead))
    b = TB.Builder(tree, 44)                                                  # three rotation bins kept, the fourth and fifth removed
    for k, (rot, count) in enumerate(((10.0, 12), (120.0, 8), (250.0, 5), (330.0, 3), (60.0, 1))):
        nd = b.nodes[k]
        for j in range(count):
            p = b.payload(); fa = 40.0 + j if j % 2 else 300.0 - j; ka = fa + rot
            b.add_kf(nd, p, angle=ka - 360.0 if ka >= 360.0 else ka); b.add_f(nd, b.flipped(p, b.pick(2)), angle=fa)
    out.append(_bow_scene(b, "bow_rotation"))
    for which in ("kf1", "kf2"):
        b = TB.Builder(tree, 45); b.good(b.node(), 3)
        if which == "kf1":
            b.kf = []
        else:
            b.f = []
        out.append(_bow_scene(b, "bow_empty_" + which))
    return {s["name"]: s for s in out}
