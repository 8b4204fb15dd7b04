"""projection_ref.py -- plain-Python restatement, END TO END, of the two projection searches of a tracked frame (test infrastructure only):

  Tracking::SearchLocalPoints' matcher part: Frame::isInFrustum (ORB/src/Frame.cc:557-613), MapPoint::PredictScale (MapPoint.cc:407-422),
  ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th) (ORBmatcher.cc:45-135), RadiusByViewingCos (:137-143);
  Tracking::TrackWithMotionModel's matcher part: UpdateLastFrame's points (Tracking.cc:1256-1300), Frame::UnprojectStereo (Frame.cc:958-972),
  ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, false) (ORBmatcher.cc:1372-1518), the retry (Tracking.cc:1320-1330);
  Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea (Frame.cc:415-430, :615-680) and glibc's logf for both.

Nothing here calls the C oracle.  The float / double mix is the one frozen in DESIGN.md A-11 (cv::gemm on CV_32F: double accumulation, one
narrowing; norm and dot in double) and A-12 (PredictScale through logf and a float quotient).  Besides the assignment every search says, per
query, WHERE the query left the loop (an outcome code) and the intermediates it had on the way: the scenes of tests/projection_scenes.py are
built to stand on both sides of every comparison, and tests/test_projection_scenes_cpu.py checks through these codes that they still do."""
import math

import numpy as np

F = np.float32
D = np.float64
TH_HIGH, HISTO_LENGTH = 100, 30
GRID_COLS, GRID_ROWS = 64, 48

# outcome of one local map point (SearchLocalPoints)
SKIPPED, BEHIND, OUT_OF_IMAGE, TOO_NEAR, TOO_FAR, VIEW_ANGLE, EMPTY_WINDOW, ALL_BLOCKED, OVER_TH_HIGH, RATIO_FAILED, ACCEPTED, ACCEPTED_THEN_REPLACED = range(12)
LOCAL_NAMES = ["skipped", "behind the camera", "out of the image", "too near", "too far", "viewing angle", "empty window", "every candidate blocked",
               "over TH_HIGH", "ratio failed", "accepted", "accepted, then replaced"]
# outcome of one last-frame keypoint (TrackWithMotionModel); the last three share their codes' meaning with the local search
NO_DEPTH, FLAG_OFF, BEYOND_CLOSE_RULE, M_BEHIND, M_OUT_OF_IMAGE, M_EMPTY_WINDOW, ALL_REFUSED, M_OVER_TH_HIGH, M_ACCEPTED, M_ACCEPTED_THEN_REPLACED, ROT_REMOVED = range(11)
MOTION_NAMES = ["no depth", "flag off", "beyond the close-point rule", "behind the camera", "out of the image", "empty window", "every candidate refused",
                "over TH_HIGH", "accepted", "accepted, then replaced", "accepted, removed by the rotation filter"]

H = float.fromhex
_LOGF_T = [(H("0x1.661ec79f8f3bep+0"), H("-0x1.57bf7808caadep-2")), (H("0x1.571ed4aaf883dp+0"), H("-0x1.2bef0a7c06ddbp-2")), (H("0x1.49539f0f010bp+0"), H("-0x1.01eae7f513a67p-2")),
           (H("0x1.3c995b0b80385p+0"), H("-0x1.b31d8a68224e9p-3")), (H("0x1.30d190c8864a5p+0"), H("-0x1.6574f0ac07758p-3")), (H("0x1.25e227b0b8eap+0"), H("-0x1.1aa2bc79c81p-3")),
           (H("0x1.1bb4a4a1a343fp+0"), H("-0x1.a4e76ce8c0e5ep-4")), (H("0x1.12358f08ae5bap+0"), H("-0x1.1973c5a611cccp-4")), (H("0x1.0953f419900a7p+0"), H("-0x1.252f438e10c1ep-5")),
           (H("0x1p+0"), H("0x0p+0")), (H("0x1.e608cfd9a47acp-1"), H("0x1.aa5aa5df25984p-5")), (H("0x1.ca4b31f026aap-1"), H("0x1.c5e53aa362eb4p-4")),
           (H("0x1.b2036576afce6p-1"), H("0x1.526e57720db08p-3")), (H("0x1.9c2d163a1aa2dp-1"), H("0x1.bc2860d22477p-3")), (H("0x1.886e6037841edp-1"), H("0x1.1058bc8a07ee1p-2")),
           (H("0x1.767dcf5534862p-1"), H("0x1.4043057b6ee09p-2"))]


def logf(x):
    """glibc >= 2.27 logf (sysdeps/ieee754/flt-32/e_logf.c) for a positive normal float: table of 1/c and log c, degree-3 polynomial in
    double, one narrowing.  Python's floats are the doubles of the C text."""
    ix = int(np.array(x, F).view(np.uint32))
    assert 0x00800000 <= ix < 0x7f800000
    if ix == 0x3f800000:
        return F(0.0)
    tmp = (ix - 0x3f330000) & 0xffffffff
    i = (tmp >> 19) & 15
    k = (tmp >> 23) - (512 if tmp & 0x80000000 else 0)                              # (int32_t) tmp >> 23
    iz = (ix - (tmp & 0xff800000)) & 0xffffffff
    z = float(np.array(iz, np.uint32).view(F))
    invc, logc = _LOGF_T[i]
    r = z * invc - 1.0
    y0 = logc + float(k) * H("0x1.62e42fefa39efp-1")
    r2 = r * r
    y = H("0x1.5575b0be00b6ap-2") * r + H("-0x1.ffffef20a4123p-2")
    y = H("-0x1.00ea348b88334p-2") * r2 + y
    y = y * r2 + (y0 + r)
    return F(y)


def scale_table(nlevels=8, sf=1.2):
    """mvScaleFactor (ORBextractor.cc:419-425): scaleFactor is the double of the float 1.2"""
    s = [F(1.0)]
    for _ in range(1, nlevels):
        s.append(F(D(s[-1]) * D(F(sf))))
    return np.array(s, F)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def c_round(x):
    """roundf: halves away from zero"""
    x = float(x)
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def mul_add(R, p, t):
    R = np.asarray(R, D); p = np.asarray(p, D); t = np.asarray(t, D)
    return np.array([R[i, 0] * p[0] + R[i, 1] * p[1] + R[i, 2] * p[2] + t[i] for i in range(3)], D).astype(F)


def neg_rt_mul(R, t):
    R = np.asarray(R, D); t = np.asarray(t, D)
    return np.array([-(R[0, j] * t[0] + R[1, j] * t[1] + R[2, j] * t[2]) for j in range(3)], D).astype(F)


# ---- the frame grid -------------------------------------------------------------------------------------------------------------
def grid_inv(bounds):
    return F(F(GRID_COLS) / F(F(bounds[2]) - F(bounds[0]))), F(F(GRID_ROWS) / F(F(bounds[3]) - F(bounds[1])))


def cell_of(x, y, bounds):
    """Frame::PosInGrid (Frame.cc:670-680): (posX, posY) or None"""
    iw, ih = grid_inv(bounds)
    px = c_round(F(F(F(x) - F(bounds[0])) * iw)); py = c_round(F(F(F(y) - F(bounds[1])) * ih))
    if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:
        return None
    return px, py


def build_grid(kps, bounds):
    grid = {}
    for i in range(len(kps)):
        c = cell_of(kps["x"][i], kps["y"][i], bounds)
        if c is not None:
            grid.setdefault(c, []).append(i)
    return grid


def features_in_area(grid, kps, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (Frame.cc:615-668): ix in the outer loop, iy in the inner one, insertion order inside a cell"""
    iw, ih = grid_inv(bounds)
    x = F(x); y = F(y); r = F(r); minx = F(bounds[0]); miny = F(bounds[1])
    x0 = max(0, int(math.floor(F(F(F(x - minx) - r) * iw))))
    if x0 >= GRID_COLS:
        return []
    x1 = min(GRID_COLS - 1, int(math.ceil(F(F(F(x - minx) + r) * iw))))
    if x1 < 0:
        return []
    y0 = max(0, int(math.floor(F(F(F(y - miny) - r) * ih))))
    if y0 >= GRID_ROWS:
        return []
    y1 = min(GRID_ROWS - 1, int(math.ceil(F(F(F(y - miny) + r) * ih))))
    if y1 < 0:
        return []
    check = min_level > 0 or max_level >= 0
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for i in grid.get((ix, iy), ()):
                o = int(kps["octave"][i])
                if check:
                    if o < min_level:
                        continue
                    if max_level >= 0 and o > max_level:
                        continue
                if abs(F(F(kps["x"][i]) - x)) < r and abs(F(F(kps["y"][i]) - y)) < r:
                    out.append(i)
    return out


def project(cam, xc, invz):
    """u = fx * xc * invz + cx, left to right in float"""
    u = F(F(F(F(cam["fx"]) * xc[0]) * invz) + F(cam["cx"])); v = F(F(F(F(cam["fy"]) * xc[1]) * invz) + F(cam["cy"]))
    return u, v


def outside(cam, u, v):
    b = [F(x) for x in cam["bounds"]]
    return bool(u < b[0] or u > b[2] or v < b[1] or v > b[3])


# ---- SearchLocalPoints ----------------------------------------------------------------------------------------------------------
def predict_scale(cam, max_dist, dist):
    ratio = F(F(max_dist) / F(dist))
    q = F(logf(ratio) / logf(cam["scale"][1]))                                     # mfLogScaleFactor = log(mfScaleFactor): logf (Frame.cc:106)
    n = int(math.ceil(float(q)))
    return min(max(n, 0), len(cam["scale"]) - 1)


def frustum(cam, T, p, cos_limit):
    """Frame::isInFrustum: (outcome or None, dict of what it computed)"""
    R, t = T[:3, :3], T[:3, 3]
    P = np.asarray(p["pos"], F)
    Pc = mul_add(R, P, t)
    info = dict(pcz=Pc[2])
    if Pc[2] < F(0.0):
        return BEHIND, info
    with np.errstate(all="ignore"):
        invz = F(F(1.0) / Pc[2])
        u, v = project(cam, Pc, invz)
    info.update(u=u, v=v)
    if outside(cam, u, v):
        return OUT_OF_IMAGE, info
    PO = (P - neg_rt_mul(R, t)).astype(F)
    dist = F(math.sqrt(float(D(PO[0]) * D(PO[0]) + D(PO[1]) * D(PO[1]) + D(PO[2]) * D(PO[2]))))
    info.update(dist=dist)
    if dist < F(F(0.8) * F(p["minDist"])):
        return TOO_NEAR, info
    if dist > F(F(1.2) * F(p["maxDist"])):
        return TOO_FAR, info
    n = np.asarray(p["normal"], F)
    view_cos = F(float(D(PO[0]) * D(n[0]) + D(PO[1]) * D(n[1]) + D(PO[2]) * D(n[2])) / float(dist))
    info.update(view_cos=view_cos)
    if view_cos < F(cos_limit):
        return VIEW_ANGLE, info
    info.update(level=predict_scale(cam, p["maxDist"], dist), ur=F(u - F(F(cam["bf"]) * invz)))
    return None, info


def search_local(cam, cur, T, points, occupied, th, nn_ratio, cos_limit=0.5):
    """-> (nmatches, per current keypoint the point it received in this call or -1, outcome per point, info per point).
    cur: dict(kps, desc, uright); points: dict(pos, normal, minDist, maxDist, desc, skip, nObs) in list order; occupied: per keypoint,
    True = holds a map point with observations before the call."""
    kps = cur["kps"]; n = len(kps)
    grid = build_grid(kps, cam["bounds"])
    state = [(-2, True) if (occupied is not None and occupied[i]) else None for i in range(n)]      # (point, blocks)
    outcome = np.zeros(len(points), np.int32)
    infos = []
    nm = 0
    th = F(th); nn = F(nn_ratio)
    for k, p in enumerate(points):
        if p["skip"]:
            outcome[k] = SKIPPED; infos.append({}); continue
        oc, info = frustum(cam, T, p, cos_limit)
        infos.append(info)
        if oc is not None:
            outcome[k] = oc; continue
        r = F(2.5) if float(info["view_cos"]) > 0.998 else F(4.0)                   # a float against the double 0.998 (:139)
        if float(th) != 1.0:
            r = F(r * th)
        lv = info["level"]
        radius = F(r * F(cam["scale"][lv]))
        info["radius"] = radius
        cand = features_in_area(grid, kps, cam["bounds"], info["u"], info["v"], radius, lv - 1, lv)
        info.update(n_window=len(cand), n_admitted=0, best_dist=256, best_dist2=256, best_level=-1, best_level2=-1, best_idx=-1)
        if not cand:
            outcome[k] = EMPTY_WINDOW; continue
        best, best2, lvl, lvl2, bidx, adm = 256, 256, -1, -1, -1, 0
        for i in cand:
            if state[i] is not None and state[i][1]:
                continue                                                             # :87-89
            if cur["uright"][i] > 0:
                if abs(F(info["ur"] - F(cur["uright"][i]))) > radius:
                    continue                                                         # :91-96
            adm += 1
            d = hamming(p["desc"], cur["desc"][i])
            if d < best:
                best2, best, lvl2, lvl, bidx = best, d, lvl, int(kps["octave"][i]), i
            elif d < best2:
                lvl2, best2 = int(kps["octave"][i]), d
        info.update(n_admitted=adm, best_dist=best, best_dist2=best2, best_level=lvl, best_level2=lvl2, best_idx=bidx)
        if adm == 0:
            outcome[k] = ALL_BLOCKED; continue
        if best > TH_HIGH:
            outcome[k] = OVER_TH_HIGH; continue
        if lvl == lvl2 and F(best) > F(nn * F(best2)):
            outcome[k] = RATIO_FAILED; continue
        if state[bidx] is not None:
            outcome[state[bidx][0]] = ACCEPTED_THEN_REPLACED
        state[bidx] = (k, p["nObs"] > 0)
        outcome[k] = ACCEPTED
        nm += 1
    assign = np.array([s[0] if (s is not None and s[0] >= 0) else -1 for s in state], np.int32).reshape(n)
    return nm, assign, outcome, infos


# ---- TrackWithMotionModel -------------------------------------------------------------------------------------------------------
def update_last_frame_points(depth, th_depth):
    """Tracking::UpdateLastFrame (Tracking.cc:1256-1300): sorted by (depth, index), taken until one lies beyond mThDepth AND more than 100
    have been taken (that one included)"""
    idx = sorted((float(z), i) for i, z in enumerate(depth) if z > 0)
    if th_depth <= 0:
        return set(i for _, i in idx)
    out = set()
    for z, i in idx:
        out.add(i)
        if z > th_depth and len(out) > 100:
            break
    return out


def rot_bin(a_last, a_cur):
    rot = F(F(a_last) - F(a_cur))
    neg = bool(rot < 0.0)
    if neg:
        rot = F(rot + F(360.0))
    b = c_round(F(rot * F(F(1.0) / F(HISTO_LENGTH))))
    wrapped = b == HISTO_LENGTH
    return (0 if wrapped else b), neg, wrapped


def three_maxima(sizes):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s; ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s; ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s; ind3 = i
    if F(max2) < F(0.1) * F(max1):
        ind2 = ind3 = -1
    elif F(max3) < F(0.1) * F(max1):
        ind3 = -1
    return ind1, ind2, ind3


def track_motion(cam, last, cur, T_last, T_cur, th, th_retry, retry_below, check_orientation=True, th_depth=0.0, points_block=True, point_flags=None):
    """-> (nmatches, per current keypoint the LAST keypoint whose point it holds or -1, outcome per last keypoint, info per last keypoint,
    passes run).  last / cur: dict(kps, desc, uright, depth)."""
    nL, nC = len(last["kps"]), len(cur["kps"])
    outcome = np.zeros(nL, np.int32)
    infos = [dict() for _ in range(nL)]
    if point_flags is not None:
        has = [bool(last["depth"][i] > 0 and (int(point_flags[i]) & 1)) for i in range(nL)]
        blocks = [bool((int(point_flags[i]) >> 1) & 1) for i in range(nL)]
    else:
        taken = update_last_frame_points(last["depth"], th_depth)
        has = [i in taken for i in range(nL)]
        blocks = [bool(points_block) and not th_depth > 0] * nL
    Rl, tl = T_last[:3, :3], T_last[:3, 3]
    Rc, tc = T_cur[:3, :3], T_cur[:3, 3]
    twc = neg_rt_mul(Rc, tc)
    tlc = mul_add(Rl, twc, tl)
    fwd = bool(tlc[2] > F(cam["b"])); bwd = bool(-tlc[2] > F(cam["b"]))
    Owl = neg_rt_mul(Rl, tl)
    invfx = F(F(1.0) / F(cam["fx"])); invfy = F(F(1.0) / F(cam["fy"]))
    grid = build_grid(cur["kps"], cam["bounds"])
    queries = {}
    for i in range(nL):
        z = F(last["depth"][i])
        if not z > 0:
            outcome[i] = NO_DEPTH; continue
        if not has[i]:
            outcome[i] = FLAG_OFF if point_flags is not None else BEYOND_CLOSE_RULE; continue
        x3 = np.array([F(F(F(F(last["kps"]["x"][i]) - F(cam["cx"])) * z) * invfx), F(F(F(F(last["kps"]["y"][i]) - F(cam["cy"])) * z) * invfy), z], F)
        xw = mul_add(np.ascontiguousarray(Rl.T), x3, Owl)
        xc = mul_add(Rc, xw, tc)
        with np.errstate(all="ignore"):
            invz = F(D(1.0) / D(xc[2]))                                              # 1.0 / float: a double quotient, narrowed (:1409)
        infos[i].update(zc=xc[2])
        if invz < 0:
            outcome[i] = M_BEHIND; continue
        u, v = project(cam, xc, invz)
        infos[i].update(u=u, v=v)
        if outside(cam, u, v):
            outcome[i] = M_OUT_OF_IMAGE; continue
        o = int(last["kps"]["octave"][i])
        lo, hi = (o, -1) if fwd else ((0, o) if bwd else (o - 1, o + 1))
        infos[i].update(ur=F(u - F(F(cam["bf"]) * invz)), octave=o, min_level=lo, max_level=hi, forward=fwd, backward=bwd)
        queries[i] = (u, v, o, lo, hi)

    def one(th_):
        th_ = F(th_)
        state = [None] * nC                                                          # (last keypoint, blocks)
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        nm = 0
        claims = {}                                                                  # last keypoint -> (current keypoint, bin)
        for i in range(nL):
            if i not in queries:
                continue
            u, v, o, lo, hi = queries[i]
            info = infos[i]
            radius = F(th_ * F(cam["scale"][o]))
            cand = features_in_area(grid, cur["kps"], cam["bounds"], u, v, radius, lo, hi)
            info.update(radius=radius, level=o, n_window=len(cand), n_admitted=0, best_dist=256, best_idx=-1, negative_rot=False, wrapped=False)
            if not cand:
                outcome[i] = M_EMPTY_WINDOW; continue
            best, bidx, adm = 256, -1, 0
            for i2 in cand:
                if state[i2] is not None and state[i2][1]:
                    continue                                                         # :1447-1449
                if cur["uright"][i2] > 0:
                    if abs(F(info["ur"] - F(cur["uright"][i2]))) > radius:
                        continue                                                     # :1451-1457
                adm += 1
                d = hamming(last["desc"][i], cur["desc"][i2])
                if d < best:
                    best, bidx = d, i2
            info.update(n_admitted=adm, best_dist=best, best_idx=bidx)
            if adm == 0:
                outcome[i] = ALL_REFUSED; continue
            if best > TH_HIGH:
                outcome[i] = M_OVER_TH_HIGH; continue
            if state[bidx] is not None:
                outcome[state[bidx][0]] = M_ACCEPTED_THEN_REPLACED
            state[bidx] = (i, blocks[i])
            outcome[i] = M_ACCEPTED
            nm += 1
            b = -1
            if check_orientation:
                b, neg, wrapped = rot_bin(last["kps"]["angle"][i], cur["kps"]["angle"][bidx])
                info.update(negative_rot=neg, wrapped=wrapped)
                rot_hist[b].append(bidx)
            info["bin"] = b
            claims[i] = (bidx, b)
        if check_orientation:
            keep = three_maxima([len(h) for h in rot_hist])
            for b in range(HISTO_LENGTH):
                if b in keep:
                    continue
                for i2 in rot_hist[b]:
                    state[i2] = None                                                 # :1506: whoever holds it now
                    nm -= 1
            for i, (i2, b) in claims.items():
                if b not in keep:
                    outcome[i] = ROT_REMOVED
        for i, (i2, b) in claims.items():
            infos[i]["kept"] = state[i2] is not None and state[i2][0] == i
        return nm, np.array([s[0] if s is not None else -1 for s in state], np.int32).reshape(nC)

    nm, assign = one(th)
    passes = 1
    if nm < retry_below:                                                             # Tracking.cc:1320-1330: the frame's points are cleared first
        nm, assign = one(th_retry)
        passes = 2
    return nm, assign, outcome, infos, passes
