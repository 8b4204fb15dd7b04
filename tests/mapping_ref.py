"""mapping_ref.py -- plain-Python restatements of the mapping and loop-closing searches of ORBmatcher (test infrastructure only), written
from the reference's own text, ORB/src/ORBmatcher.cc:

  CheckDistEpipolarLine (:146-163), SearchByProjection(KeyFrame*, Scw, ...) (:296-409, the loop :368-404), SearchForInitialization (:411-526),
  SearchByBoW(KeyFrame*, KeyFrame*) (:528-661), SearchForTriangulation (:663-829), Fuse(KeyFrame*, vpMapPoints, th) (:831-981, the loop
  :898-977), Fuse(KeyFrame*, Scw, ...) (:983-1106, the loop :1057-1102), SearchBySim3 (:1145-1369, the loops :1234-1267, :1314-1347, :1350-1366),
  ComputeThreeMaxima (:1654-1698), Frame::GetFeaturesInArea (Frame.cc:615-668), KeyFrame::GetFeaturesInArea (KeyFrame.cc:606-645).

Nothing here calls the C oracle or the device.  Inputs are the flat-query contract of include/ivfront.h: the caller has projected the map points
(u, v, ur, radius = th * mvScaleFactors[level], level = nPredictedLevel, desc, valid), feature vectors are {node id: [feature indices]}.
float32 where the reference computes in `float`; double where it compares a float with a double literal (`7.8`, `5.99`, `3.84*sigma2`).

Besides its result every search says, per item, WHERE the item left the loop (an outcome code) and what it had on the way (an info dict):
tests/mapping_scenes.py builds scenes on both sides of every comparison and tests/test_mapping_scenes_cpu.py checks through these codes that
they still stand there.  Where no candidate of an item is taken, the code is the stage the candidate that came furthest was refused at.

`fault=` names ONE deliberate misreading (FAULTS); the CPU module shows that each changes the result of some scene.

KeyFrame::mnMinX .. mnMaxY are `int` (KeyFrame.h:212) where Frame's are float: the scenes use integral bounds, where the two agree."""
import bisect
import math

import numpy as np

from projection_ref import F, D, hamming, c_round, build_grid, grid_inv, rot_bin, three_maxima, GRID_COLS, GRID_ROWS, HISTO_LENGTH

TH_LOW, TH_HIGH, INT_MAX = 50, 100, 2 ** 31 - 1

(INVALID, SKIPPED_LEVEL, EMPTY_WINDOW, OCCUPIED, OVER_TH, RATIO_FAILED, CHI2_FAILED, EPIPOLE_TOO_CLOSE, DEN_ZERO, OFF_EPIPOLAR_LINE, ACCEPTED,
 ACCEPTED_THEN_STOLEN, ROT_REMOVED, NO_AGREEMENT, NODE_NOT_SHARED, MAP_POINT, NOT_STEREO) = range(17)
NAMES = ["not valid", "skipped level", "empty window", "occupied", "over TH", "ratio failed", "chi-square failed", "epipole too close", "den == 0",
         "off the epipolar line", "accepted", "accepted, then stolen", "accepted, removed by the rotation filter", "no mutual agreement",
         "node on one side only", "map point rule", "not stereo"]
# the codes each search can end an item with; the CPU module reaches every one
CODES = dict(
    keyframe=(INVALID, EMPTY_WINDOW, SKIPPED_LEVEL, OCCUPIED, OVER_TH, ACCEPTED),
    fuse=(INVALID, EMPTY_WINDOW, SKIPPED_LEVEL, CHI2_FAILED, OVER_TH, ACCEPTED),
    fuse_scw=(INVALID, EMPTY_WINDOW, SKIPPED_LEVEL, OVER_TH, ACCEPTED),
    sim3=(INVALID, EMPTY_WINDOW, SKIPPED_LEVEL, OVER_TH, NO_AGREEMENT, ACCEPTED),
    init=(SKIPPED_LEVEL, EMPTY_WINDOW, OCCUPIED, OVER_TH, RATIO_FAILED, ACCEPTED, ACCEPTED_THEN_STOLEN, ROT_REMOVED),
    bow=(NODE_NOT_SHARED, MAP_POINT, OCCUPIED, OVER_TH, RATIO_FAILED, ACCEPTED, ROT_REMOVED),
    triangulation=(NODE_NOT_SHARED, MAP_POINT, NOT_STEREO, OCCUPIED, OVER_TH, EPIPOLE_TOO_CLOSE, DEN_ZERO, OFF_EPIPOLAR_LINE, ACCEPTED, ROT_REMOVED))
FAULTS = dict(
    keyframe=("window_le", "level_up", "th_lt"),
    fuse=("window_le", "level_up", "th_lt", "chi2_float"),
    fuse_scw=("window_le", "level_up", "th_lt"),
    sim3=("window_le", "level_up", "th_lt", "no_agreement_check"),
    init=("window_le", "th_lt", "no_decrement_on_steal", "decrement_twice"),
    bow=("th_le", "ignores_matched2"),
    triangulation=("th_lt", "sets_matched2", "first_minimum", "epipolar_float", "epipole_gate_on_stereo"))


# ---- GetFeaturesInArea --------------------------------------------------------------------------------------------------------------
def window(grid, kps, bounds, x, y, r, min_level=-1, max_level=-1, fault=None):
    """Frame::GetFeaturesInArea (Frame.cc:615-668); with min_level = max_level = -1 it is KeyFrame::GetFeaturesInArea (KeyFrame.cc:606-645),
    which has no level test.  Cells: ix outer, iy inner, insertion order inside a cell."""
    iw, ih = grid_inv(bounds)
    x = F(x); y = F(y); r = F(r); minx = F(bounds[0]); miny = F(bounds[1])
    x0 = max(0, int(math.floor(F(F(F(x - minx) - r) * iw))))                                 # KeyFrame.cc:611
    if x0 >= GRID_COLS:
        return []
    x1 = min(GRID_COLS - 1, int(math.ceil(F(F(F(x - minx) + r) * iw))))                      # :615
    if x1 < 0:
        return []
    y0 = max(0, int(math.floor(F(F(F(y - miny) - r) * ih))))                                 # :619
    if y0 >= GRID_ROWS:
        return []
    y1 = min(GRID_ROWS - 1, int(math.ceil(F(F(F(y - miny) + r) * ih))))                      # :623
    if y1 < 0:
        return []
    check = min_level > 0 or max_level >= 0                                                    # Frame.cc:638
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for i in grid.get((ix, iy), ()):
                o = int(kps["octave"][i])
                if check:
                    if o < min_level:
                        continue                                                               # Frame.cc:650
                    if max_level >= 0 and o > max_level:
                        continue                                                               # Frame.cc:653
                dx = abs(F(F(kps["x"][i]) - x)); dy = abs(F(F(kps["y"][i]) - y))
                if (dx <= r and dy <= r) if fault == "window_le" else (dx < r and dy < r):     # KeyFrame.cc:638, Frame.cc:660: strict
                    out.append(i)
    return out


def level_ok(o, level, fault):
    """kpLevel<nPredictedLevel-1 || kpLevel>nPredictedLevel -> continue (:386, :917, :1073, :1250, :1330)"""
    if fault == "level_up":
        return level <= o <= level + 1
    return not (o < level - 1 or o > level)


def th_ok(best, th, fault):
    """bestDist<=TH (:400, :958, :1088, :1264, :1344, :465)"""
    return best < th if fault == "th_lt" else best <= th


def _best_in_window(grid, kps, desc, bounds, q, i, fault, occupied=None, start=256):
    """the window walk the four KeyFrame searches share: (outcome or None, info).  None = some candidate was compared."""
    cand = window(grid, kps, bounds, q["u"][i], q["v"][i], q["radius"][i], fault=fault)
    info = dict(n_window=len(cand), n_level=0, n_compared=0, best_dist=start, best_idx=-1)
    if not cand:
        return EMPTY_WINDOW, info                                                              # vIndices.empty() (:370)
    lv = int(q["level"][i])
    best, bidx, n_level, n_cmp = start, -1, 0, 0
    for idx in cand:
        if occupied is not None and occupied[idx]:
            continue                                                                           # if(vpMatched[idx]) (:381)
        if not level_ok(int(kps["octave"][idx]), lv, fault):
            continue
        n_level += 1
        n_cmp += 1
        d = hamming(q["desc"][i], desc[idx])
        if d < best:                                                                           # strict: the first minimum stays (:393)
            best, bidx = d, idx
    info.update(n_level=n_level, n_compared=n_cmp, best_dist=best, best_idx=bidx)
    return None, info


def _refused(kps, cand, lv, fault, occupied):
    """why nothing was compared: an in-level candidate exists but is occupied, or none is in level"""
    return OCCUPIED if any(level_ok(int(kps["octave"][i]), lv, fault) for i in cand if occupied is not None and occupied[i]) else SKIPPED_LEVEL


# ---- SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th): the loop :368-404 ---------------------------------------------------
def search_keyframe_points(kps, desc, bounds, q, matched=None, fault=None):
    """-> (matched [n_kf]: -1 free, -2 occupied on entry, >= 0 the query matched there; nmatches; outcome per query; info per query)"""
    n = len(kps); nq = len(q["u"])
    m = np.full(n, -1, np.int32) if matched is None else np.array(matched, np.int32)
    grid = build_grid(kps, bounds)
    outcome = np.zeros(nq, np.int32); infos = []
    nm = 0
    for i in range(nq):
        if not q["valid"][i]:
            outcome[i] = INVALID; infos.append({}); continue
        occ = m != -1
        oc, info = _best_in_window(grid, kps, desc, bounds, q, i, fault, occupied=occ)
        infos.append(info)
        if oc is not None:
            outcome[i] = oc; continue
        if info["n_compared"] == 0:
            outcome[i] = _refused(kps, window(grid, kps, bounds, q["u"][i], q["v"][i], q["radius"][i], fault=fault), int(q["level"][i]), fault, occ); continue
        if th_ok(info["best_dist"], TH_LOW, fault):                                            # :400
            m[info["best_idx"]] = i; nm += 1; outcome[i] = ACCEPTED
        else:
            outcome[i] = OVER_TH
    return m, nm, outcome, infos


# ---- Fuse(KeyFrame*, vpMapPoints, th) :898-977 and Fuse(KeyFrame*, Scw, ...) :1057-1102 ------------------------------------------------
def fuse_candidates(kps, desc, uright, bounds, inv_level_sigma2, q, fault=None):
    """-> (best_idx, best_dist, outcome, infos).  inv_level_sigma2 None: the Scw variant, no reprojection gate; its bestDist starts at INT_MAX
    (:1066) and is reported as 256 while nothing was compared, which is what the interface says for `nothing` (a distance never exceeds 256)."""
    nq = len(q["u"])
    gate = inv_level_sigma2 is not None
    grid = build_grid(kps, bounds)
    bi = np.full(nq, -1, np.int32); bd = np.full(nq, 256, np.int32)
    outcome = np.zeros(nq, np.int32); infos = []
    for i in range(nq):
        if not q["valid"][i]:
            outcome[i] = INVALID; infos.append({}); continue
        u = F(q["u"][i]); v = F(q["v"][i]); lv = int(q["level"][i])
        cand = window(grid, kps, bounds, u, v, q["radius"][i], fault=fault)                    # :898
        info = dict(n_window=len(cand), n_level=0, n_compared=0, best_dist=256, best_idx=-1)
        infos.append(info)
        if not cand:
            outcome[i] = EMPTY_WINDOW; continue                                                # :900
        best, bidx = (256 if gate else INT_MAX), -1                                            # :907, :1066
        for idx in cand:
            o = int(kps["octave"][idx])
            if not level_ok(o, lv, fault):
                continue                                                                       # :917, :1073
            info["n_level"] += 1
            if gate:
                ex = F(u - F(kps["x"][idx])); ey = F(v - F(kps["y"][idx]))
                if uright[idx] >= 0:                                                           # :920: 0 is stereo
                    er = F(F(q["ur"][i]) - F(uright[idx]))
                    e2 = F(F(F(ex * ex) + F(ey * ey)) + F(er * er))                            # :929
                    limit = 7.8
                else:
                    e2 = F(F(ex * ex) + F(ey * ey))                                            # :940
                    limit = 5.99
                chi2 = F(e2 * F(inv_level_sigma2[o]))                                          # a float product ...
                info.update(e2=e2, chi2=chi2, stereo=bool(uright[idx] >= 0))
                if (chi2 > F(limit)) if fault == "chi2_float" else (float(chi2) > limit):      # ... against a double literal (:931, :942)
                    continue
            info["n_compared"] += 1
            d = hamming(q["desc"][i], desc[idx])
            if d < best:                                                                       # :950, :1080
                best, bidx = d, idx
        info.update(best_dist=min(best, 256), best_idx=bidx)
        bd[i] = min(best, 256)
        if info["n_compared"] == 0:
            outcome[i] = CHI2_FAILED if info["n_level"] else SKIPPED_LEVEL; continue
        if th_ok(best, TH_LOW, fault):                                                         # :958, :1088
            bi[i] = bidx; outcome[i] = ACCEPTED
        else:
            outcome[i] = OVER_TH
    return bi, bd, outcome, infos


# ---- SearchBySim3: :1234-1267, :1314-1347, :1350-1366 -----------------------------------------------------------------------------------
def search_by_sim3(kps1, desc1, bounds1, kps2, desc2, bounds2, q12, q21, fault=None):
    """-> (matches12 [n1], nFound, (outcome per KF1 slot, outcome per KF2 slot), (infos1, infos2)).  No occupancy: vnMatch1 / vnMatch2 are
    written per query, two queries may name the same keypoint."""
    def direction(q, kps, desc, bounds):
        nq = len(q["u"]); grid = build_grid(kps, bounds)
        match = np.full(nq, -1, np.int32); outcome = np.zeros(nq, np.int32); infos = []
        for i in range(nq):
            if not q["valid"][i]:
                outcome[i] = INVALID; infos.append({}); continue
            oc, info = _best_in_window(grid, kps, desc, bounds, q, i, fault, start=INT_MAX)    # bestDist = INT_MAX (:1242, :1322)
            info["best_dist"] = min(info["best_dist"], 256)
            infos.append(info)
            if oc is not None:
                outcome[i] = oc
            elif info["n_compared"] == 0:
                outcome[i] = SKIPPED_LEVEL
            elif th_ok(info["best_dist"], TH_HIGH, fault):                                     # :1264, :1344
                match[i] = info["best_idx"]; outcome[i] = ACCEPTED
            else:
                outcome[i] = OVER_TH
        return match, outcome, infos
    m1, o1, i1 = direction(q12, kps2, desc2, bounds2)
    m2, o2, i2 = direction(q21, kps1, desc1, bounds1)
    m12 = np.full(len(kps1), -1, np.int32)
    nf = 0
    for a in range(len(kps1)):
        b = m1[a]
        if b >= 0:                                                                             # :1357
            if m2[b] == a or fault == "no_agreement_check":                                    # :1360
                m12[a] = b; nf += 1
            else:
                o1[a] = NO_AGREEMENT
    for b in range(len(kps2)):
        if m2[b] >= 0 and m12[m2[b]] != b:
            o2[b] = NO_AGREEMENT
    return m12, nf, (o1, o2), (i1, i2)


# ---- the rotation histogram the three remaining searches share -----------------------------------------------------------------------
def _kept_bins(hist):
    return three_maxima([len(h) for h in hist])


# ---- SearchForInitialization :411-526 -------------------------------------------------------------------------------------------------
def search_for_initialization(kps1, desc1, kps2, desc2, bounds2, prev_matched, window_size, nn_ratio, check_orientation, fault=None):
    """-> (vnMatches12, vbPrevMatched updated, nmatches, outcome per F1 keypoint, infos)"""
    n1, n2 = len(kps1), len(kps2)
    prev = np.array(prev_matched, F).reshape(-1, 2).copy()
    m12 = np.full(n1, -1, np.int32); m21 = np.full(n2, -1, np.int32)
    mdist = [INT_MAX] * n2                                                                     # vMatchedDistance (:421)
    grid = build_grid(kps2, bounds2)
    hist = [[] for _ in range(HISTO_LENGTH)]
    outcome = np.zeros(n1, np.int32); infos = [dict() for _ in range(n1)]
    nm = 0
    nn = F(nn_ratio)
    for i1 in range(n1):
        level1 = int(kps1["octave"][i1])
        if level1 > 0:
            outcome[i1] = SKIPPED_LEVEL; continue                                              # :428
        cand = window(grid, kps2, bounds2, prev[i1, 0], prev[i1, 1], F(int(window_size)), level1, level1, fault=fault)   # :431
        info = infos[i1]
        info.update(n_window=len(cand), n_compared=0, best_dist=INT_MAX, best_dist2=INT_MAX, best_idx=-1)
        if not cand:
            outcome[i1] = EMPTY_WINDOW; continue                                               # :433
        best, best2, bidx, n_cmp = INT_MAX, INT_MAX, -1, 0
        for i2 in cand:
            d = hamming(desc1[i1], desc2[i2])
            if mdist[i2] <= d:
                continue                                                                       # :450
            n_cmp += 1
            if d < best:
                best2, best, bidx = best, d, i2                                                # :453-458
            elif d < best2:
                best2 = d                                                                      # :459-462
        info.update(n_compared=n_cmp, best_dist=best, best_dist2=best2, best_idx=bidx)
        if n_cmp == 0:
            outcome[i1] = OCCUPIED; continue
        if not th_ok(best, TH_LOW, fault):                                                     # :465
            outcome[i1] = OVER_TH; continue
        if not float(F(best)) < float(F(F(best2) * nn)):                                       # bestDist<(float)bestDist2*mfNNratio (:467)
            outcome[i1] = RATIO_FAILED; continue
        if m21[bidx] >= 0:                                                                     # :469-473
            m12[m21[bidx]] = -1
            outcome[m21[bidx]] = ACCEPTED_THEN_STOLEN
            if fault != "no_decrement_on_steal":
                nm -= 1
        m12[i1] = bidx; m21[bidx] = i1; mdist[bidx] = best; nm += 1                            # :474-477
        outcome[i1] = ACCEPTED
        if check_orientation:
            b, _, _ = rot_bin(kps1["angle"][i1], kps2["angle"][bidx])                          # :481-486
            hist[b].append(i1); info["bin"] = b
    if check_orientation:
        keep = _kept_bins(hist)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for i1 in hist[b]:
                if m12[i1] >= 0:                                                               # :510: a stolen entry was counted down already
                    m12[i1] = -1; nm -= 1; outcome[i1] = ROT_REMOVED
                elif fault == "decrement_twice":
                    nm -= 1
    for i1 in range(n1):
        if m12[i1] >= 0:                                                                       # :521-523: survivors only
            prev[i1, 0] = kps2["x"][m12[i1]]; prev[i1, 1] = kps2["y"][m12[i1]]
    return m12, prev, nm, outcome, infos


# ---- the walk over two DBoW2::FeatureVector (std::map) both BoW searches share --------------------------------------------------------
def shared_nodes(fv1, fv2):
    """:556-638 / :697-795 -> (node ids visited with both sides present, lower_bound calls on side 1, on side 2)"""
    n1, n2 = sorted(fv1), sorted(fv2)
    a = b = 0
    out, j1, j2 = [], 0, 0
    while a < len(n1) and b < len(n2):
        if n1[a] == n2[b]:
            out.append(n1[a]); a += 1; b += 1
        elif n1[a] < n2[b]:
            a = bisect.bisect_left(n1, n2[b]); j1 += 1                                         # f1it = vFeatVec1.lower_bound(f2it->first)
        else:
            b = bisect.bisect_left(n2, n1[a]); j2 += 1
    return out, j1, j2


# ---- SearchByBoW(KeyFrame*, KeyFrame*) :528-661 -----------------------------------------------------------------------------------------
def search_by_bow_keyframes(kps1, desc1, has1, fv1, kps2, desc2, has2, fv2, nn_ratio, check_orientation, fault=None):
    """-> (matches12 [n1], nmatches, outcome per KF1 feature, infos, dict(jumps1, jumps2, nodes))"""
    n1, n2 = len(kps1), len(kps2)
    m12 = np.full(n1, -1, np.int32)
    matched2 = [False] * n2                                                                    # vbMatched2 (:541)
    hist = [[] for _ in range(HISTO_LENGTH)]
    outcome = np.full(n1, NODE_NOT_SHARED, np.int32); infos = [dict() for _ in range(n1)]
    nm = 0
    nn = F(nn_ratio)
    nodes, j1, j2 = shared_nodes(fv1, fv2)
    for node in nodes:
        for idx1 in fv1[node]:
            if not has1[idx1]:
                outcome[idx1] = MAP_POINT; continue                                            # :565-568
            best1, best2, bidx, n_cmp = 256, 256, -1, 0
            for idx2 in fv2[node]:
                if (matched2[idx2] and fault != "ignores_matched2") or not has2[idx2]:
                    continue                                                                   # :582-586
                n_cmp += 1
                d = hamming(desc1[idx1], desc2[idx2])
                if d < best1:
                    best2, best1, bidx = best1, d, idx2                                        # :592-597
                elif d < best2:
                    best2 = d                                                                  # :598-601
            infos[idx1].update(node=node, n_compared=n_cmp, best_dist=best1, best_dist2=best2, best_idx=bidx)
            if n_cmp == 0:
                outcome[idx1] = OCCUPIED; continue
            if not (best1 <= TH_LOW if fault == "th_le" else best1 < TH_LOW):                  # :604: strict here
                outcome[idx1] = OVER_TH; continue
            if not float(F(best1)) < float(F(nn * F(best2))):                                  # :606
                outcome[idx1] = RATIO_FAILED; continue
            m12[idx1] = bidx; matched2[bidx] = True; nm += 1; outcome[idx1] = ACCEPTED         # :608-609, :622
            if check_orientation:
                b, _, _ = rot_bin(kps1["angle"][idx1], kps2["angle"][bidx])
                hist[b].append(idx1); infos[idx1]["bin"] = b
    if check_orientation:
        keep = _kept_bins(hist)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in hist[b]:
                m12[idx1] = -1; nm -= 1; outcome[idx1] = ROT_REMOVED                           # :654-655
    return m12, nm, outcome, infos, dict(jumps1=j1, jumps2=j2, nodes=nodes)


# ---- CheckDistEpipolarLine :146-163 -----------------------------------------------------------------------------------------------------
def epipolar(kp1x, kp1y, kp2x, kp2y, F12, sigma2, fault=None):
    """-> (True / False / None for den == 0, dict(a, b, c, num, den, dsqr))"""
    f = np.asarray(F12, F).reshape(3, 3)
    x1, y1, x2, y2 = F(kp1x), F(kp1y), F(kp2x), F(kp2y)
    a = F(F(F(x1 * f[0, 0]) + F(y1 * f[1, 0])) + f[2, 0])                                      # :149
    b = F(F(F(x1 * f[0, 1]) + F(y1 * f[1, 1])) + f[2, 1])                                      # :150
    c = F(F(F(x1 * f[0, 2]) + F(y1 * f[1, 2])) + f[2, 2])                                      # :151
    num = F(F(F(a * x2) + F(b * y2)) + c)                                                      # :153
    den = F(F(a * a) + F(b * b))                                                               # :155
    info = dict(a=a, b=b, c=c, num=num, den=den)
    if den == 0:
        return None, info                                                                      # :157
    dsqr = F(F(num * num) / den)                                                               # :160
    info["dsqr"] = dsqr
    if fault == "epipolar_float":
        return bool(dsqr < F(F(3.84) * F(sigma2))), info
    return bool(float(dsqr) < 3.84 * float(F(sigma2))), info                                   # :162: a double product


# ---- SearchForTriangulation :663-829 ----------------------------------------------------------------------------------------------------
def search_for_triangulation(kps1, desc1, has1, stereo1, fv1, kps2, desc2, has2, stereo2, fv2, F12, ex, ey, scale2, sigma2_2, only_stereo,
                             check_orientation, fault=None):
    """-> (matches12 [n1], nmatches, outcome per KF1 feature, infos).  vbMatched2 is tested (:731) and never set; `dist>bestDist` (:744) lets
    a later equal distance replace the earlier one; bestDist starts at TH_LOW (:721)."""
    n1, n2 = len(kps1), len(kps2)
    m12 = np.full(n1, -1, np.int32)
    matched2 = [False] * n2                                                                    # :683
    hist = [[] for _ in range(HISTO_LENGTH)]
    outcome = np.full(n1, NODE_NOT_SHARED, np.int32); infos = [dict() for _ in range(n1)]
    nm = 0
    ex = F(ex); ey = F(ey)
    order = (OCCUPIED, NOT_STEREO, OVER_TH, EPIPOLE_TOO_CLOSE, DEN_ZERO, OFF_EPIPOLAR_LINE)
    for node in shared_nodes(fv1, fv2)[0]:
        for idx1 in fv1[node]:
            if has1[idx1]:
                outcome[idx1] = MAP_POINT; continue                                            # :708
            st1 = bool(stereo1[idx1])
            if only_stereo and not st1:
                outcome[idx1] = NOT_STEREO; continue                                           # :713-715
            best, bidx, far = TH_LOW, -1, -1                                                   # :721
            info = infos[idx1]; info.update(node=node, n_taken=0)
            for idx2 in fv2[node]:
                if matched2[idx2] or has2[idx2]:
                    far = max(far, 0); continue                                                # :731
                st2 = bool(stereo2[idx2])
                if only_stereo and not st2:
                    far = max(far, 1); continue                                                # :736-738
                d = hamming(desc1[idx1], desc2[idx2])
                worse = (d >= best and bidx >= 0) or d > best if fault == "first_minimum" else d > best
                if (d >= TH_LOW if fault == "th_lt" else d > TH_LOW) or worse:
                    far = max(far, 2); continue                                                # :744: dist>TH_LOW || dist>bestDist
                o2 = int(kps2["octave"][idx2])
                if (not st1 and not st2) or fault == "epipole_gate_on_stereo":                 # :749
                    dx = F(ex - F(kps2["x"][idx2])); dy = F(ey - F(kps2["y"][idx2]))
                    e2 = F(F(dx * dx) + F(dy * dy))
                    info["epipole_d2"] = e2
                    if e2 < F(F(100) * F(scale2[o2])):                                         # :753: int * float, a float
                        far = max(far, 3); continue
                ok, ep = epipolar(kps1["x"][idx1], kps1["y"][idx1], kps2["x"][idx2], kps2["y"][idx2], F12, sigma2_2[o2], fault)
                info.update(ep)
                if ok is None:
                    far = max(far, 4); continue
                if not ok:
                    far = max(far, 5); continue
                bidx, best = idx2, d                                                           # :759-760
                info["n_taken"] += 1
            info.update(best_dist=best, best_idx=bidx)
            if bidx < 0:
                outcome[idx1] = order[far] if far >= 0 else OCCUPIED; continue
            m12[idx1] = bidx; nm += 1; outcome[idx1] = ACCEPTED                                # :767-768
            if fault == "sets_matched2":
                matched2[bidx] = True
            if check_orientation:
                b, _, _ = rot_bin(kps1["angle"][idx1], kps2["angle"][bidx])
                hist[b].append(idx1); info["bin"] = b
    if check_orientation:
        keep = _kept_bins(hist)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in hist[b]:
                m12[idx1] = -1; nm -= 1; outcome[idx1] = ROT_REMOVED                           # :811-812
    return m12, nm, outcome, infos
