"""sim3_search_ref.py -- the numpy restatement of what ivf_tracker_search_by_sim3 adds to the per-call search (test infrastructure only):
the inlier filter of LoopClosing.cc:318-323, vbAlreadyMatched1 / 2 (ORBmatcher.cc:1175-1185) and BOTH projection loops of
ORBmatcher::SearchBySim3 (:1191-1233, :1271-1313), written from the reference's own text in the arithmetic DESIGN.md A-15 states; the
queries then go to mapping_ref.search_by_sim3 (the window searches and the agreement check) and the BoW search of the chain is
mapping_ref.search_by_bow_keyframes as it stands, on feature vectors of create_points_ref.feature_vector.

A keyframe is dict(n, kps [n] KP_DTYPE, desc [n, 32], pose [12] float32 (Tcw, row-major 3x4), points [n] LOCAL_POINT_DTYPE (pos, min_distance,
max_distance, desc, flags bit 0 = no point / isBad())); cam is dict(fx, fy, cx, cy, bounds, scale); sim3 is the 16 floats solve_sim3 writes.

f64=True runs the same loops entirely in double (from the same float inputs, nothing narrowed, libm's log): the yardstick of the gate
margins tests/test_sim3_search_cpu.py records in tests/golden/sim3_search_noise.json."""
import math

import numpy as np

import mapping_ref as M
import projection_ref as PR
from create_points_ref import feature_vector  # noqa: F401  (the chain's feature vectors)

F, D = np.float32, np.float64
(NO_POINT, ALREADY, BEHIND, OUT_OF_IMAGE, TOO_NEAR, TOO_FAR, VALID) = range(7)
STAGE_NAMES = ["no point / bad", "already matched", "z < 0", "outside the image", "too near", "too far", "searched"]


def matches_in(kf1, match12, inlier):
    """vpMatches12 on entry (LoopClosing.cc:318-323): the match where the inlier flag keeps it, else none"""
    n1 = kf1["n"]
    out = np.full(n1, -1, np.int32)
    for i in range(n1):
        if match12[i] >= 0 and (inlier is None or inlier[i]):
            out[i] = match12[i]
    return out


def similarity(sim3, f64=False):
    """-> (sR12, t12, sR21, t21) (:1160-1162)"""
    s = np.asarray(sim3, F)
    R12 = s[:9].reshape(3, 3); t12 = s[9:12]; s12 = s[12]
    with np.errstate(all="ignore"):
        sR12 = D(s12) * R12.astype(D)
        sR21 = (D(1.0) / D(s12)) * R12.T.astype(D)
        if not f64:
            sR12 = sR12.astype(F); sR21 = sR21.astype(F)
        t21 = np.array([-(D(sR21[i, 0]) * D(t12[0]) + D(sR21[i, 1]) * D(t12[1]) + D(sR21[i, 2]) * D(t12[2])) for i in range(3)], D)
    return sR12, (t12.astype(D) if f64 else t12), sR21, (t21 if f64 else t21.astype(F))


def _mul_add(R, p, t, f64):
    R = np.asarray(R, D); p = np.asarray(p, D); t = np.asarray(t, D)
    with np.errstate(all="ignore"):
        x = np.array([R[i, 0] * p[0] + R[i, 1] * p[1] + R[i, 2] * p[2] + t[i] for i in range(3)], D)
    return x if f64 else x.astype(F)


def project_side(cam, src, sR, tt, already, th, f64=False):
    """one direction (:1191-1233): -> (queries in the flat-query contract of mapping_ref, per-keypoint info: stage, z, u, v, dist, lv, ...)"""
    n = src["n"]
    T = np.asarray(src["pose"], F).reshape(3, 4)
    q = dict(u=np.zeros(n, F), v=np.zeros(n, F), radius=np.zeros(n, F), level=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8), valid=np.zeros(n, np.uint8))
    info = []
    b = [F(x) for x in cam["bounds"]]
    N = (lambda x: D(x)) if f64 else (lambda x: F(x))
    fx, fy, cx, cy = (N(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    for i in range(n):
        mp = src["points"][i]
        it = dict(stage=NO_POINT)
        info.append(it)
        if int(mp["flags"]) & 1:
            continue                                                                            # :1195, :1198
        if already[i]:
            it["stage"] = ALREADY; continue                                                     # :1195
        pa = _mul_add(T[:, :3], mp["pos"], T[:, 3], f64)                                        # :1202
        pb = _mul_add(sR, pa, tt, f64)                                                          # :1203
        it.update(z=pb[2], pc=pb)
        if pb[2] < 0.0:
            it["stage"] = BEHIND; continue                                                      # :1206
        with np.errstate(all="ignore"):
            invz = N(D(1.0) / D(pb[2]))                                                         # :1209: a double quotient, narrowed once
            x = N(pb[0] * invz); y = N(pb[1] * invz)                                            # :1210-1211
            u = N(N(fx * x) + cx); v = N(N(fy * y) + cy)                                        # :1213-1214
        it.update(u=u, v=v)
        if not (u >= b[0] and u < b[2] and v >= b[1] and v < b[3]):                             # KeyFrame::IsInImage (KeyFrame.cc:647-650)
            it["stage"] = OUT_OF_IMAGE; continue
        dist = N(math.sqrt(float(D(pb[0]) * D(pb[0]) + D(pb[1]) * D(pb[1]) + D(pb[2]) * D(pb[2]))))   # cv::norm(p3Dc2) (:1222)
        min_d = N(N(F(0.8)) * N(mp["min_distance"])); max_d = N(N(F(1.2)) * N(mp["max_distance"]))  # MapPoint.cc:378-388
        it.update(dist=dist, min_d=min_d, max_d=max_d, max_distance=F(mp["max_distance"]))
        if dist < min_d:
            it["stage"] = TOO_NEAR; continue                                                    # :1225
        if dist > max_d:
            it["stage"] = TOO_FAR; continue
        if f64:
            lv = int(math.ceil(math.log(float(D(mp["max_distance"]) / dist)) / math.log(float(D(cam["scale"][1])))))
            lv = min(max(lv, 0), len(cam["scale"]) - 1)
        else:
            lv = PR.predict_scale(cam, mp["max_distance"], dist)                                # :1229
        it.update(stage=VALID, lv=lv)
        q["u"][i] = u; q["v"][i] = v; q["radius"][i] = F(F(th) * F(cam["scale"][lv])); q["level"][i] = lv; q["desc"][i] = mp["desc"]; q["valid"][i] = 1
    return q, info


def search(cam, kf1, kf2, sim3, match12, inlier=None, th=7.5, f64=False, nf=None):
    """-> dict(matches, nfound, match1 = vnMatch1, match2 = vnMatch2, q12, q21, info1, info2, outcome, infos); matches / match1 / match2
    are padded with -1 to nf entries where nf is given"""
    n1, n2 = kf1["n"], kf2["n"]
    m_in = matches_in(kf1, match12, inlier)
    am1 = m_in >= 0                                                                             # :1175-1185
    am2 = np.zeros(n2, bool)
    for m in m_in:
        if 0 <= m < n2:
            am2[m] = True
    sR12, t12, sR21, t21 = similarity(sim3, f64)
    q12, info1 = project_side(cam, kf1, sR21, t21, am1, th, f64)
    q21, info2 = project_side(cam, kf2, sR12, t12, am2, th, f64)
    m12, nfound, outcome, infos = M.search_by_sim3(kf1["kps"], kf1["desc"], cam["bounds"], kf2["kps"], kf2["desc"], cam["bounds"], q12, q21)
    vn = []
    for o, inf, n in ((outcome[0], infos[0], n1), (outcome[1], infos[1], n2)):
        vn.append(np.array([inf[i]["best_idx"] if o[i] in (M.ACCEPTED, M.NO_AGREEMENT) else -1 for i in range(n)], np.int32).reshape(n))
    matches = m_in.copy()
    matches[m12 >= 0] = m12[m12 >= 0]
    pad = (lambda a: a) if nf is None else (lambda a: np.concatenate([a, np.full(nf - len(a), -1, np.int32)]).astype(np.int32))
    return dict(matches=pad(matches), nfound=int(nfound), match1=pad(vn[0]), match2=pad(vn[1]), q12=q12, q21=q21, info1=info1, info2=info2,
                outcome=outcome, infos=infos, m_in=m_in)


def search_by_bow_keyframes(tree, levelsup, kf1, has1, kf2, has2, nn_ratio=0.75, check_orientation=True, nf=None):
    """the BoW search of the chain on feature vectors computed from the descriptors -> (match12 padded to nf, nmatches, outcome, infos)"""
    fv1 = feature_vector(tree, kf1["desc"], levelsup) if kf1["n"] else {}
    fv2 = feature_vector(tree, kf2["desc"], levelsup) if kf2["n"] else {}
    m12, nm, outcome, infos, _ = M.search_by_bow_keyframes(kf1["kps"], kf1["desc"], has1, fv1, kf2["kps"], kf2["desc"], has2, fv2, nn_ratio, check_orientation)
    if nf is not None:
        m12 = np.concatenate([m12, np.full(nf - len(m12), -1, np.int32)]).astype(np.int32)
    return m12, int(nm), outcome, infos, (fv1, fv2)
