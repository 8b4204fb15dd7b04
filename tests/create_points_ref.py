"""create_points_ref.py -- a plain-Python restatement of LocalMapping::CreateNewMapPoints, stereo / RGB-D branch (test infrastructure
only), written from the reference's own text:

  ORB/src/LocalMapping.cc:273-525 (the loop over neighbours, the triangulation and its gates), :609-626 (ComputeF12), :771-776
  (SkewSymmetricMatrix), ORB/src/ORBmatcher.cc:670-676 (the epipole), ORB/src/MapPoint.cc:247-376 (ComputeDistinctiveDescriptors and
  UpdateNormalAndDepth for N = 2 observations), ORB/src/Frame.cc:958-972 (UnprojectStereo).

SearchForTriangulation itself (ORBmatcher.cc:663-829) is tests/mapping_ref.py's, imported.  Nothing here calls the C oracle or the device.
np.float32 where the reference computes in float, double where it compares with a double literal; cv::Mat products, dot and norm as DESIGN.md
A-11 (double accumulation, one narrowing); the frozen forms of DESIGN.md section 3 "CreateNewMapPoints": F12 in closed form in f64, the stereo
cosine as (d^2 - h^2) / (d^2 + h^2), the singular vector from a cyclic one-sided Jacobi in f64 (Python floats are the doubles of the
device text; neither side fuses a multiply with an add).

Besides the outputs of ivf_tracker_create_map_points every match keeps its stage code and an info dict.  `fault=` names ONE deliberate
misreading (FAULTS); tests/test_create_points_cpu.py shows that each changes the result of some scene."""
import math

import numpy as np

from mapping_ref import search_for_triangulation
from projection_ref import F, hamming, mul_add, neg_rt_mul

LOCAL_POINT_DTYPE = np.dtype([("pos", np.float32, 3), ("normal", np.float32, 3), ("min_distance", np.float32), ("max_distance", np.float32),
                              ("desc", np.uint8, 32), ("flags", np.int32), ("pad", np.int32, 3)])
(NONE, BASELINE, LOW_PARALLAX, W_ZERO, Z1, Z2, CHI2_1_MONO, CHI2_1_STEREO, CHI2_2_MONO, CHI2_2_STEREO, DIST_ZERO, RATIO_LOW, RATIO_HIGH, BY_SVD,
 BY_STEREO1, BY_STEREO2) = range(16)
NAMES = ["no match", "neighbour skipped for its baseline", "low parallax without stereo", "w == 0", "z1 <= 0", "z2 <= 0", "chi-square 1 mono",
         "chi-square 1 stereo", "chi-square 2 mono", "chi-square 2 stereo", "distance zero", "scale ratio low", "scale ratio high", "created by SVD",
         "created by UnprojectStereo(1)", "created by UnprojectStereo(2)"]
FAULTS = ("has1_not_updated", "has1_updated_on_failure", "first_minimum", "stereo2_cos_always", "chi2_float", "chi2_mono_78", "z_lt", "ratio_fabs",
          "min_distance_octave", "desc_ignores_order", "quality_max", "order_by_idx1")
SWEEPS, EPS = 30, 2.0 ** -52


# ---- KeyFrame::ComputeBoW reduced to mFeatVec (TemplatedVocabulary.h:1217-1259, FeatureVector.cpp:31-45) -----------------------------
def feature_vector(tree, desc, levelsup):
    """{node at level L - levelsup: [feature indices ascending]}; the first minimum in child order; a stopped word adds nothing"""
    nid_level = tree["depth"] - levelsup
    fv = {}
    for f in range(len(desc)):
        node, level, nid = 0, 0, 0
        while tree["children"][node]:
            level += 1
            node = min(tree["children"][node], key=lambda c: hamming(desc[f], tree["desc"][c]))       # min() keeps the first of equals
            if level == nid_level:
                nid = node
        if tree["weight"][node] > 0:
            fv.setdefault(nid if nid_level > 0 else 0, []).append(f)
    return fv


# ---- double-accumulated pieces ----------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2])


def norm3(a):
    return math.sqrt(dot3(a, a))


def compute_f12(cam, T1, T2):
    """K1^-T [t12]x R12 K2^-1 (LocalMapping.cc:609-626) in closed form, f64 from the float inputs, narrowed once -> float32 [9]"""
    R1 = [[float(T1[i, j]) for j in range(3)] for i in range(3)]; t1 = [float(T1[i, 3]) for i in range(3)]
    R2 = [[float(T2[i, j]) for j in range(3)] for i in range(3)]; t2 = [float(T2[i, 3]) for i in range(3)]
    fx, fy, cx, cy = float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"])
    R12 = [[R1[i][0] * R2[j][0] + R1[i][1] * R2[j][1] + R1[i][2] * R2[j][2] for j in range(3)] for i in range(3)]
    t12 = [t1[i] - (R12[i][0] * t2[0] + R12[i][1] * t2[1] + R12[i][2] * t2[2]) for i in range(3)]
    E = [[t12[1] * R12[2][j] - t12[2] * R12[1][j] for j in range(3)],
         [t12[2] * R12[0][j] - t12[0] * R12[2][j] for j in range(3)],
         [t12[0] * R12[1][j] - t12[1] * R12[0][j] for j in range(3)]]
    M = [[E[0][j] / fx for j in range(3)], [E[1][j] / fy for j in range(3)], None]
    M[2] = [(E[2][j] - cx * M[0][j]) - cy * M[1][j] for j in range(3)]
    out = []
    for i in range(3):
        f0 = M[i][0] / fx; f1 = M[i][1] / fy
        out += [f0, f1, (M[i][2] - cx * f0) - cy * f1]
    return np.array(out, np.float64).astype(F)


def stereo_cos(b, depth):
    """cos(2 atan2(b / 2, depth)) (:378, :380) as (d^2 - h^2) / (d^2 + h^2)"""
    h = float(b) * 0.5; d = float(depth)
    den = d * d + h * h
    return F((d * d - h * h) / den) if den != 0 else F(np.nan)


def jacobi_smallest4(A32):
    """the right singular vector of the smallest singular value of a 4x4 float matrix: cyclic one-sided Jacobi in f64, pairs (p, q) ascending,
    at most SWEEPS sweeps; among equal singular values the larger column index; -> (float32 [4], the f64 vector, sweeps used)"""
    A = [[float(A32[i][j]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    used = 0
    for sweep in range(SWEEPS):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                a = b = g = 0.0
                for k in range(4):
                    x, y = A[k][p], A[k][q]
                    a = a + x * x; b = b + y * y; g = g + x * y
                if not abs(g) > EPS * math.sqrt(a * b):
                    continue
                rotated = True
                zeta = (b - a) / (2.0 * g)
                tn = math.copysign(1.0, zeta) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                c = 1.0 / math.sqrt(1.0 + tn * tn); s = c * tn
                for M in (A, V):
                    for k in range(4):
                        x, y = M[k][p], M[k][q]
                        M[k][p] = c * x - s * y; M[k][q] = s * x + c * y
        if not rotated:
            break
        used = sweep + 1
    best, wbest = 0, 0.0
    for j in range(4):
        a = 0.0
        for k in range(4):
            a = a + A[k][j] * A[k][j]
        w = math.sqrt(a)
        if j == 0 or w <= wbest:
            best, wbest = j, w
    v64 = np.array([V[k][best] for k in range(4)], np.float64)
    return v64.astype(F), v64, used


def unproject_stereo(cam, T, kp, z):
    """Frame::UnprojectStereo (Frame.cc:958-972): mRwc * x3Dc + mOw"""
    R, t = T[:3, :3], T[:3, 3]
    invfx = F(F(1.0) / F(cam["fx"])); invfy = F(F(1.0) / F(cam["fy"]))
    z = F(z)
    x3 = np.array([F(F(F(F(kp["x"]) - F(cam["cx"])) * z) * invfx), F(F(F(F(kp["y"]) - F(cam["cy"])) * z) * invfy), z], F)
    return mul_add(R.T, x3, neg_rt_mul(R, t))


def _reprojection(cam, T, x3D, z, kp, ur, stereo, sigma2, fault):
    """:428-479 -> (refused, the float sum)"""
    R, t = T[:3, :3], T[:3, 3]
    fx, fy, cx, cy, bf = (F(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    x = F(dot3(R[0], x3D) + float(t[0])); y = F(dot3(R[1], x3D) + float(t[1]))
    invz = F(np.float64(1.0) / np.float64(z))
    u = F(F(F(fx * x) * invz) + cx); v = F(F(F(fy * y) * invz) + cy)
    ex = F(u - F(kp["x"])); ey = F(v - F(kp["y"]))
    if not stereo:
        s = F(F(ex * ex) + F(ey * ey)); lim = 7.8 if fault == "chi2_mono_78" else 5.991
    else:
        er = F(F(u - F(bf * invz)) - F(ur))
        s = F(F(F(ex * ex) + F(ey * ey)) + F(er * er)); lim = 7.8
    if fault == "chi2_float":
        return bool(s > F(F(lim) * F(sigma2))), s
    return bool(float(s) > lim * float(F(sigma2))), s


def triangulate(cam, T1, T2, Ow1, Ow2, kp1, ur1, depth1, kp2, ur2, depth2, fault=None):
    """LocalMapping.cc:352-497 for one match -> (stage code, info dict with x3D, normal1, normal2, dist1, dist2 on a created point)"""
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    invfx = F(F(1.0) / fx); invfy = F(F(1.0) / fy)
    scale = cam["scale"]; sigma2 = [F(s * s) for s in scale]
    st1 = bool(F(ur1) >= 0); st2 = bool(F(ur2) >= 0)
    xn1 = np.array([F(F(F(kp1["x"]) - cx) * invfx), F(F(F(kp1["y"]) - cy) * invfy), F(1.0)], F)
    xn2 = np.array([F(F(F(kp2["x"]) - cx) * invfx), F(F(F(kp2["y"]) - cy) * invfy), F(1.0)], F)
    zero = np.zeros(3, F)
    ray1 = mul_add(T1[:3, :3].T, xn1, zero); ray2 = mul_add(T2[:3, :3].T, xn2, zero)
    n12 = norm3(ray1) * norm3(ray2)
    cos_rays = F(dot3(ray1, ray2) / n12) if n12 != 0 else F(np.nan)
    cs = F(cos_rays + F(1.0)); cs1 = cs2 = cs
    if st1:
        cs1 = stereo_cos(cam["b"], depth1)
    if st2 and (not st1 or fault == "stereo2_cos_always"):                                       # :379: `else if`
        cs2 = stereo_cos(cam["b"], depth2)
    cs = cs2 if cs2 < cs1 else cs1                                                               # std::min(cs1, cs2)
    info = dict(cos_rays=cos_rays, cs1=cs1, cs2=cs2, stereo1=st1, stereo2=st2)
    if cos_rays < cs and cos_rays > 0 and (st1 or st2 or float(cos_rays) < 0.9998):
        A = np.zeros((4, 4), F)
        for j in range(4):
            A[0, j] = F(F(xn1[0] * T1[2, j]) - T1[0, j]); A[1, j] = F(F(xn1[1] * T1[2, j]) - T1[1, j])
            A[2, j] = F(F(xn2[0] * T2[2, j]) - T2[0, j]); A[3, j] = F(F(xn2[1] * T2[2, j]) - T2[1, j])
        v, v64, sweeps = jacobi_smallest4(A)
        info.update(A=A, v=v, v64=v64, sweeps=sweeps)
        if v[3] == 0:
            return W_ZERO, info
        x3D = np.array([F(v[0] / v[3]), F(v[1] / v[3]), F(v[2] / v[3])], F)
        made = BY_SVD
    elif st1 and cs1 < cs2:
        x3D = unproject_stereo(cam, T1, kp1, depth1); made = BY_STEREO1
    elif st2 and cs2 < cs1:
        x3D = unproject_stereo(cam, T2, kp2, depth2); made = BY_STEREO2
    else:
        return LOW_PARALLAX, info
    info["x3D"] = x3D
    behind = (lambda z: z < 0) if fault == "z_lt" else (lambda z: z <= 0)
    z1 = F(dot3(T1[2, :3], x3D) + float(T1[2, 3])); info["z1"] = z1
    if behind(z1):
        return Z1, info
    z2 = F(dot3(T2[2, :3], x3D) + float(T2[2, 3])); info["z2"] = z2
    if behind(z2):
        return Z2, info
    o1, o2 = int(kp1["octave"]), int(kp2["octave"])
    bad, info["chi2_1"] = _reprojection(cam, T1, x3D, z1, kp1, ur1, st1, sigma2[o1], fault)
    if bad:
        return (CHI2_1_STEREO if st1 else CHI2_1_MONO), info
    bad, info["chi2_2"] = _reprojection(cam, T2, x3D, z2, kp2, ur2, st2, sigma2[o2], fault)
    if bad:
        return (CHI2_2_STEREO if st2 else CHI2_2_MONO), info
    normal1 = (x3D - Ow1).astype(F); normal2 = (x3D - Ow2).astype(F)
    dist1 = F(norm3(normal1)); dist2 = F(norm3(normal2))
    info.update(normal1=normal1, normal2=normal2, dist1=dist1, dist2=dist2)
    if dist1 == 0 or dist2 == 0:
        return DIST_ZERO, info
    ratio_dist = F(dist2 / dist1); ratio_octave = F(F(scale[o1]) / F(scale[o2]))
    ratio_factor = F(F(1.5) * F(scale[1] if len(scale) > 1 else 1.0))
    info.update(ratio_dist=ratio_dist, ratio_octave=ratio_octave, ratio_factor=ratio_factor)
    if fault == "ratio_fabs":                                                                    # the commented-out form of :494
        if abs(F(ratio_dist - ratio_octave)) > ratio_factor:
            return RATIO_HIGH, info
    else:
        if F(ratio_dist * ratio_factor) < ratio_octave:
            return RATIO_LOW, info
        if ratio_dist > F(ratio_octave * ratio_factor):
            return RATIO_HIGH, info
    return made, info


def create_new_map_points(cam, tree, levelsup, records, poses, has_point, kf, neigh, key_quality=None, F12=None, kf_order=None, fault=None):
    """One keyframe slot.  records: list of dict(kps, desc, uright, depth); poses: float32 [n_records, 3, 4]; has_point: uint8
    [n_records, nf]; kf: the record; neigh: the neighbour records (-1 = none); key_quality: float32 [n_records, nf] or None; F12: float32
    [max_neigh, 9] or None; kf_order: record indices in std::map order or None.  -> dict(new_point, new_neigh, new_idx2, new_order,
    new_quality, n_new, matches, stage, infos {(rank, idx1): dict})"""
    nf = has_point.shape[1]; n_rec = len(records); mn = len(neigh)
    out = dict(new_point=np.zeros(nf, LOCAL_POINT_DTYPE), new_neigh=np.full(nf, -1, np.int32), new_idx2=np.full(nf, -1, np.int32),
               new_order=np.full(nf, -1, np.int32), new_quality=np.zeros(nf, F), n_new=np.int32(0), matches=np.full((mn, nf), -1, np.int32),
               stage=np.zeros((mn, nf), np.uint8), infos={})
    if not 0 <= kf < n_rec:
        out["n_new"] = np.int32(-1)
        return out
    scale = cam["scale"]; sigma2 = np.array([F(s * s) for s in scale], F)
    r1 = records[kf]; n1 = len(r1["kps"])
    T1 = np.asarray(poses[kf], F).reshape(3, 4)
    Ow1 = neg_rt_mul(T1[:3, :3], T1[:3, 3])
    has1 = [bool(has_point[kf][i]) for i in range(n1)]
    fv1 = feature_vector(tree, r1["desc"], levelsup)
    pos_of = (lambda r: r) if kf_order is None else (lambda r: min([i for i, o in enumerate(kf_order) if o == r] or [2 ** 31 - 1]))
    nnew = 0
    created = []                                                                                 # (rank, idx1) in creation order
    with np.errstate(all="ignore"):
        for rank, nb in enumerate(neigh):
            if not 0 <= nb < n_rec:
                continue
            r2 = records[nb]
            T2 = np.asarray(poses[nb], F).reshape(3, 4)
            Ow2 = neg_rt_mul(T2[:3, :3], T2[:3, 3])
            baseline = F(norm3((Ow2 - Ow1).astype(F)))                                           # :311-313
            if baseline < F(cam["b"]):                                                           # :317
                out["stage"][rank, :n1] = BASELINE
                continue
            f12 = compute_f12(cam, T1, T2) if F12 is None else np.asarray(F12[rank], F)
            C2 = mul_add(T2[:3, :3], Ow1, T2[:3, 3])                                             # ORBmatcher.cc:670-676
            invz = F(F(1.0) / C2[2])
            ex = F(F(F(F(cam["fx"]) * C2[0]) * invz) + F(cam["cx"])); ey = F(F(F(F(cam["fy"]) * C2[1]) * invz) + F(cam["cy"]))
            fv2 = feature_vector(tree, r2["desc"], levelsup)
            m12, _, _, _ = search_for_triangulation(r1["kps"], r1["desc"], has1, r1["uright"] >= 0, fv1, r2["kps"], r2["desc"],
                                                    [bool(x) for x in has_point[nb][:len(r2["kps"])]], r2["uright"] >= 0, fv2, f12, ex, ey, scale,
                                                    sigma2, False, False, fault="first_minimum" if fault == "first_minimum" else None)
            out["matches"][rank, :n1] = m12
            first = kf if (pos_of(kf), kf) <= (pos_of(nb), nb) else nb
            if fault == "desc_ignores_order":
                first = kf
            for idx1 in range(n1):                                                               # vMatchedIndices: idx1 ascending (:821-826)
                idx2 = int(m12[idx1])
                if idx2 < 0:
                    continue
                code, info = triangulate(cam, T1, T2, Ow1, Ow2, r1["kps"][idx1], r1["uright"][idx1], r1["depth"][idx1], r2["kps"][idx2],
                                         r2["uright"][idx2], r2["depth"][idx2], fault)
                out["stage"][rank, idx1] = code; out["infos"][(rank, idx1)] = info
                if code < BY_SVD:
                    if fault == "has1_updated_on_failure":
                        has1[idx1] = True
                    continue
                mp = out["new_point"][idx1]
                o1 = int(r1["kps"]["octave"][idx1])
                mp["pos"] = info["x3D"]
                u1 = np.array([F(info["normal1"][i] / info["dist1"]) for i in range(3)], F)
                u2 = np.array([F(info["normal2"][i] / info["dist2"]) for i in range(3)], F)
                mp["normal"] = np.array([F(F(u1[i] + u2[i]) * F(0.5)) for i in range(3)], F)       # MapPoint.cc:353-374, n = 2
                mp["max_distance"] = F(info["dist1"] * F(scale[o1]))                             # :372
                mp["min_distance"] = F(mp["max_distance"] / F(scale[o1 if fault == "min_distance_octave" else len(scale) - 1]))   # :373
                mp["desc"] = r1["desc"][idx1] if first == kf else r2["desc"][idx2]               # MapPoint.cc:292-306: row 0 of vDescriptors
                mp["flags"] = 2
                out["new_neigh"][idx1] = rank; out["new_idx2"][idx1] = idx2; out["new_order"][idx1] = nnew
                q = F(1.0)
                if key_quality is not None:
                    qa, qb = F(key_quality[kf][idx1]), F(key_quality[nb][idx2])
                    q = (qa if qb < qa else qb) if fault == "quality_max" else (qb if qb < qa else qa)      # std::min (:513-516)
                out["new_quality"][idx1] = q
                created.append((rank, idx1))
                nnew += 1
                if fault != "has1_not_updated":
                    has1[idx1] = True                                                            # AddMapPoint(pMP, idx1) (:505)
    if fault == "order_by_idx1":
        for n, (_, idx1) in enumerate(sorted(created, key=lambda c: c[1])):
            out["new_order"][idx1] = n
    out["n_new"] = np.int32(nnew)
    return out


KEYS = ("new_point", "new_neigh", "new_idx2", "new_order", "new_quality", "n_new", "matches", "stage")


def same(a, b):
    """the first output that differs byte for byte, or None"""
    for k in KEYS:
        if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes():
            return k
    return None
