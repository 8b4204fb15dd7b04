"""track_bow_ref.py -- numpy restatement of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORB/src/ORBmatcher.cc:165-294)
and of the part of Frame::ComputeBoW it reads (mFeatVec), test infrastructure only.  Besides the assignment it says, per keyframe
feature, where the feature left the loop: the scenes of tests/track_bow_scenes.py are built to reach every such exit, and
tests/test_track_bow_cpu.py checks through these codes that they still do."""
import numpy as np

F = np.float32
# outcome of one keyframe feature
NO_POINT, NODE_ABSENT, ALL_CLAIMED, OVER_TH_LOW, RATIO_FAILED, ACCEPTED, ROT_REMOVED, NOT_IN_VECTOR = range(8)
OUTCOME_NAMES = ["no map point", "node absent in the frame", "every candidate claimed", "over TH_LOW", "ratio failed", "accepted",
                 "accepted, removed by the rotation filter", "stopped word: in no node"]
REQUIRED = (NO_POINT, NODE_ABSENT, ALL_CLAIMED, OVER_TH_LOW, RATIO_FAILED, ACCEPTED, ROT_REMOVED)
TH_LOW, HISTO_LENGTH = 50, 30


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def feature_vector(node_id, weight):
    """mFeatVec as {node: [feature indices ascending]}: TemplatedVocabulary::transform adds a feature when its word's weight is > 0
    (TemplatedVocabulary.h:1157), FeatureVector::addFeature pushes in feature order (FeatureVector.cpp:31-45)"""
    fv = {}
    for i, (nd, w) in enumerate(zip(node_id, weight)):
        if w > 0:
            fv.setdefault(int(nd), []).append(i)
    return fv


def three_maxima(sizes):
    """ComputeThreeMaxima (ORBmatcher.cc:1654-1695) on the bin sizes"""
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


def c_round(x):
    """round() of <cmath> on a float: halves away from zero"""
    x = float(x)
    return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def search_by_bow(kf_kps, kf_desc, kf_has, kf_fv, f_kps, f_desc, f_fv, nn_ratio=0.7, check_orientation=True):
    """-> (vpMapPointMatches as keyframe keypoint index per frame keypoint or -1, nmatches, outcome code per keyframe keypoint,
    negative_rot: accepted matches whose rot was negative before the + 360)"""
    n_kf, n_f = len(kf_kps), len(f_kps)
    match = np.full(n_f, -1, np.int32)
    outcome = np.full(n_kf, NOT_IN_VECTOR, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = F(1.0) / F(HISTO_LENGTH)
    nn = F(nn_ratio)
    nmatches = 0
    negative_rot = 0
    kn, fn = sorted(kf_fv), sorted(f_fv)
    for nd in kn:
        for i in kf_fv[nd]:
            outcome[i] = NODE_ABSENT if kf_has[i] else NO_POINT
    a = b = 0
    while a < len(kn) and b < len(fn):                                       # :186-270
        if kn[a] == fn[b]:
            for i_kf in kf_fv[kn[a]]:
                if not kf_has[i_kf]:
                    continue                                                     # :199-203
                best1, best_idx, best2, seen = 256, -1, 256, 0
                for i_f in f_fv[fn[b]]:
                    if match[i_f] >= 0:
                        continue                                                 # :215
                    seen += 1
                    d = hamming(kf_desc[i_kf], f_desc[i_f])
                    if d < best1:
                        best2, best1, best_idx = best1, d, i_f
                    elif d < best2:
                        best2 = d
                if seen == 0:
                    outcome[i_kf] = ALL_CLAIMED
                elif best1 > TH_LOW:
                    outcome[i_kf] = OVER_TH_LOW
                elif not (F(best1) < nn * F(best2)):
                    outcome[i_kf] = RATIO_FAILED
                else:
                    outcome[i_kf] = ACCEPTED
                    match[best_idx] = i_kf
                    if check_orientation:
                        rot = F(kf_kps["angle"][i_kf]) - F(f_kps["angle"][best_idx])
                        if rot < 0.0:
                            rot = F(rot + F(360.0)); negative_rot += 1
                        bn = c_round(F(rot * factor))
                        if bn == HISTO_LENGTH:
                            bn = 0
                        assert 0 <= bn < HISTO_LENGTH
                        rot_hist[bn].append(best_idx)
                    nmatches += 1
            a += 1; b += 1
        elif kn[a] < fn[b]:
            while a < len(kn) and kn[a] < fn[b]:                                 # lower_bound (:264)
                a += 1
        else:
            while b < len(fn) and fn[b] < kn[a]:                                 # lower_bound (:268)
                b += 1
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for j in rot_hist[i]:
                outcome[match[j]] = ROT_REMOVED
                match[j] = -1
                nmatches -= 1
    return match, nmatches, outcome, negative_rot
