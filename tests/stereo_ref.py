"""stereo_ref.py -- TEST-SIDE RESTATEMENT (test infrastructure only) of Frame::ComputeStereoMatches (ORB/src/Frame.cc:758-932), written
from the reference's Frame.cc and not from oracle/ivf_oracle.c or the kernel.  Float variables of the source are np.float32 and every
operation on them is rounded to float32 in the source's order; int variables are Python ints; `uL-0.01` is computed in double and then
narrowed (Frame.cc:909).  Besides mvuRight / mvDepth it reports, for every left keypoint, the step at which it ended (STAGES).

Where the reference's behaviour is undefined, the restatement gives the library's frozen answer and says so:
  * a SAD window that leaves its pyramid level (cv::Mat::rowRange / colRange throw): stage `outside_domain`, result -1;
  * vRowIndices[yi] with yi outside [0, rows) (Frame.cc:784 writes outside the vector): the band is clamped to the image's rows;
  * vRowIndices[vL] with (int)vL outside [0, rows): stage `outside_domain`, result -1;
  * an empty vDistIdx (Frame.cc:919 reads element 0 of an empty vector): no gate;
  * deltaR = 0/0 (three equal distances): NaN passes `deltaR<-1 || deltaR>1` and fails `disparity>=minD`: stage `disparity`.
"""
import numpy as np

F = np.float32
STAGES = ("no_candidates", "hamming", "right_border", "outside_domain", "edge_inc", "delta", "disparity", "gated", "matched")
TH_HIGH, TH_LOW = 100, 50                                     # ORBmatcher.h
INT_MAX = 2147483647
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance: the number of differing bits of two 32-byte descriptors (b may be [n][32])"""
    return _POP[np.bitwise_xor(a, b)].sum(axis=-1)


def _round(x):
    """C round() on a float: half away from zero (np.round is half to even)"""
    x = float(x)
    return F(np.floor(x + 0.5) if x >= 0 else -np.floor(-x + 0.5))


def _window(plane, r0, r1, c0, c1):
    """plane.rowRange(r0, r1).colRange(c0, c1) as float32, or None where OpenCV would throw"""
    if r0 < 0 or c0 < 0 or r1 > plane.shape[0] or c1 > plane.shape[1] or r0 > r1 or c0 > c1:
        return None
    win = plane[r0:r1, c0:c1].astype(F)
    return win - win[5, 5] * np.ones_like(win)


def stereo_match(pyr_left, pyr_right, scale, inv_scale, kps_left, desc_left, kps_right, desc_right, bf, b, th_orb_dist=None, tie_last=False):
    """-> dict(uright, depth: float32 [N]; stage: list of STAGES names; sad, iR, bestinc: int [N], -1 / 0 where the step was not reached;
    delta: float32 [N]).  pyr_left / pyr_right: the planes of mvImagePyramid; scale / inv_scale: mvScaleFactors / mvInvScaleFactors.
    th_orb_dist and tie_last exist for the tests' own strength checks (a deliberately wrong restatement must fail them)."""
    N = len(kps_left)
    mvuRight = np.full(N, -1.0, F)
    mvDepth = np.full(N, -1.0, F)
    stage = ["no_candidates"] * N
    sad = np.full(N, -1, np.int64); win_iR = np.full(N, -1, np.int64); binc = np.zeros(N, np.int64); dlt = np.zeros(N, F)
    bf = F(bf); b = F(b)
    desc_left = np.asarray(desc_left, np.uint8).reshape(-1, 32); desc_right = np.asarray(desc_right, np.uint8).reshape(-1, 32)

    thOrbDist = (TH_HIGH + TH_LOW) // 2 if th_orb_dist is None else th_orb_dist
    nRows = pyr_left[0].shape[0]

    vRowIndices = [[] for _ in range(nRows)]
    Nr = len(kps_right)
    xR = kps_right["x"]; yR = kps_right["y"]; oR = kps_right["octave"]
    for iR in range(Nr):
        kpY = F(yR[iR])
        r = F(F(2.0) * scale[oR[iR]])
        maxr = int(np.ceil(F(kpY + r)))
        minr = int(np.floor(F(kpY - r)))
        for yi in range(max(minr, 0), min(maxr, nRows - 1) + 1):            # undefined outside [0, nRows): clamped
            vRowIndices[yi].append(iR)

    minZ = b
    minD = F(0)
    maxD = F(bf / minZ)

    vDistIdx = []
    with np.errstate(all="ignore"):
        for iL in range(N):
            levelL = int(kps_left["octave"][iL])
            vL = F(kps_left["y"][iL]); uL = F(kps_left["x"][iL])
            row = int(vL)
            if row < 0 or row >= nRows:
                stage[iL] = "outside_domain"
                continue
            vCandidates = vRowIndices[row]
            if not vCandidates:
                continue
            minU = F(uL - maxD)
            maxU = F(uL - minD)
            if maxU < 0:
                continue

            bestDist = TH_HIGH
            bestIdxR = 0
            cand = np.asarray(vCandidates, np.int64)
            dists = descriptor_distance(desc_left[iL], desc_right[cand])
            for iC in range(len(cand)):
                iR = int(cand[iC])
                if oR[iR] < levelL - 1 or oR[iR] > levelL + 1:
                    continue
                uR = F(xR[iR])
                if uR >= minU and uR <= maxU:
                    dist = int(dists[iC])
                    if dist < bestDist or (tie_last and dist == bestDist and dist < TH_HIGH):
                        bestDist = dist
                        bestIdxR = iR

            stage[iL] = "hamming"
            if not bestDist < thOrbDist:
                continue
            win_iR[iL] = bestIdxR
            uR0 = F(xR[bestIdxR])
            scaleFactor = F(inv_scale[levelL])
            scaleduL = _round(F(uL * scaleFactor))
            scaledvL = _round(F(vL * scaleFactor))
            scaleduR0 = _round(F(uR0 * scaleFactor))

            w = 5
            r0 = int(F(scaledvL - w)); r1 = int(F(scaledvL + w + 1))
            IL = _window(pyr_left[levelL], r0, r1, int(F(scaleduL - w)), int(F(scaleduL + w + 1)))
            if IL is None:
                stage[iL] = "outside_domain"
                continue

            bestDistS = INT_MAX
            bestincR = 0
            L = 5
            vDists = np.zeros(2 * L + 1, F)

            iniu = F(scaleduR0 + L - w)
            endu = F(scaleduR0 + L + w + 1)
            if iniu < 0 or endu >= pyr_right[levelL].shape[1]:
                stage[iL] = "right_border"
                continue

            outside = False
            for incR in range(-L, L + 1):
                IR = _window(pyr_right[levelL], r0, r1, int(F(scaleduR0 + incR - w)), int(F(scaleduR0 + incR + w + 1)))
                if IR is None:
                    outside = True
                    break
                dist = F(np.abs(IL.astype(np.float64) - IR.astype(np.float64)).sum())      # cv::norm accumulates in double
                if dist < F(bestDistS):
                    bestDistS = int(dist)
                    bestincR = incR
                vDists[L + incR] = dist
            if outside:
                stage[iL] = "outside_domain"
                continue
            binc[iL] = bestincR

            if bestincR == -L or bestincR == L:
                stage[iL] = "edge_inc"
                continue

            dist1 = vDists[L + bestincR - 1]
            dist2 = vDists[L + bestincR]
            dist3 = vDists[L + bestincR + 1]
            deltaR = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))
            dlt[iL] = deltaR
            if deltaR < -1 or deltaR > 1:
                stage[iL] = "delta"
                continue

            bestuR = F(scale[levelL] * F(F(F(scaleduR0) + F(bestincR)) + deltaR))
            disparity = F(uL - bestuR)
            if disparity >= minD and disparity < maxD:
                if disparity <= 0:
                    disparity = F(0.01)
                    bestuR = F(np.float64(uL) - 0.01)
                mvDepth[iL] = F(bf / disparity)
                mvuRight[iL] = bestuR
                vDistIdx.append((bestDistS, iL))
                sad[iL] = bestDistS
                stage[iL] = "matched"
            else:
                stage[iL] = "disparity"

    if vDistIdx:                                                              # undefined when empty: no gate
        vDistIdx.sort()
        median = F(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F(F(F(1.5) * F(1.4)) * median)
        for i in range(len(vDistIdx) - 1, -1, -1):
            if F(vDistIdx[i][0]) < thDist:
                break
            mvuRight[vDistIdx[i][1]] = -1
            mvDepth[vDistIdx[i][1]] = -1
            stage[vDistIdx[i][1]] = "gated"
    return dict(uright=mvuRight, depth=mvDepth, stage=stage, sad=sad, iR=win_iR, bestinc=binc, delta=dlt)
