"""ransac_ref.py -- what tests/pnp_ref.py (PnPsolver, 4 points per sample) and tests/sim3_ref.py (Sim3Solver, 3) share (test infrastructure
only): DUtils::Random::RandomInt on a given rand() value, the sampling loop (PnPsolver.cc:192-205, Sim3Solver.cc:166-180), draws that make it
return wanted indices, the tail of SetRansacParameters (PnPsolver.cc:148-156, Sim3Solver.cc:130-138), mvLevelSigma2.  Device: ivf_solve.h."""
import math

import numpy as np

D = np.float64
F = np.float32
RAND_MAX = 2147483647


def level_sigma2(scale):
    s = np.asarray(scale, F)
    return (s * s).astype(F)


def random_int(r, lo, hi):
    """DUtils::Random::RandomInt on the value r that rand() returned"""
    d = hi - lo + 1
    return int((float(int(r) & RAND_MAX) / (RAND_MAX + 1.0)) * d) + lo


def sample_indices(N, draws, k, mis=()):
    """transcribed: the available indices, k times RandomInt, swap with the back, pop; mis = {"no_swap"}: erased in order instead"""
    avail = list(range(N))
    out = []
    for i in range(k):
        randi = random_int(draws[i], 0, len(avail) - 1)
        out.append(avail[randi])
        if "no_swap" in mis:
            avail.pop(randi)
        else:
            avail[randi] = avail[-1]
            avail.pop()
    return out


def draws_for(N, wanted):
    """the rand() values under which sample_indices(N, ., len(wanted)) returns `wanted` (distinct indices): the middle of each RandomInt bin"""
    avail = list(range(N))
    out = []
    for w in wanted:
        randi = avail.index(w)
        r = int((randi + 0.5) * (RAND_MAX + 1.0) / len(avail))
        assert random_int(r, 0, len(avail) - 1) == randi
        out.append(r)
        avail[randi] = avail[-1]
        avail.pop()
    return np.array(out, np.uint32)


def iteration_count(probability, eps, all_inliers, max_iterations):
    """-> (mRansacMaxIts, x) for the float `eps`; all_inliers: mRansacMinInliers == N; x = the real number whose ceil is taken (None where
    there is none).  numpy's log: eps = 0 gives log(1) = 0 and x = -inf, where math.log raises"""
    if all_inliers:
        return 1, None
    with np.errstate(all="ignore"):
        x = D(math.log(1 - probability)) / np.log(D(1) - D(math.pow(float(eps), 3)))
    its = int(max_iterations) if not x < max_iterations else 1 if x < 1.0 else int(math.ceil(x))
    return max(1, min(its, int(max_iterations))), float(x)
