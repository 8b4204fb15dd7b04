"""The yardstick of ivf_tracker_optimize_pose checked on its own: tests/pose_opt_ref.py, the f64 numpy restatement of
Optimizer::PoseOptimization (ORB/src/Optimizer.cc:251-503) -- g2o itself cannot be built without Eigen.  No GPU.

tests/golden/pose_opt_noise.json is the restatement's own noise floor for every scenario of tests/pose_opt_scenes.py: the largest
difference between its float poses under 8 random orders of the sums over edges (rotation angle; translation relative to max(|t|, 1)),
and the edges whose chi2 comes within that noise of the threshold they are classified against.  It is data, written by
    python tests/test_pose_opt_cpu.py --write
and checked here against a fresh computation.  `floor` = max(measured spread, sqrt(3) * 2^-23): the pose leaves as float, so two double
results arbitrarily close to each other may land on neighbouring floats in each of three unit-magnitude components; the measured spread of
most scenarios is exactly 0 and cannot express that quantum."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_opt_ref as PR
import pose_opt_scenes as S

NOISE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_opt_noise.json")
QUANTUM = float(np.sqrt(3.0) * 2.0 ** -23)
# observations are float: at u ~ 1000 px one float ulp is 6e-5 px, an angle of 6e-5 / fx ~ 1e-7 rad; ten times that
GT_BOUND = 1e-6


def measure():
    out = {}
    for name, sc in S.scenarios().items():
        rot = tr = gt_rot = gt_tr = 0.0
        border = {}
        n_edges = 0
        for k, fr in enumerate(sc["frames"]):
            base, r, t, b = S.spread_and_borderline(fr, sc["n_rounds"])
            rot = max(rot, r); tr = max(tr, t)
            n_edges += len(base["edges"])
            if b:
                border[str(k)] = b
            if fr["noise_free"] and len(base["edges"]) >= 3:
                g = PR.pose_difference(base["pose"], fr["pose_gt"])
                gt_rot = max(gt_rot, g[0]); gt_tr = max(gt_tr, g[1])
        out[name] = dict(spread_rot=rot, spread_trans=tr, floor_rot=max(rot, QUANTUM), floor_trans=max(tr, QUANTUM), borderline=border,
                         n_edges=n_edges, gt_rot=gt_rot, gt_trans=gt_tr, noise_free=all(fr["noise_free"] for fr in sc["frames"]))
    return out


@pytest.fixture(scope="module")
def measured():
    return measure()


def test_noise_floor_file_is_current_and_under_the_cap(measured):
    """the committed floor covers a fresh measurement; at most 1 % of a scenario's edges are borderline, none in a noise-free one"""
    gold = json.load(open(NOISE_PATH))
    assert sorted(gold) == sorted(measured)
    for name, m in measured.items():
        g = gold[name]
        assert m["spread_rot"] <= g["floor_rot"] and m["spread_trans"] <= g["floor_trans"], (name, m, g)
        assert g["floor_rot"] >= QUANTUM and g["floor_trans"] >= QUANTUM
        assert g["borderline"] == m["borderline"], name
        nb = sum(len(v) for v in g["borderline"].values())
        assert nb <= 0.01 * g["n_edges"], "%s: %d of %d edges are borderline" % (name, nb, g["n_edges"])
        if g["noise_free"]:
            assert nb == 0, name
        assert m["gt_rot"] <= g["gt_rot"] * (1 + 1e-9) + 1e-30 and m["gt_trans"] <= g["gt_trans"] * (1 + 1e-9) + 1e-30


def test_noise_free_scenes_recover_the_pose_and_the_planted_outliers(measured):
    n = 0
    for name, sc in S.scenarios().items():
        for fr in sc["frames"]:
            if not fr["noise_free"]:
                continue
            r = S.reference(fr, sc["n_rounds"])
            ne = int(fr["has"].sum())
            if ne < 3:
                assert r["ninliers"] == 0 and r["pose"].tobytes() == fr["pose_in"].tobytes() and not r["outlier"].any()
                continue
            rot, tr = PR.pose_difference(r["pose"], fr["pose_gt"])
            assert rot < GT_BOUND and tr < GT_BOUND, (name, ne, rot, tr)
            assert np.array_equal(r["outlier"][:fr["n"]], fr["planted"]), name
            assert r["ninliers"] == ne - int(fr["planted"].sum())
            n += 1
    assert n >= 6


def test_gradient_vanishes_at_the_solution():
    """b = -J^T W e over the last round's level-0 edges.  Noise-free scene: the residuals left are the float rounding of the observations
    (~3e-5 px against ~40 px at the prior), so b falls by six orders of magnitude and the Gauss-Newton step H^-1 b is below the 1e-6 of GT_BOUND; noisy
    scene: LM stops on its 0.1 % rule (levenberg.cpp:154-161), with the Gauss-Newton step below 1e-3"""
    fr = S.make_frame(701, 200, 150, "mixed", 0.0, 12, prior=(0.2, 3.0))
    r = S.reference(fr, 4)
    E = PR.Edges(fr["kps"], fr["n"], fr["uright"], S.INV_SIGMA2, *(S.CAM[k] for k in ("fx", "fy", "cx", "cy", "bf")), fr["xw"], fr["has"], None)
    act = r["outlier"][r["edges"]] == 0
    _, b0, _ = PR.build_system(E, PR.se3_from_pose(fr["pose_in"]), act, False, list(range(len(act))))
    assert np.abs(r["b"]).max() < 1e-6 * np.abs(b0).max()
    H, b, _ = PR.build_system(E, r["pose64"], act, False, list(range(len(act))))
    x, ok = PR.ldlt_solve(H, b)
    print("Gauss-Newton step at the noise-free solution", np.abs(x).max())
    assert ok and np.abs(x).max() < GT_BOUND
    fr = S.make_frame(702, 200, 150, "mixed", 1.0, 12, prior=(0.2, 3.0))
    r = S.reference(fr, 4)
    E = PR.Edges(fr["kps"], fr["n"], fr["uright"], S.INV_SIGMA2, *(S.CAM[k] for k in ("fx", "fy", "cx", "cy", "bf")), fr["xw"], fr["has"], None)
    act = r["outlier"][r["edges"]] == 0
    H, b, _ = PR.build_system(E, r["pose64"], act, False, list(range(len(act))))
    x, ok = PR.ldlt_solve(H, b)
    assert ok and np.abs(x).max() < 1e-3
    assert np.allclose(np.array(H, float) @ np.array(x, float), np.array(b, float), rtol=1e-9, atol=1e-9 * np.abs(b).max())   # the LDLT restatement solves


def test_quality_below_one_downweights_the_points_it_marks():
    """a third of the edges carry a +2.5 px bias in x; with their quality at 0.2 the Huber width shrinks to a fifth (Optimizer.cc:342,
    :380) and the solution of the robust round moves towards the truth, in rotation and in translation.  n_rounds = 1: the kernels are never dropped."""
    for seed in (711, 712, 713):
        a = S.make_frame(seed, 200, 180, "mixed", 0.0, 0, prior=(0.05, 0.5), biased=60)
        b = S.make_frame(seed, 200, 180, "mixed", 0.0, 0, prior=(0.05, 0.5), biased=60, quality="biased")
        assert a["kps"].tobytes() == b["kps"].tobytes() and a["quality"] is None and (b["quality"] < 1).sum() == 60
        ra = S.reference(a, 1); rb = S.reference(b, 1)
        ea = PR.pose_difference(ra["pose"], a["pose_gt"]); eb = PR.pose_difference(rb["pose"], b["pose_gt"])
        assert eb[0] < ea[0] and eb[1] < ea[1], (seed, ea, eb)
    # quality 1 everywhere is the same as none
    fr = S.make_frame(714, 64, 60, "mixed", 1.0, 5)
    r0 = S.reference(fr, 4); fr["quality"] = np.ones(64, np.float32); r1 = S.reference(fr, 4)
    assert r0["pose"].tobytes() == r1["pose"].tobytes() and np.array_equal(r0["outlier"], r1["outlier"])


def test_summation_order_is_the_only_thing_a_permutation_changes():
    fr = S.make_frame(721, 64, 50, "mixed", 1.0, 4)
    r0 = S.reference(fr, 4); r1 = S.reference(fr, 4, perm=np.arange(50)); r2 = S.reference(fr, 4, perm=np.arange(50)[::-1])
    assert r0["pose"].tobytes() == r1["pose"].tobytes() and np.array_equal(r0["chi2"], r1["chi2"])
    assert PR.pose_difference(r2["pose"], r0["pose"])[0] < 1e-6 and np.array_equal(r2["outlier"], r0["outlier"])


if __name__ == "__main__":
    if "--write" in sys.argv:
        os.makedirs(os.path.dirname(NOISE_PATH), exist_ok=True)
        with open(NOISE_PATH, "w") as f:
            json.dump(measure(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", NOISE_PATH)
