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


class Reach:
    """what the restatement ran, recorded by wrapping its functions in place (they look each other up in the module at call time).  A trial
    is one ldlt_solve; an LM iteration is one build_system followed by its trials, so the trial loop's exit is the number of solves between
    two build_system calls: more than one = a rejected trial, ten = maxTrialsAfterFailure exhausted (levenberg.cpp:149-152)."""
    NAMES = ("quat_from_rot", "quat_normalize_rotation", "ldlt_solve", "se3_exp", "build_system")

    def __init__(self):
        self.quat = {"trace": 0, 0: 0, 1: 0, 2: 0}
        self.flips = self.solves = self.failed = self.rejected = self.exhausted = self.exp_small = self.exp_large = 0
        self._trials = 0
        self._orig = {}

    def _close_iteration(self):
        self.rejected += max(self._trials - 1, 0)
        self.exhausted += self._trials == 10
        self._trials = 0

    def __enter__(self):
        o = self._orig = {n: getattr(PR, n) for n in self.NAMES}

        def quat_from_rot(m):
            if m[0][0] + m[1][1] + m[2][2] > 0.0:
                self.quat["trace"] += 1
            else:
                i = 1 if m[1][1] > m[0][0] else 0
                self.quat[2 if m[2][2] > m[i][i] else i] += 1
            return o["quat_from_rot"](m)

        def quat_normalize_rotation(q):
            self.flips += q[3] < 0
            return o["quat_normalize_rotation"](q)

        def ldlt_solve(A, b):
            x, ok = o["ldlt_solve"](A, b)
            self.solves += 1; self.failed += not ok; self._trials += 1
            return x, ok

        def se3_exp(u):
            theta = float(np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))
            self.exp_small += theta < 0.00001; self.exp_large += not theta < 0.00001
            return o["se3_exp"](u)

        def build_system(*a):
            self._close_iteration()
            return o["build_system"](*a)

        for n, f in dict(quat_from_rot=quat_from_rot, quat_normalize_rotation=quat_normalize_rotation, ldlt_solve=ldlt_solve, se3_exp=se3_exp,
                         build_system=build_system).items():
            setattr(PR, n, f)
        return self

    def __exit__(self, *exc):
        self._close_iteration()
        for n, f in self._orig.items():
            setattr(PR, n, f)


def points_behind_the_input_pose(fr):
    T = fr["pose_in"].astype(np.float64).reshape(3, 4)
    z = fr["xw"].astype(np.float64) @ T[2, :3] + T[2, 3]
    return int((z[fr["has"][:fr["n"]] != 0] < 0).sum())


def test_scenarios_reach_every_branch_of_the_restatement():
    """every branch the kernel transcribes is run by some scenario, so by the GPU test of that scenario: the four cases of
    Quaterniond(Matrix3d), normalizeRotation's sign flip, a failed LDLT, a rejected trial, ten trials exhausted, both branches of
    SE3Quat::exp, a point behind the camera at the input pose.  The scenarios before the half turns reach none of the first four lines."""
    total = Reach()
    behind = 0
    per = {}
    for name, sc in S.scenarios().items():
        with Reach() as r:
            for fr in sc["frames"]:
                S.reference(fr, sc["n_rounds"])
        per[name] = r
        behind += sum(points_behind_the_input_pose(fr) for fr in sc["frames"])
        for k in r.quat:
            total.quat[k] += r.quat[k]
        for k in ("flips", "solves", "failed", "rejected", "exhausted", "exp_small", "exp_large"):
            setattr(total, k, getattr(total, k) + getattr(r, k))
    print("quaternion branches", total.quat, "flips", total.flips, "solves", total.solves, "failed", total.failed, "rejected trials", total.rejected,
          "exhausted", total.exhausted, "exp small / large", total.exp_small, total.exp_large, "points behind", behind)
    assert total.quat["trace"] > 0 and total.quat[0] > 0 and total.quat[1] > 0 and total.quat[2] > 0, total.quat
    assert total.flips > 0 and total.failed > 0 and total.rejected > 0 and total.exhausted > 0
    assert total.exp_small > 0 and total.exp_large > 0 and behind > 0
    # and where: the scenario that was written for a branch still reaches it
    for name in ("half_turn_clean", "half_turn_noisy", "exact_axis_poses"):
        q = per[name].quat
        assert q[0] > 0 and q[1] > 0 and q[2] > 0 and per[name].flips > 0, (name, q)
    assert per["branch_boundary"].quat["trace"] > 0 and per["branch_boundary"].quat[1] > 0
    nq = per["negative_quality"]
    assert nq.failed > 0 and nq.rejected > 0 and nq.exp_small > 0
    q = per["conversion_only"].quat
    assert q["trace"] > 0 and q[0] > 0 and q[1] > 0 and q[2] > 0 and per["conversion_only"].flips > 0 and per["conversion_only"].exp_large == 0
    assert per["counts64_clean"].exhausted > 0 and per["half_turn_noisy"].exhausted > 0      # qmax == 10: a converged estimate rejects ten trials
    assert sum(points_behind_the_input_pose(fr) for fr in S.scenarios()["behind_camera"]["frames"]) == 6


def test_negative_quality_fails_solves_and_leaves_the_pose():
    """quality -1 makes the Huber width and with it rho[1] = delta / sqrt(chi2) negative on 30 of 40 edges: H + lambda I is not positive,
    LinearSolverDense reports failure, x stays what it was and tempChi = DBL_MAX (levenberg.cpp:126-127).  Traced with this seed: the
    first six solves of round 0 fail and are rejected, the seventh (lambda grown 2^21-fold) succeeds, and from there each of the ten
    iterations accepts its first trial, "descending" a robust chi2 that is negative (-1570 -> -49249) while the estimate walks more than
    0.3 rad away from the input.  Every edge is an outlier there, so rounds 1-3, which restart from the input pose (Optimizer.cc:418),
    have no level-0 edge, a zero system and a zero step: the output is the input pose, to the bit, with 0 inliers.  Ten trials are not
    exhausted here; the reach test names the scenarios that do that."""
    fr = S.scenarios()["negative_quality"]["frames"][0]
    assert (fr["quality"][fr["has"] != 0] == -1).sum() == 30 and (fr["quality"][fr["has"] != 0] == 1).sum() == 10
    with Reach() as r:
        ref = S.reference(fr, 4)
    print("negative quality: solves", r.solves, "failed", r.failed, "iterations", ref["iterations"], "inliers", ref["ninliers"])
    assert r.failed > 0 and r.rejected > 0 and ref["iterations"] == [10, 1, 1, 1]
    assert ref["pose"].tobytes() == fr["pose_in"].tobytes() and ref["ninliers"] == 0 and ref["outlier"][fr["has"] != 0].all()


def test_conversion_only_scenario_returns_the_converted_input_pose():
    """quality 0 everywhere, one round: no weight, no step, and the pose that leaves is the input through Converter::toSE3Quat and
    Converter::toCvMat and nothing else.  For each case i = 0, 1, 2 of Quaterniond(Matrix3d) there are frames about a single axis with
    |w| > 0.35 and frames about a generic axis whose four quaternion components all exceed 0.17 in magnitude, both signs of w before
    normalizeRotation: one wrong sign or index in a case is a pose tens of degrees off, with no optimiser to repair it."""
    sc = S.scenarios()["conversion_only"]
    flags = 0
    generic = {0: 0, 1: 0, 2: 0}
    for fr in sc["frames"]:
        assert not fr["quality"].any()
        with Reach() as r:
            ref = S.reference(fr, sc["n_rounds"])
        q, t = PR.se3_from_pose(fr["pose_in"])
        assert ref["iterations"] == [1] and ref["pose"].tobytes() == PR.pose_from_se3(q, t).tobytes()
        assert PR.pose_difference(ref["pose"], fr["pose_in"])[0] < 4 * QUANTUM
        flags += int(ref["outlier"].sum())
        for i in (0, 1, 2):
            if r.quat[i] and min(abs(v) for v in q) > 0.17:
                assert abs(q[i]) == max(abs(v) for v in q)
                generic[i] += 1
    assert min(abs(PR.se3_from_pose(fr["pose_in"])[0][3]) for fr in sc["frames"][:6]) > 0.35
    assert all(v >= 2 for v in generic.values()), generic
    assert 0 < flags < sum(int(fr["has"].sum()) for fr in sc["frames"])


def test_has_point_past_the_count_is_ignored_by_the_restatement():
    fr = S.scenarios()["has_past_count"]["frames"][0]
    assert fr["n"] == 50 and fr["has_tail"] == 1
    a = S.reference(fr, 4)
    b = S.reference(dict(fr, has=np.concatenate([fr["has"], np.ones(14, np.uint8)]), xw=np.concatenate([fr["xw"], np.ones((14, 3), np.float32)])), 4)
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["ninliers"] == b["ninliers"] and not b["outlier"][50:].any() and not b["chi2"][50:].any()


def test_rotation_to_quaternion_and_back_is_the_rotation():
    """the yardstick's own conversion checked without the kernel: Quaterniond(Matrix3d) -> normalizeRotation -> toRotationMatrix returns the
    matrix, for 2000 rotations of 100..180 degrees about random axes (all of Quaterniond's cases) and the six exact matrices of
    exact_axis_poses.  Each step is a handful of double operations on unit-magnitude numbers: measured 1.3e-15, bound 1e-14."""
    rng = np.random.default_rng(11)
    mats = [S.rot(rng.normal(size=3), d) for d in rng.uniform(100, 180, 2000)]
    mats += [fr["pose_gt"].reshape(3, 4)[:, :3] for fr in S.scenarios()["exact_axis_poses"]["frames"][::2]]
    assert len(mats) == 2006
    worst = 0.0
    with Reach() as r:
        for m in mats:
            q = PR.quat_normalize_rotation(PR.quat_from_rot([[np.float64(v) for v in row] for row in m]))
            assert q[3] >= 0 and abs(sum(v * v for v in q) - 1.0) < 1e-14
            worst = max(worst, float(np.abs(np.array(PR.quat_to_rot(q), np.float64) - m).max()))
    print("rotation -> quaternion -> rotation: worst entry", worst, "branches", r.quat, "flips", r.flips)
    assert worst <= 1e-14
    assert all(v > 0 for v in r.quat.values()) and r.flips > 0


if __name__ == "__main__":
    if "--write" in sys.argv:
        os.makedirs(os.path.dirname(NOISE_PATH), exist_ok=True)
        with open(NOISE_PATH, "w") as f:
            json.dump(measure(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", NOISE_PATH)
