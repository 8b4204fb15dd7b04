"""The restatement of CreateNewMapPoints (tests/create_points_ref.py) on the hand-made scenes (tests/create_points_scenes.py), without a
GPU: every expectation of every scene is met, every stage code is reached, every injected fault changes the result of a named scene, the
Jacobi's triangulated point agrees with numpy's f64 SVD within a derived bound, and the C-ABI entry exists."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import create_points_ref as R          # noqa: E402
import create_points_scenes as SC      # noqa: E402

F = np.float32
SCENES = SC.all_scenes()
RESULTS = {sc["name"]: SC.run_ref(sc) for sc in SCENES}
# the scene that catches each injected fault
CAUGHT_BY = dict(has1_not_updated="ranks_identity", has1_updated_on_failure="ranks_identity", first_minimum="ranks_identity",
                 stereo2_cos_always="stereo_forward", chi2_float="exact_chi2_1", chi2_mono_78="stereo_forward", z_lt="stereo_forward",
                 ratio_fabs="exact_ratio_1", min_distance_octave="stereo_forward", desc_ignores_order="ranks_reversed", quality_max="ranks_identity",
                 order_by_idx1="ranks_identity")


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scene_expectations(sc):
    out = RESULTS[sc["name"]]
    for (rank, idx1), code in sc["expect"].items():
        got = int(out["stage"][rank, idx1])
        if code is None:
            assert got > R.BASELINE and out["matches"][rank, idx1] >= 0, (sc["name"], rank, idx1, R.NAMES[got])
        else:
            assert got == code, "%s rank %d idx1 %d: %s, expected %s" % (sc["name"], rank, idx1, R.NAMES[got], R.NAMES[code])
        if code is not None and code >= R.BY_SVD:
            assert out["new_neigh"][idx1] == rank and out["new_idx2"][idx1] == out["matches"][rank, idx1] and out["new_point"]["flags"][idx1] == 2
    made = out["new_order"] >= 0
    assert sorted(out["new_order"][made].tolist()) == list(range(int(max(out["n_new"], 0))))
    assert ((out["stage"] >= R.BY_SVD).sum(axis=0) <= 1).all(), "an idx1 creates at most one point per call"


def test_every_stage_code_is_reached():
    seen = {}
    for sc in SCENES:
        for code in np.unique(RESULTS[sc["name"]]["stage"]):
            seen.setdefault(int(code), sc["name"])
    assert sorted(seen) == list(range(16)), "not reached: %s" % [R.NAMES[c] for c in range(16) if c not in seen]


def test_what_the_scenes_are_about():
    by = {sc["name"]: sc for sc in SCENES}
    o = RESULTS["ranks_identity"]; sc = by["ranks_identity"]
    a, b, c, e, g = 0, 1, 2, 3, 4                                               # the order ranks_scene adds them in
    assert o["matches"][0, a] >= 0 and o["new_neigh"][a] == 2 and o["new_neigh"][b] == 0 and o["matches"][2, b] == -1
    assert o["new_idx2"][c] == o["new_idx2"][e] >= 0, "two idx1 on one idx2"
    assert o["new_order"][a] == o["n_new"] - 1 and o["new_order"][b] == 0, "creation order: neighbour rank first"
    assert o["new_idx2"][g] == o["matches"][0, g] and by["ranks_identity"]["records"][1]["kps"]["x"][o["new_idx2"][g]] == F(336.0), "the later equal minimum"
    assert (o["matches"][1] == -1).all() and (o["matches"][3] == -1).all() and (o["stage"][[1, 3]] == 0).all(), "a -1 and an out-of-range neighbour are skipped"
    # kf_order decides the descriptor
    r1, r2 = RESULTS["ranks_identity"], RESULTS["ranks_reversed"]
    i2 = r1["new_idx2"][b]
    assert r1["new_point"]["desc"][b].tobytes() == sc["records"][0]["desc"][b].tobytes()
    assert r2["new_point"]["desc"][b].tobytes() == sc["records"][1]["desc"][i2].tobytes()
    q = sc["key_quality"]
    assert r1["new_quality"][b] == min(q[0][b], q[1][i2])
    assert RESULTS["bad_keyframe"]["n_new"] == -1 and RESULTS["nothing_eligible"]["n_new"] == 0 and RESULTS["empty_keyframe"]["n_new"] == 0
    assert RESULTS["svd_chi2"]["n_new"] == 1 and RESULTS["baseline"]["n_new"] >= 0
    # computed F12 and given F12, with and without key qualities
    assert by["svd_real"]["F12"] is None and by["stereo_forward"]["F12"] is not None
    assert by["exact_ratio_0"]["key_quality"] is None and (RESULTS["exact_ratio_0"]["new_quality"][0] == 1.0)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_fault_is_caught(fault):
    name = CAUGHT_BY[fault]
    sc = [s for s in SCENES if s["name"] == name][0]
    k = R.same(RESULTS[name], SC.run_ref(sc, fault=fault))
    assert k is not None, "fault %s leaves scene %s unchanged" % (fault, name)


# ---- the Jacobi against numpy's f64 SVD ----------------------------------------------------------------------------------------------
# x = v[0:3] / v[3] of the smallest right singular vector.  Both solvers are backward stable in f64: each returns the exact vector of a
# matrix A + E with |E| <= c 2^-52 sigma1, c a small constant of the method (Demmel & Veselic for one-sided Jacobi; LAPACK's gesdd); by
# Wedin's theorem the vector then moves by at most |E| / gap, gap = sigma3 - sigma4 >= sigma3 / 2 for the matrices kept below (sigma4 <=
# sigma3 / 2 is asserted).  With c = 64 for the two solvers together the two unit vectors differ by at most 2 c 2^-52 sigma1 / sigma3;
# the unit vector is (x, 1) / sqrt(1 + |x|^2), so 1 / |w| = sqrt(1 + |x|^2) and the quotient x = v / w turns a perturbation d of the unit vector
# into at most sqrt(1 + |x|^2) (1 + |x|) d to first order; narrowing v and w to float and the float division add three roundings of
# 2^-24 relative to each component.  DESIGN.md section 3 holds c and the measured maximum (0.60 of the bound over 313 matrices).
C_SVD = 64.0
COND_CAP = 1.0e4


def svd_bound(A, x):
    s = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    assert s[3] <= 0.5 * s[2]
    d = 2.0 * C_SVD * 2.0 ** -52 * s[0] / s[2]                                  # between the two unit vectors
    nx = float(np.linalg.norm(x))
    hom = np.sqrt(1.0 + nx * nx)                                                # 1 / |w| of the unit vector (x, 1) / hom
    return hom * (1.0 + nx) * d + 3.0 * 2.0 ** -24 * max(nx, 1e-30), s[0] / s[2]


def numpy_point(A):
    _, _, vt = np.linalg.svd(A.astype(np.float64))
    v = vt[3]
    return v[:3] / v[3]


def random_two_view(rng):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0, 0.3)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    T1 = SC.pose((0, 0, 0)); T2 = SC.pose(rng.uniform(-1, 1, 3) * (1, 1, 0.3) + (1.0, 0, 0), Rm.astype(F))
    X = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 30)])
    kps = []
    for T in (T1, T2):
        u, v, z = SC.project(T, X)
        kps.append(dict(x=F(u + rng.normal(0, 0.3)), y=F(v + rng.normal(0, 0.3)), octave=0))
    return T1, T2, kps


def test_jacobi_point_agrees_with_numpy_svd():
    rng = np.random.default_rng(2024)
    cases = []
    for sc in SCENES:
        for info in RESULTS[sc["name"]]["infos"].values():
            if "A" in info and info["v"][3] != 0:
                sv = np.linalg.svd(info["A"].astype(np.float64), compute_uv=False)
                if sv[0] / sv[2] < COND_CAP and sv[3] <= 0.5 * sv[2]:
                    cases.append(info["A"])
    n_scene = len(cases)
    assert n_scene >= 8
    while len(cases) < n_scene + 300:
        T1, T2, kps = random_two_view(rng)
        _, info = R.triangulate(SC.CAM, T1, T2, np.zeros(3, F), -(T2[:3, :3].T @ T2[:3, 3]), kps[0], F(-1), F(-1), kps[1], F(-1), F(-1))
        if "A" not in info or info["v"][3] == 0:
            continue
        s = np.linalg.svd(info["A"].astype(np.float64), compute_uv=False)
        if s[0] / s[2] < COND_CAP and s[3] <= 0.5 * s[2]:
            cases.append(info["A"])
    worst = 0.0
    for A in cases:
        v, _, _ = R.jacobi_smallest4(A)
        x = np.array([F(v[0] / v[3]), F(v[1] / v[3]), F(v[2] / v[3])], np.float64)
        ref = numpy_point(A)
        bound, cond = svd_bound(A, ref)
        assert cond < COND_CAP
        err = float(np.abs(x - ref).max())
        worst = max(worst, err / bound)
        assert err <= bound, (err, bound, cond)
    print("jacobi vs numpy: %d cases, worst error / bound = %.3g" % (len(cases), worst))


def test_abi_entry_exists_and_refuses_a_null_handle():
    from iv_slam_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "ivf_tracker_create_map_points")
    rc = lib.ivf_tracker_create_map_points(None, None, 0, None, 0, 0, None, 0, None, 1, None, None, None, None, None, None, None, None, None, None, None,
                                           None, None, None)
    assert rc == _lib.IVF_E_INVALID
