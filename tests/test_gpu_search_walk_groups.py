"""The group boundaries of the prefetched list walk that SearchLocalPoints and Relocalization share (walk_lists_prefetched,
iv_slam_amd/csrc/ivf_search.h): the greedy kernels load the candidate lists of 16 queries per group and alternate two register sets, so an
error shows at a query count just below, at or just above a multiple of 16 and of 32.  n in {1, 15, 16, 17, 31, 32, 33, 48, 49} queries per
frame (local map points for ivf_tracker_search_local, keyframe keypoints for ivf_tracker_search_reloc), two frames / pairs per call.

A case is hand-made on the camera of tests/projection_scenes.py, every window of radius 12 (local: th 3 x RadiusByViewingCos 4; reloc:
th 12 at level 0):
  * most queries stand on one of 14 clusters of four keypoints, several queries per cluster, each with a best candidate of its own once
    the earlier ones are taken -- a dependence that crosses the group boundaries;
  * query n - 2 and every fifth query see no keypoint at all (an empty list inside a group);
  * with 128 features the LAST query stands on a crowd of 70 near-identical keypoints: its window overflows the 64 listed candidates and
    its best candidate sits behind them, so the last group re-walks a window.  A record of 64 features cannot hold such a crowd: the
    64-feature cases have every other property, their last query stands on a cluster.
The second frame / pair of a call is a variant: other queries empty, some keypoints held on entry, the crowd's best at the very last place.

Bar: the device's assignment and nmatches IDENTICAL to the oracle's, through the comparison helpers of tests/test_gpu_track_local.py
(check_local) and of tests/test_gpu_track_reloc.py's random sweep.  Before the device is involved, the restatements (projection_ref.py,
reloc_scenes.py:walk), held to the oracle's output, say that a case is not vacuous: a match made by a query of the last group; an empty
window in a group that also holds a match (n = 1 excepted: one query cannot be both); with 128 features an overflowing window in the last
group."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import projection_ref as R
import projection_scenes as PS
import reloc_scenes as RS
from projection_scenes import F, at_distance, spot, world
from test_gpu_track import iv  # noqa: F401  (the module fixture)

NS = (1, 15, 16, 17, 31, 32, 33, 48, 49)
NFS = (64, 128)
GROUP = 16                                          # kPrefetch
CROWD, CLUSTERS, RADIUS = 70, 14, 12.0
LOCAL_TH, RELOC_TH, ORB_DIST, NN_RATIO = 3.0, 12.0, 100, 0.8
CROWD_AT, EMPTY_AT = spot(20), spot(30)             # away from the clusters on spots 0 .. 13


def layout(n, nf, variant, min_level, max_level):
    """-> queries [(u, v, descriptor, cluster or None)], keypoints [[x, y, descriptor, held on entry]]"""
    rng = np.random.default_rng(1000 * n + 2 * nf + variant)
    desc = lambda: rng.integers(0, 256, 32).astype(np.uint8)                          # noqa: E731  (random descriptors lie ~128 bits apart)
    keys, cluster_desc = [], []
    for c in range(CLUSTERS):
        u, v = spot(c); d = desc(); cluster_desc.append(d)
        for k, (dx, dy) in enumerate(((-3, -3), (3, -3), (-3, 3), (3, 3))):
            keys.append([u + dx, v + dy, at_distance(d, (2, 30, 45, 60)[k], 40 * k), variant == 1 and k == 0 and c % 3 == 0])
    queries, c = [], 0
    for i in range(n):
        if i == n - 1 and nf >= 128:
            queries.append((CROWD_AT[0], CROWD_AT[1], desc(), None))
        elif i != n - 1 and (i == n - 2 or i % 5 == (2, 0)[variant]):
            queries.append((EMPTY_AT[0], EMPTY_AT[1], desc(), None))
        else:
            u, v = spot(c % CLUSTERS); queries.append((u, v, cluster_desc[c % CLUSTERS], c % CLUSTERS)); c += 1
    if nf >= 128:
        u, v, d, _ = queries[-1]
        first = len(keys)
        for i, (x, y) in enumerate(PS._lattice(CROWD, 9, 2.5, u - 10, v - 8.75)):
            keys.append([x, y, at_distance(d, 40 + i % 3, 3 * i), False])
        kps = np.zeros(len(keys), PS.KP_DTYPE); kps["x"] = [k[0] for k in keys]; kps["y"] = [k[1] for k in keys]
        order = R.features_in_area(R.build_grid(kps, PS.CAM["bounds"]), kps, PS.CAM["bounds"], u, v, F(RADIUS), min_level, max_level)
        assert len(order) == CROWD and min(order) == first
        keys[order[(66, 69)[variant]]][2] = at_distance(d, 10, 100)                   # the best: behind the 64 listed candidates
        if variant == 1:
            keys[order[2]][2] = at_distance(d, 4, 50); keys[order[2]][3] = True       # a better one among the listed, held on entry
    assert len(keys) <= nf
    return queries, keys


def last_group(n):
    return range(GROUP * ((n - 1) // GROUP), n)


def assert_not_vacuous(what, n, nf, matched, empty, n_window):
    """matched / empty: per query; n_window: per query or None"""
    assert any(matched[i] for i in last_group(n)), "%s: no match in the last group" % what
    if n > 1:
        assert any(empty[i] and any(matched[g] for g in range(i - i % GROUP, min(n, i - i % GROUP + GROUP))) for i in range(n)), \
            "%s: no empty window beside a match" % what
    if nf >= 128:
        assert any((n_window[i] or 0) > 64 for i in last_group(n)), "%s: no overflowing window in the last group" % what


# ---- SearchLocalPoints --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def local_case(n, nf):
    import projection_oracle as PO
    cam = dict(PS.CAM, nf=nf)
    scs = []
    for variant in (0, 1):
        queries, keys = layout(n, nf, variant, -1, 0)
        s = PS.Local("walk_groups_%d_%d_%d" % (n, nf, variant), th=LOCAL_TH, nn_ratio=NN_RATIO)
        for x, y, d, held in keys:
            s.kp(x, y, 0, d, occupied=held)
        for i, (u, v, d, c) in enumerate(queries):
            s.pt(world(u, v), d, nObs=0 if (c is not None and i % 7 == 3) else 1)
        s.done()
        nm, assign, outcome, infos = PS.ref_local(s)
        onm, oassign = PS.oracle_local(O, PO, s)
        assert nm == onm and np.array_equal(assign, oassign), s.name
        assert_not_vacuous(s.name, n, nf, [o in (R.ACCEPTED, R.ACCEPTED_THEN_REPLACED) for o in outcome], [o == R.EMPTY_WINDOW for o in outcome],
                           [i.get("n_window") for i in infos])
        scs.append(s)
    return cam, scs


@pytest.mark.gpu
@pytest.mark.parametrize("nf", NFS)
@pytest.mark.parametrize("n", NS)
def test_search_local_at_the_group_boundaries(iv, n, nf):
    from test_gpu_track_local import check_local, run_local
    cam, scs = local_case(n, nf)
    recs, per_frame, occ = [s.rec for s in scs], [s.points for s in scs], [s.occupied for s in scs]
    a, nm = run_local(iv, cam, recs, [0, 1], per_frame, None, occ, LOCAL_TH, NN_RATIO)
    check_local(cam, recs, [0, 1], per_frame, None, occ, LOCAL_TH, NN_RATIO, a, nm, what="n %d, nfeatures %d" % (n, nf))


# ---- Relocalization -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reloc_case(n, nf):
    """-> the two scenes with the oracle's (nmatches, assignment) of each"""
    import projection_oracle as PO
    scs = []
    for variant in (0, 1):
        queries, keys = layout(n, nf, variant, -1, 1)
        s = RS.Scene("walk_groups_%d_%d_%d" % (n, nf, variant), calls=((RELOC_TH, ORB_DIST, "given"),), nf=nf)
        for u, v, d, _ in queries:
            s.pt(world(u, v), d, lv=0)
        for x, y, d, held in keys:
            s.kp(x, y, 0, d, holds=0 if held else -1)                                 # held on entry: by whichever point, it is occupied
        s.done()
        s.ref = RS.oracle_search(O, PO, s, s.assign0, s.T, s.found, RELOC_TH, ORB_DIST)
        w = RS.walk(O, PO, s, s.assign0, 0)
        assert w[0] == s.ref[0] and np.array_equal(w[1], s.ref[1]), s.name
        assert_not_vacuous(s.name, n, nf, [g == RS.MATCHED for g in w[2]], [g == RS.EMPTY_WINDOW for g in w[2]], [i.get("n_window") for i in w[3]])
        scs.append(s)
    return scs


@pytest.mark.gpu
@pytest.mark.parametrize("nf", NFS)
@pytest.mark.parametrize("n", NS)
def test_search_reloc_at_the_group_boundaries(iv, n, nf):
    from test_gpu_track_reloc import FILL, run_scenes
    scs = reloc_case(n, nf)
    got = run_scenes(iv, scs)
    for k, sc in enumerate(scs):
        nC = len(sc.rec_cur["kps"])
        nm, ref = sc.ref
        a = got[0][0][k]
        bad = np.nonzero(a[:nC] != ref)[0]
        assert bad.size == 0, "n %d pair %d: %d keypoints differ, first %d: device %d, oracle %d" % (n, k, bad.size, bad[0], a[bad[0]], ref[bad[0]])
        assert int(got[0][1][k]) == nm and (a[nC:] == FILL).all()


# ---- the cases themselves, without a device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", NFS)
def test_cases_are_not_vacuous(nf):
    """restatement == oracle and the three conditions of the module's docstring, for every n (asserted while the cases are built)"""
    for n in NS:
        local_case(n, nf); reloc_case(n, nf)
