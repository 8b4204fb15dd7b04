"""local_map_scenes.py -- hand-made maps for ivf_tracker_update_local_map, one per gate of Tracking::UpdateLocalKeyFrames /
UpdateLocalPoints (test infrastructure only), shared by tests/test_local_map_cpu.py (the restatement's stage codes, the injected
faults) and tests/test_gpu_local_map.py (the device against the restatement).

The base map: keyframe k holds the points 3k, 3k + 1, 3k + 2 and point m is observed by keyframe m // 3, so holding point 3k is one
vote for keyframe k.  Every scene says what the reference must do in `expect`: the local list, pKFmax (None = untouched), the early
return, stage codes of the keyframes it is about, the stop of the walk, and the point list where the scene is about points."""
import numpy as np

import local_map_ref as R

NF = 256
PREV_REF = -7                                   # d_ref_kf as it comes in: a mark the call must leave where there is no pKFmax


def base(n_kf=12, **kw):
    obs = {m: [m // 3] for m in range(3 * n_kf)}
    kfp = {k: [3 * k, 3 * k + 1, 3 * k + 2] for k in range(n_kf)}
    obs.update(kw.pop("obs", {})); kfp.update(kw.pop("kf_points", {}))
    return R.make_map(3 * n_kf, n_kf, obs=obs, kf_points=kfp, **kw)


def scene(name, M, held, prev=(), prev_n=None, max_lk=96, max_pts=64, **expect):
    fp = np.full(NF, -1, np.int32); fp[:len(held)] = held
    row = np.full(max_lk, -3, np.int32); row[:len(prev)] = prev
    return dict(name=name, map=M, frame_points=fp, prev_row=row, prev_n=len(prev) if prev_n is None else prev_n, prev_ref=PREV_REF,
                max_pts=max_pts, expect=expect)


def votes_for(*kfs):
    """held points that give one vote to each listed keyframe (repeat a keyframe for more: its points 3k, 3k + 1, 3k + 2)"""
    seen, out = {}, []
    for k in kfs:
        out.append(3 * k + seen.get(k, 0)); seen[k] = seen.get(k, 0) + 1
    return out


def all_scenes():
    S = []
    # ---- votes and liveness
    S.append(scene("no_held_no_prev", base(), [], early=True, list=[], ref=None, ids=[]))
    S.append(scene("no_held_prev_list", base(), [], prev=[2, 0], early=True, list=[2, 0], ref=None, ids=[6, 7, 8, 0, 1, 2]))
    S.append(scene("bad_held_nulled_no_vote", base(bad_points=[0]), [0], prev=[1], early=True, list=[1], ref=None, ids=[3, 4, 5], nulled=[0]))
    S.append(scene("bad_keyframe_most_votes", base(bad_keyframes=[0]), votes_for(0, 0, 0, 1, 1, 2), early=False, list=[1, 2], ref=1,
                   stages={0: [R.VOTED_BAD], 1: [R.VOTED], 2: [R.VOTED]}))
    S.append(scene("all_voted_bad", base(bad_keyframes=[0]), votes_for(0), prev=[4], early=False, list=[], ref=None, ids=[]))
    S.append(scene("tie_identity_order", base(), votes_for(0, 0, 1, 1), early=False, list=[0, 1], ref=0))
    S.append(scene("tie_permuted_order", base(order=[1, 0] + list(range(2, 12))), votes_for(0, 0, 1, 1), early=False, list=[1, 0], ref=1))
    S.append(scene("later_keyframe_strictly_larger", base(), votes_for(0, 1, 1, 2), early=False, list=[0, 1, 2], ref=1))
    # ---- neighbours
    S.append(scene("neighbour_bad_or_included_before_first_eligible", base(neigh={0: [3, 0, -1, 4, 5]}, bad_keyframes=[3]), votes_for(0),
                   early=False, list=[0, 4], ref=0, stages={4: [(R.NEIGHBOUR_OF, 0)]}, absent=[3, 5]))
    S.append(scene("neighbour_padding_only", base(neigh={0: [-1] * 10}), votes_for(0), early=False, list=[0], ref=0))
    # ---- children
    S.append(scene("first_eligible_child_in_given_order", base(children={0: [2, 5, 4]}, bad_keyframes=[2]), votes_for(0), early=False,
                   list=[0, 5], ref=0, stages={5: [(R.CHILD_OF, 0)]}, absent=[2, 4]))
    # ---- parents
    S.append(scene("bad_parent_still_appended", base(parent={0: 5}, bad_keyframes=[5]), votes_for(0), early=False, list=[0, 5], ref=0,
                   stages={5: [(R.PARENT_OF, 0)]}, stops=[R.STOPPED_BY_PARENT]))
    S.append(scene("parent_ends_expansion_for_later_keyframes", base(parent={0: 5}, neigh={1: [6]}), votes_for(0, 1), early=False,
                   list=[0, 1, 5], ref=0, stops=[R.STOPPED_BY_PARENT], absent=[6]))
    S.append(scene("parent_already_included_goes_on", base(parent={0: 1}, neigh={1: [6]}), votes_for(0, 1), early=False, list=[0, 1, 6],
                   ref=0, stops=[]))
    S.append(scene("neighbour_child_parent_of_one_keyframe", base(neigh={0: [3]}, children={0: [4]}, parent={0: 5}), votes_for(0),
                   early=False, list=[0, 3, 4, 5], ref=0))
    # ---- the 80 check: keyframe 0 has a neighbour and a child, keyframe 1 a neighbour
    for K, want, stops in ((81, list(range(81)), [R.STOPPED_BY_80]), (80, list(range(80)) + [100, 101], [R.STOPPED_BY_80]),
                           (79, list(range(79)) + [100, 101], [R.STOPPED_BY_80]), (78, list(range(78)) + [100, 101, 102], [R.STOPPED_BY_80])):
        M = base(n_kf=110, neigh={0: [100], 1: [102]}, children={0: [101]})
        S.append(scene("limit_80_K%d" % K, M, votes_for(*range(K)), early=False, list=want, ref=0, stops=stops, max_pts=300))
    S.append(scene("appended_keyframe_not_expanded", base(neigh={0: [3], 3: [4]}), votes_for(0), early=False, list=[0, 3], ref=0, absent=[4]))
    # ---- points
    kfp = {0: [-1, 7, 0], 1: [7, 3, 9], 2: [9, 7, 6, 1]}
    S.append(scene("points_first_place_skips_held_and_flags", base(kf_points=kfp, obs={1: [2]}, bad_points=[3], no_obs_points=[6, 9]),
                   [0, 1, 6], early=False, list=[0, 2], ref=2, ids=[7, 0, 9, 6, 1], held_listed=[0, 6, 1], bit1_clear=[9, 6],
                   points=[(0, 0, R.NO_POINT), (0, 1, R.KEPT), (0, 2, R.KEPT), (1, 0, R.KEPT), (1, 1, R.DUPLICATE), (1, 2, R.KEPT), (1, 3, R.KEPT)]))
    S.append(scene("point_in_three_keyframes", base(kf_points=kfp, bad_points=[3]), [0, 4, 6], early=False, list=[0, 1, 2], ref=0,
                   ids=[7, 0, 9, 6, 1], points=[(0, 0, R.NO_POINT), (0, 1, R.KEPT), (0, 2, R.KEPT), (1, 0, R.DUPLICATE), (1, 1, R.BAD_POINT),
                                                (1, 2, R.KEPT), (2, 0, R.DUPLICATE), (2, 1, R.DUPLICATE), (2, 2, R.KEPT), (2, 3, R.KEPT)]))
    # ---- caps: the list has four keyframes and the row two; their six points meet a cap of four
    S.append(scene("both_caps_hit", base(neigh={0: [3]}, children={0: [4]}), votes_for(0, 1), max_lk=2, max_pts=4, early=False, list=[0, 1, 3, 4],
                   ref=0, ids=[0, 1, 2, 3, 4, 5], points=[(0, 0, R.KEPT), (0, 1, R.KEPT), (0, 2, R.KEPT), (1, 0, R.KEPT), (1, 1, R.CUT_BY_CAP),
                                                          (1, 2, R.CUT_BY_CAP)]))
    S.append(scene("previous_count_clamped", base(), [], prev=[1, 2], prev_n=1000, max_lk=2, early=True, list=[1, 2], ref=None, ids=[3, 4, 5, 6, 7, 8]))
    # ---- hostile tables: out-of-range entries everywhere and decreasing offsets
    M = base(neigh={0: [99, -5, 3]}, children={0: [1 << 30, 4]}, parent={0: 12, 1: -9}, order=[0, 77, 1, 2, 3, 4, 5, 6, 7, 8, 9, -2])
    M.obs_kf[3] = 500                                                            # point 3's only observation names no keyframe
    M.kf_points[3 * 4 + 1] = 4000                                                # keyframe 4 holds a point outside the map
    M.kf_point_offsets[3], M.kf_point_offsets[4] = 12, 9                         # keyframe 3: a decreasing row
    M.obs_offsets[36] = 1 << 20                                                  # the last point's row ends past the table
    S.append(scene("hostile_tables", M, [0, 3, 35, 900, -4], early=False, list=[0, 3, 4], ref=0, ids=[0, 1, 2, 9, 10, 11, 12, 14]))      # keyframe 4's row now starts at 9
    Mp = base(); Mp.kf_point_offsets[:] = Mp.kf_point_offsets[::-1].copy()
    S.append(scene("hostile_previous_list", Mp, [], prev=[5, 400, -1, 0], early=True, list=[5, 400, -1, 0], ref=None, ids=[]))
    return S
