"""Loop closing on the batched tracker's handle, device-resident.  LoopDetect: LoopClosing::DetectLoop (ORB/src/LoopClosing.cc:108-234) for a
batch of new keyframes -- loop_candidates (minScore and KeyFrameDatabase::DetectLoopCandidates) and loop_consistency (the covisibility
consistency groups), ivf_tracker_loop_candidates / ivf_tracker_loop_consistency in include/ivfront.h.  LoopSearch adds the two searches of
LoopClosing::ComputeSim3 (LoopClosing.cc:236-405) around BatchTracker.solve_sim3: SearchByBoW(KF, KF) in front of the solver and SearchBySim3
behind it (ivf_tracker_search_by_bow_keyframes, ivf_tracker_search_by_sim3).  The chain bow_vectors -> loop_candidates -> loop_consistency ->
search_by_bow_keyframes -> solve_sim3 -> search_by_sim3 runs without the host reading anything: pairs / select go from loop_consistency to the
searches, match12 from the first search to the other two calls, (ninliers > 0).to(torch.int32) is the select of the last.  Every tensor goes
through track._ptr, the one check of the tracker's Python layer, before its address is taken."""
from functools import partial

from ._lib import check
from .track import BYTES, F32, F64, I32, KF_NEIGH, KF_NEIGH_IS, LOCAL_POINT_BYTES, U8, _ptr, _require, _tensor


class LoopDetect:
    """LoopClosing::DetectLoop on a BatchTracker's handle, whose device and sizes it borrows; its calls obey the handle's
    one-call-at-a-time rule like the tracker's own.  The keyframe database is reloc_candidates' (flat tensors, keyframe index = insertion
    order); the current keyframes are rows of it.  Not a second entry point: the package exports LoopSearch alone, which inherits these two
    methods.  They sit in a base class because LoopSearch's own namespace is pinned by tests/test_loop_args_cpu.py to the two searches of
    ComputeSim3 and that table; tests/test_loop_detect_args_cpu.py holds the table of these two."""

    def __init__(self, tracker):
        self._tracker, self._lib, self._h = tracker, tracker._lib, tracker._h         # the tracker owns the handle: keep it alive
        self.nfeatures, self.record_bytes, self.device = tracker.nfeatures, tracker.record_bytes, tracker.device

    def loop_candidates(self, kf_bow_word, kf_bow_value, kf_bow_n, kf_neigh, conn_start, conn, query_kf, query_visible, min_score, cand, ncand,
                        kf_live=None, query_select=None, scores=None, common=None, stream_ptr=None):
        """minScore (ORB/src/LoopClosing.cc:129-143) and KeyFrameDatabase::DetectLoopCandidates (ORB/src/KeyFrameDatabase.cc:76-197) for
        n_queries current keyframes.  kf_bow_word / kf_bow_value [n_keyframes, nfeatures], kf_bow_n [n_keyframes], kf_neigh: torch.int32
        [n_keyframes, 10] and kf_live: torch.uint8 [n_keyframes] or None as reloc_candidates() takes them; conn_start: torch.int32
        [n_keyframes + 1] and conn: torch.int32 [n_conn], the connected keyframes of every keyframe as a CSR of keyframe indices;
        query_kf: torch.int32 [n_queries] keyframe indices; query_visible: torch.int32 [n_queries], keyframe k is in the inverted file
        of query q iff k < query_visible[q], it is live and it is not the query; query_select: torch.int32 [n_queries] or None, 0 =
        mnId < mLastLoopKFid + 10 (ncand -2, nothing else written).  Outputs: min_score: torch.float32 [n_queries]; cand: torch.int32
        [n_queries, max_candidates] in the reference's order, -1 beyond the count; ncand: torch.int32 [n_queries], the true count;
        scores: torch.float32 / common: torch.int32 [n_queries, n_keyframes] or None.  Asynchronous on the given stream, no host read."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        n_kf, n_q, n_conn = _tensor("kf_bow_n", kf_bow_n).numel(), _tensor("query_kf", query_kf).numel(), _tensor("conn", conn).numel()
        max_cand = int(_tensor("cand", cand, 2, "[n_queries, max_candidates]").shape[1])
        _require(cand.shape[0] == n_q and max_cand >= 1, "cand is [n_queries, max_candidates]", cand)
        check(self._lib.ivf_tracker_loop_candidates(
            self._h, p("kf_bow_word", kf_bow_word, I32, n_kf * nf), p("kf_bow_value", kf_bow_value, F64, n_kf * nf), p("kf_bow_n", kf_bow_n, I32, n_kf),
            p("kf_live", kf_live, U8, n_kf, optional=True), p("kf_neigh", kf_neigh, I32, n_kf * KF_NEIGH, exact=True, what=KF_NEIGH_IS), n_kf,
            p("conn_start", conn_start, I32, n_kf + 1, exact=True, what="conn_start is [n_keyframes + 1]"), p("conn", conn, I32, n_conn), n_conn,
            p("query_kf", query_kf, I32, n_q), p("query_visible", query_visible, I32, n_q), p("query_select", query_select, I32, n_q, optional=True),
            n_q, max_cand, p("min_score", min_score, F32, n_q), p("cand", cand, I32, n_q * max_cand, exact=True), p("ncand", ncand, I32, n_q),
            p("scores", scores, F32, n_q * n_kf, optional=True), p("common", common, I32, n_q * n_kf, optional=True), stream_ptr))

    def loop_consistency(self, kf_record, conn_start, conn, query_kf, cand, ncand, group_member, group_size, group_count, n_groups, enough, nenough,
                         pairs, select, status, th=3, stream_ptr=None):
        """The covisibility-consistency groups of LoopClosing::DetectLoop (ORB/src/LoopClosing.cc:148-230) for the queries of the call in
        order, from cand / ncand of loop_candidates().  kf_record: torch.int32 [n_keyframes], the keyframe's gather record or -1;
        conn_start / conn / query_kf as above.  The state mvConsistentGroups, read and written: group_member: torch.int32
        [group_cap, member_cap] keyframe indices ascending, -1 padded; group_size, group_count: torch.int32 [group_cap]; n_groups:
        torch.int32 [1].  Outputs: enough: torch.int32 [n_queries, max_candidates] = mvpEnoughConsistentCandidates, -1 padded; nenough:
        torch.int32 [n_queries]; pairs: torch.int32 [n_queries, max_candidates, 2] = (current keyframe's record, candidate's record) and
        select: torch.int32 [n_queries, max_candidates], what search_by_bow_keyframes() takes as [n_pairs, 2] / [n_pairs]; status:
        torch.int32 [n_queries], 1 from the first query whose groups or candidates exceed member_cap, group_cap or max_candidates (the
        state then stays as it was before that query).  th: mnCovisibilityConsistencyTh.  Asynchronous on the given stream."""
        p = partial(_ptr, self.device)
        n_kf, n_q, n_conn = _tensor("kf_record", kf_record).numel(), _tensor("query_kf", query_kf).numel(), _tensor("conn", conn).numel()
        max_cand = int(_tensor("cand", cand, 2, "[n_queries, max_candidates]").shape[1])
        _require(cand.shape[0] == n_q and max_cand >= 1, "cand is [n_queries, max_candidates]", cand)
        group_cap, member_cap = (int(v) for v in _tensor("group_member", group_member, 2, "[group_cap, member_cap]").shape)
        _require(group_cap >= 1 and member_cap >= 1, "group_member is [group_cap, member_cap]", group_member)
        _require(tuple(_tensor("pairs", pairs, 3, "[n_queries, max_candidates, 2]").shape) == (n_q, max_cand, 2), "pairs is [n_queries, max_candidates, 2]", pairs)
        check(self._lib.ivf_tracker_loop_consistency(
            self._h, p("kf_record", kf_record, I32, n_kf), n_kf, p("conn_start", conn_start, I32, n_kf + 1, exact=True, what="conn_start is [n_keyframes + 1]"),
            p("conn", conn, I32, n_conn), n_conn, p("query_kf", query_kf, I32, n_q), n_q, p("cand", cand, I32, n_q * max_cand, exact=True),
            p("ncand", ncand, I32, n_q), max_cand, int(th), p("group_member", group_member, I32, group_cap * member_cap, exact=True),
            p("group_size", group_size, I32, group_cap), p("group_count", group_count, I32, group_cap), p("n_groups", n_groups, I32, 1), group_cap, member_cap,
            p("enough", enough, I32, n_q * max_cand), p("nenough", nenough, I32, n_q), p("pairs", pairs, I32, n_q * max_cand * 2, exact=True),
            p("select", select, I32, n_q * max_cand), p("status", status, I32, n_q), stream_ptr))


class LoopSearch(LoopDetect):
    """DetectLoop's two calls (LoopDetect) and the two searches of ComputeSim3 on one borrowed handle"""

    def search_by_bow_keyframes(self, vocabulary, records, pairs, match12, nmatches, levelsup=4, select=None, point_flags=None, nn_ratio=0.75,
                                check_orientation=True, stream_ptr=None):
        """ORBmatcher(nn_ratio, check_orientation).SearchByBoW(pKF1, pKF2, vpMatches12) (ORB/src/ORBmatcher.cc:528-661; LoopClosing.cc:270
        passes 0.75, true) for n_pairs (KF1, KF2) record pairs, the feature vectors of both records computed in the call.  vocabulary: an
        ORBVocabulary on the tracker's device; records: torch.uint8 [n_records * record_bytes]; pairs: torch.int32 [n_pairs, 2]; select:
        torch.int32 [n_pairs] or None, 0 leaves a pair out (nmatches -2, match12 untouched); point_flags: torch.uint8
        [n_records, nfeatures], bit 0 = the keypoint holds a live map point (both sides), or None = every keypoint with a stereo depth;
        match12: torch.int32 [n_pairs, nfeatures] by KF1 keypoint = the KF2 keypoint whose point it is matched to or -1, what
        solve_sim3() and search_by_sim3() take; nmatches: torch.int32 [n_pairs] (-1: a record index outside the block).  Asynchronous
        on the given stream."""
        p, nf, tr = partial(_ptr, self.device), self.nfeatures, self._tracker
        (records_p, n_rec), (pairs_p, n_pairs) = tr._records(records), tr._pairs(pairs)
        check(self._lib.ivf_tracker_search_by_bow_keyframes(
            self._h, vocabulary._h, int(levelsup), records_p, self.record_bytes, n_rec, pairs_p, n_pairs,
            p("select", select, I32, n_pairs, optional=True), p("point_flags", point_flags, U8, n_rec * nf, optional=True),
            float(nn_ratio), int(bool(check_orientation)), p("match12", match12, I32, n_pairs * nf), p("nmatches", nmatches, I32, n_pairs), stream_ptr))

    def search_by_sim3(self, records, pairs, poses, kf_points, sim3, match12, matches, nfound, th=7.5, select=None, inlier=None, match1=None,
                       match2=None, stream_ptr=None):
        """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORB/src/ORBmatcher.cc:1145-1369) with both projection
        loops, behind the inlier filter of LoopClosing.cc:318-323, for n_pairs (KF1, KF2) record pairs.  poses: torch.float32
        [n_records, 12] (Tcw) and sim3: torch.float32 [n_pairs, 16] as solve_sim3() takes and writes them; kf_points: torch.uint8 view of
        LOCAL_POINT_DTYPE records [n_records, nfeatures] as search_reloc() takes it (flags bit 0 = none / bad); match12: torch.int32
        [n_pairs, nfeatures]; inlier: torch.uint8 [n_pairs, nfeatures] (solve_sim3()'s) or None = every match is kept; select:
        torch.int32 [n_pairs] or None, 0 leaves a pair out (nfound -2, nothing else written): (ninliers > 0).to(torch.int32) of
        solve_sim3(), whose sim3 is unwritten for a failed pair; th: 7.5 at LoopClosing.cc:328.  matches: torch.int32
        [n_pairs, nfeatures] = vpMatches12 on return as KF2 keypoint indices by KF1 keypoint, the kept input entries plus the agreed new
        ones, another tensor than match12; nfound: torch.int32 [n_pairs]; match1 / match2: torch.int32 [n_pairs, nfeatures] or None
        (vnMatch1 / vnMatch2).  The projections use the tracker's intrinsics in both directions.  Asynchronous on the given stream."""
        p, nf, tr = partial(_ptr, self.device), self.nfeatures, self._tracker
        (records_p, n_rec), (pairs_p, n_pairs) = tr._records(records), tr._pairs(pairs)
        check(self._lib.ivf_tracker_search_by_sim3(
            self._h, records_p, self.record_bytes, n_rec, pairs_p, n_pairs, p("select", select, I32, n_pairs, optional=True),
            p("poses", poses, F32, n_rec * 12, exact=True, what="poses are per RECORD: [n_records, 12]"),
            p("kf_points", kf_points, BYTES, n_rec * nf * LOCAL_POINT_BYTES), p("sim3", sim3, F32, n_pairs * 16, exact=True, what="sim3 is [n_pairs, 16]"),
            p("match12", match12, I32, n_pairs * nf), p("inlier", inlier, U8, n_pairs * nf, optional=True), float(th),
            p("matches", matches, I32, n_pairs * nf), p("nfound", nfound, I32, n_pairs), p("match1", match1, I32, n_pairs * nf, optional=True),
            p("match2", match2, I32, n_pairs * nf, optional=True), stream_ptr))
