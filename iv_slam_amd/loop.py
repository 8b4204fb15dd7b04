"""The two searches of LoopClosing::ComputeSim3 (ORB/src/LoopClosing.cc:236-405) around BatchTracker.solve_sim3, batched and
device-resident on the same handle: SearchByBoW(KF, KF) in front of the solver and SearchBySim3 behind it (ivf_tracker_search_by_bow_keyframes,
ivf_tracker_search_by_sim3 in include/ivfront.h).  The chain search_by_bow_keyframes -> solve_sim3 -> search_by_sim3 runs without the host
reading anything: match12 goes from the first call to the other two, (ninliers > 0).to(torch.int32) is the select of the last.  Every tensor
goes through track._ptr, the one check of the tracker's Python layer, before its address is taken."""
from functools import partial

from ._lib import check
from .track import BYTES, F32, I32, LOCAL_POINT_BYTES, U8, _ptr


class LoopSearch:
    """borrows a BatchTracker's handle, device and sizes; its calls obey the handle's one-call-at-a-time rule like the tracker's own"""

    def __init__(self, tracker):
        self._tracker, self._lib, self._h = tracker, tracker._lib, tracker._h         # the tracker owns the handle: keep it alive
        self.nfeatures, self.record_bytes, self.device = tracker.nfeatures, tracker.record_bytes, tracker.device

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
