"""Batched, device-resident tracker step (ivf_tracker_* in include/ivfront.h): for every (last, cur) pair of gather records
the matcher part of Tracking::TrackWithMotionModel (ORB/src/Tracking.cc:1303-1330) -- UpdateLastFrame's stereo points,
ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, false) (ORB/src/ORBmatcher.cc:1372-1518), the retry with the wider
window -- in one launch sequence on the device.  torch tensors are only the device-memory plumbing."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Bounds, TrackConfig, check


def record_bytes(nfeatures):
    return int(_lib.load().ivf_track_record_bytes(int(nfeatures)))


class BatchTracker:
    """TrackWithMotionModel's matcher call for up to max_pairs frame pairs per launch sequence.

    th = 7 for stereo (Tracking.cc:1313-1317), th_retry = 2 * th and retry_below = 20 (Tracking.cc:1320-1330) are the
    reference's values; th_depth = mThDepth selects UpdateLastFrame's close-point rule (localization mode)."""

    def __init__(self, nfeatures, scale_factors, fx, fy, cx, cy, bf, bounds, max_pairs, th=7.0, th_retry=None, retry_below=20,
                 check_orientation=True, th_depth=0.0, points_block=True, b=None, device_id=0):
        self._lib = _lib.load()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        cfg = TrackConfig()
        cfg.nfeatures = nfeatures; cfg.nlevels = len(sf)
        for i, v in enumerate(sf):
            cfg.scale_factors[i] = float(v)
        cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.bf = fx, fy, cx, cy, bf
        cfg.b = b if b is not None else bf / fx                          # mb = mbf / fx (Frame.cc:410)
        cfg.bounds = Bounds(*bounds)
        cfg.th = th; cfg.th_retry = 2.0 * th if th_retry is None else th_retry
        cfg.retry_below = int(retry_below); cfg.check_orientation = int(bool(check_orientation))
        cfg.th_depth = th_depth; cfg.points_block = int(bool(points_block)); cfg.max_pairs = max_pairs; cfg.device_id = device_id
        h = C.c_void_p()
        check(self._lib.ivf_tracker_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.nfeatures, self.max_pairs, self.record_bytes = nfeatures, max_pairs, record_bytes(nfeatures)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.ivf_tracker_destroy(self._h)
            self._h = None

    def run(self, records, pairs, assign, nmatches, poses=None, point_flags=None, point_quality=None, key_quality=None, stream_ptr=None):
        """records: torch.uint8 [n_records * record_bytes] (a packed block or the all-gathered buffer); pairs: torch.int32
        [n_pairs, 2] = (last, cur) record indices; assign: torch.int32 [n_pairs, nfeatures]; nmatches: torch.int32 [n_pairs];
        poses: torch.float32 [n_pairs, 2, 12] = per pair {LastFrame.mTcw, CurrentFrame.mTcw prior}, row-major 3x4, or None = zero
        motion; point_flags: torch.uint8 [n_records, nfeatures] or None; point_quality / key_quality: torch.float32
        [n_pairs, nfeatures] in/out (UpdateQualityScores on the device) or None.  Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_pairs = pairs.shape[0]
        assert pairs.dtype.is_floating_point is False and pairs.element_size() == 4 and pairs.is_contiguous()
        assert assign.element_size() == 4 and assign.numel() >= n_pairs * self.nfeatures and nmatches.numel() >= n_pairs
        assert poses is None or (poses.is_contiguous() and poses.numel() == n_pairs * 24), "poses are per PAIR: [n_pairs, 2, 12]"
        for q in (point_quality, key_quality):
            assert q is None or (q.is_contiguous() and q.element_size() == 4 and q.numel() >= n_pairs * self.nfeatures)
        check(self._lib.ivf_tracker_run(self._h, records.data_ptr(), self.record_bytes, n_rec, pairs.data_ptr(), n_pairs,
                                        None if poses is None else poses.data_ptr(),
                                        None if point_flags is None else point_flags.data_ptr(),
                                        None if point_quality is None else point_quality.data_ptr(),
                                        None if key_quality is None else key_quality.data_ptr(),
                                        assign.data_ptr(), nmatches.data_ptr(), stream_ptr))

    def search_local(self, records, frames, points, point_offsets, max_points_per_frame, assign, nmatches, poses=None, occupied=None,
                     th=1.0, nn_ratio=0.8, cos_limit=0.5, point_quality=None, key_quality=None, stream_ptr=None):
        """Tracking::SearchLocalPoints (ORB/src/Tracking.cc:2088-2132) for n_frames frames at once: Frame::isInFrustum of every local
        map point, then ORBmatcher(nn_ratio).SearchByProjection(F, vpMapPoints, th).  frames: torch.int32 [n_frames] record indices;
        points: torch.uint8 view of LOCAL_POINT_DTYPE records (80 B each); point_offsets: torch.int32 [n_frames + 1] (CSR);
        poses: torch.float32 [n_frames, 12] (the pose of frame SLOT f) or None; occupied: torch.uint8 [n_frames, nfeatures] or None;
        assign: torch.int32 [n_frames, nfeatures] (index within the frame's point range or -1); nmatches: torch.int32 [n_frames];
        point_quality: torch.float32 indexed like points, key_quality: torch.float32 [n_frames, nfeatures] (both in/out) or None.
        Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_frames = frames.numel()
        assert frames.element_size() == 4 and point_offsets.element_size() == 4 and point_offsets.numel() >= n_frames + 1
        assert assign.element_size() == 4 and assign.numel() >= n_frames * self.nfeatures and nmatches.numel() >= n_frames
        assert poses is None or (poses.is_contiguous() and poses.numel() == n_frames * 12), "poses are per frame SLOT: [n_frames, 12]"
        check(self._lib.ivf_tracker_search_local(self._h, records.data_ptr(), self.record_bytes, n_rec, frames.data_ptr(), n_frames,
                                                 None if poses is None else poses.data_ptr(), points.data_ptr(), point_offsets.data_ptr(),
                                                 int(max_points_per_frame), None if occupied is None else occupied.data_ptr(),
                                                 float(th), float(nn_ratio), float(cos_limit),
                                                 None if point_quality is None else point_quality.data_ptr(),
                                                 None if key_quality is None else key_quality.data_ptr(),
                                                 assign.data_ptr(), nmatches.data_ptr(), stream_ptr))

    def points_from_pairs(self, records, pairs, assign, xw, has_point, poses=None, stream_ptr=None):
        """The map points behind run()'s assignments: xw[p, i2] = Frame::UnprojectStereo(assign[p, i2]) of the LAST record of pair p under
        its last pose (ORB/src/Frame.cc:958-972), has_point[p, i2] = 1 where there is one.  pairs / poses / assign as run() took and
        wrote them; xw: torch.float32 [n_pairs, nfeatures, 3], has_point: torch.uint8 [n_pairs, nfeatures].  Asynchronous."""
        n_rec = records.numel() // self.record_bytes
        n_pairs = pairs.shape[0]
        assert pairs.element_size() == 4 and pairs.is_contiguous() and assign.element_size() == 4 and assign.numel() >= n_pairs * self.nfeatures
        assert poses is None or (poses.is_contiguous() and poses.numel() == n_pairs * 24), "poses are per PAIR: [n_pairs, 2, 12]"
        assert xw.element_size() == 4 and xw.numel() >= n_pairs * self.nfeatures * 3 and has_point.element_size() == 1 and has_point.numel() >= n_pairs * self.nfeatures
        check(self._lib.ivf_tracker_points_from_pairs(self._h, records.data_ptr(), self.record_bytes, n_rec, pairs.data_ptr(), n_pairs,
                                                      None if poses is None else poses.data_ptr(), assign.data_ptr(), xw.data_ptr(),
                                                      has_point.data_ptr(), stream_ptr))

    def points_from_local(self, points, point_offsets, assign, xw, has_point, stream_ptr=None):
        """The map points behind search_local()'s assignments: xw[f, i] = points[point_offsets[f] + assign[f, i]].pos.  Asynchronous."""
        n_frames = point_offsets.numel() - 1
        assert point_offsets.element_size() == 4 and assign.element_size() == 4 and assign.numel() >= n_frames * self.nfeatures
        assert xw.element_size() == 4 and xw.numel() >= n_frames * self.nfeatures * 3 and has_point.element_size() == 1 and has_point.numel() >= n_frames * self.nfeatures
        check(self._lib.ivf_tracker_points_from_local(self._h, points.data_ptr(), point_offsets.data_ptr(), assign.data_ptr(), n_frames,
                                                      xw.data_ptr(), has_point.data_ptr(), stream_ptr))

    def search_by_bow(self, vocabulary, records, pairs, assign, nmatches, levelsup=4, select=None, point_flags=None, nn_ratio=0.7,
                      check_orientation=True, point_quality=None, key_quality=None, stream_ptr=None):
        """Tracking::TrackReferenceKeyFrame's matcher part (ORB/src/Tracking.cc:1159-1176) for n_pairs (keyframe, current) record pairs:
        Frame::ComputeBoW reduced to mFeatVec, ORBmatcher(nn_ratio, check_orientation).SearchByBoW (ORB/src/ORBmatcher.cc:165-294) and,
        with the quality arrays, UpdateQualityScores -- the fallback of the pairs run() could not track.  vocabulary: an ORBVocabulary on
        the tracker's device; pairs: torch.int32 [n_pairs, 2] = (keyframe record, current record); select: torch.int32 [n_pairs] or None,
        0 leaves a pair out (assign -1, nmatches -2), e.g. (run's nmatches < 20).to(torch.int32); point_flags: torch.uint8
        [n_records, nfeatures], bit 0 = the keypoint holds a live map point, or None = every keypoint with a stereo depth;
        point_quality (by keyframe keypoint) / key_quality (by frame keypoint): torch.float32 [n_pairs, nfeatures] in/out or None;
        assign: torch.int32 [n_pairs, nfeatures] = the keyframe keypoint whose point the frame keypoint receives or -1; nmatches:
        torch.int32 [n_pairs].  Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_pairs = pairs.shape[0]
        assert pairs.dtype.is_floating_point is False and pairs.element_size() == 4 and pairs.is_contiguous()
        assert assign.element_size() == 4 and assign.numel() >= n_pairs * self.nfeatures and nmatches.numel() >= n_pairs
        assert select is None or (select.element_size() == 4 and select.is_contiguous() and select.numel() >= n_pairs)
        assert point_flags is None or (point_flags.element_size() == 1 and point_flags.numel() >= n_rec * self.nfeatures)
        for q in (point_quality, key_quality):
            assert q is None or (q.is_contiguous() and q.element_size() == 4 and q.numel() >= n_pairs * self.nfeatures)
        check(self._lib.ivf_tracker_search_by_bow(self._h, vocabulary._h, int(levelsup), records.data_ptr(), self.record_bytes, n_rec,
                                                  pairs.data_ptr(), n_pairs, None if select is None else select.data_ptr(),
                                                  None if point_flags is None else point_flags.data_ptr(), float(nn_ratio),
                                                  int(bool(check_orientation)),
                                                  None if point_quality is None else point_quality.data_ptr(),
                                                  None if key_quality is None else key_quality.data_ptr(),
                                                  assign.data_ptr(), nmatches.data_ptr(), stream_ptr))

    def points_from_keyframe(self, pairs, kf_xw, assign, xw, has_point, stream_ptr=None):
        """The map points behind search_by_bow()'s assignments: xw[p, i] = kf_xw[keyframe record of pair p, assign[p, i]], has_point = 1
        where there is one.  kf_xw: torch.float32 [n_records, nfeatures, 3] = GetWorldPos() of the point each keypoint of each record
        holds; pairs / assign as search_by_bow() took and wrote them.  Asynchronous."""
        n_pairs = pairs.shape[0]
        n_rec = kf_xw.numel() // (self.nfeatures * 3)
        assert pairs.element_size() == 4 and pairs.is_contiguous() and assign.element_size() == 4 and assign.numel() >= n_pairs * self.nfeatures
        assert kf_xw.is_contiguous() and kf_xw.element_size() == 4 and kf_xw.numel() == n_rec * self.nfeatures * 3
        assert xw.element_size() == 4 and xw.numel() >= n_pairs * self.nfeatures * 3 and has_point.element_size() == 1 and has_point.numel() >= n_pairs * self.nfeatures
        check(self._lib.ivf_tracker_points_from_keyframe(self._h, pairs.data_ptr(), n_pairs, n_rec, kf_xw.data_ptr(), assign.data_ptr(),
                                                         xw.data_ptr(), has_point.data_ptr(), stream_ptr))

    def bow_vectors(self, vocabulary, records, frames, bow_word, bow_value, bow_n, stream_ptr=None):
        """Frame::ComputeBoW's mBowVec (ORB/src/Frame.cc:683-694; TemplatedVocabulary.h:1126-1204 with TF_IDF / L1_NORM) for n_frames
        records at once, the first line of Tracking::Relocalization (ORB/src/Tracking.cc:2274) and what a keyframe brings to the database
        when it is inserted.  frames: torch.int32 [n_frames] record indices (any number of them); bow_word: torch.int32
        [n_frames, nfeatures], the words ascending, -1 beyond the count; bow_value: torch.float64 [n_frames, nfeatures]; bow_n:
        torch.int32 [n_frames], -1 for a record index outside the block.  Bit for bit what ORBVocabulary.transform gives on the same
        descriptors.  Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_frames = frames.numel()
        nf = self.nfeatures
        assert frames.element_size() == 4 and frames.is_contiguous() and not frames.dtype.is_floating_point
        assert bow_word.element_size() == 4 and bow_word.is_contiguous() and bow_word.numel() >= n_frames * nf
        assert bow_value.element_size() == 8 and bow_value.dtype.is_floating_point and bow_value.is_contiguous() and bow_value.numel() >= n_frames * nf
        assert bow_n.element_size() == 4 and bow_n.is_contiguous() and bow_n.numel() >= n_frames
        check(self._lib.ivf_tracker_bow_vectors(self._h, vocabulary._h, records.data_ptr(), self.record_bytes, n_rec, frames.data_ptr(), n_frames,
                                                bow_word.data_ptr(), bow_value.data_ptr(), bow_n.data_ptr(), stream_ptr))

    def reloc_candidates(self, vocabulary, kf_bow_word, kf_bow_value, kf_bow_n, kf_neigh, kf_record, bow_word, bow_value, bow_n, frame_record,
                         cand, ncand, pairs, select, kf_live=None, kf_reloc_score=None, scores=None, common=None, stream_ptr=None):
        """KeyFrameDatabase::DetectRelocalizationCandidates (ORB/src/KeyFrameDatabase.cc:199-309, L1 score) for n_frames lost frames
        against a database of n_keyframes keyframes held as flat tensors, keyframe index = insertion order.  kf_bow_word / kf_bow_value
        [n_keyframes, nfeatures] and kf_bow_n [n_keyframes] as bow_vectors() wrote them; kf_neigh: torch.int32 [n_keyframes, 10] =
        GetBestCovisibilityKeyFrames(10) as keyframe indices, -1 padded; kf_record: torch.int32 [n_keyframes], the keyframe's gather record
        or -1; kf_live: torch.uint8 [n_keyframes] or None, 0 = erased; kf_reloc_score: torch.float32 [n_keyframes] or None (= 0), the
        mRelocScore every keyframe holds before this call (read-only); bow_word / bow_value / bow_n: the frames' vectors; frame_record:
        torch.int32 [n_frames].  Outputs: cand: torch.int32 [n_frames, max_candidates] (max_candidates = cand.shape[1]) keyframe indices
        in the reference's order, -1 beyond the count; ncand: torch.int32 [n_frames], the true count; pairs: torch.int32
        [n_frames * max_candidates, 2] and select: torch.int32 [n_frames * max_candidates], the pair table search_by_bow(), search_reloc()
        and solve_pnp() start from (n_frames * max_candidates <= max_pairs there); scores: torch.float32 [n_frames, n_keyframes] or None,
        the score of every scored keyframe and the NaN 0x7fc00000 elsewhere; common: torch.int32 [n_frames, n_keyframes] or None
        (mnRelocWords).  Asynchronous on the given stream, no host read."""
        nf = self.nfeatures
        n_kf = kf_bow_n.numel()
        n_frames = bow_n.numel()
        assert cand.dim() == 2 and cand.shape[0] == n_frames and cand.shape[1] >= 1, "cand is [n_frames, max_candidates]"
        max_cand = int(cand.shape[1])
        for w, v, n, m in ((kf_bow_word, kf_bow_value, kf_bow_n, n_kf), (bow_word, bow_value, bow_n, n_frames)):
            assert w.element_size() == 4 and w.is_contiguous() and w.numel() >= m * nf and n.element_size() == 4 and n.is_contiguous()
            assert v.element_size() == 8 and v.dtype.is_floating_point and v.is_contiguous() and v.numel() >= m * nf
        assert kf_neigh.element_size() == 4 and kf_neigh.is_contiguous() and kf_neigh.numel() == n_kf * 10, "kf_neigh is [n_keyframes, 10]"
        assert kf_record.element_size() == 4 and kf_record.is_contiguous() and kf_record.numel() >= n_kf
        assert kf_live is None or (kf_live.element_size() == 1 and kf_live.is_contiguous() and kf_live.numel() >= n_kf)
        assert kf_reloc_score is None or (kf_reloc_score.element_size() == 4 and kf_reloc_score.dtype.is_floating_point and kf_reloc_score.is_contiguous() and kf_reloc_score.numel() >= n_kf)
        assert frame_record.element_size() == 4 and frame_record.is_contiguous() and frame_record.numel() >= n_frames
        assert cand.element_size() == 4 and cand.is_contiguous() and ncand.element_size() == 4 and ncand.is_contiguous() and ncand.numel() >= n_frames
        assert pairs.element_size() == 4 and pairs.is_contiguous() and pairs.numel() >= n_frames * max_cand * 2
        assert select.element_size() == 4 and select.is_contiguous() and select.numel() >= n_frames * max_cand
        assert scores is None or (scores.element_size() == 4 and scores.dtype.is_floating_point and scores.is_contiguous() and scores.numel() >= n_frames * n_kf)
        assert common is None or (common.element_size() == 4 and common.is_contiguous() and common.numel() >= n_frames * n_kf)
        check(self._lib.ivf_tracker_reloc_candidates(self._h, vocabulary._h, kf_bow_word.data_ptr(), kf_bow_value.data_ptr(), kf_bow_n.data_ptr(),
                                                     None if kf_live is None else kf_live.data_ptr(), kf_neigh.data_ptr(),
                                                     None if kf_reloc_score is None else kf_reloc_score.data_ptr(), kf_record.data_ptr(), n_kf,
                                                     bow_word.data_ptr(), bow_value.data_ptr(), bow_n.data_ptr(), frame_record.data_ptr(), n_frames,
                                                     max_cand, cand.data_ptr(), ncand.data_ptr(), pairs.data_ptr(), select.data_ptr(),
                                                     None if scores is None else scores.data_ptr(),
                                                     None if common is None else common.data_ptr(), stream_ptr))

    def search_reloc(self, records, pairs, kf_points, assign, nmatches, th=10.0, orb_dist=100, select=None, poses=None, found=None,
                     check_orientation=True, point_quality=None, key_quality=None, stream_ptr=None):
        """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORB/src/ORBmatcher.cc:1520-1652) as
        Tracking::Relocalization runs it after its first pose (ORB/src/Tracking.cc:2375 with (10, 100), :2391 with (3, 64)), for n_pairs
        (keyframe, current) record pairs.  pairs: torch.int32 [n_pairs, 2]; select: torch.int32 [n_pairs] or None, 0 leaves a pair out
        (nmatches -2, assign untouched); poses: torch.float32 [n_pairs, 12] = CurrentFrame.mTcw or None = identity; kf_points:
        torch.uint8 view of LOCAL_POINT_DTYPE records [n_records, nfeatures] (80 B each), the map point each keypoint of each record holds
        (flags bit 0 = none / bad); found: torch.uint8 [n_pairs, nfeatures] by keyframe keypoint (sAlreadyFound) or None = the keyframe
        keypoints in assign on entry; assign: torch.int32 [n_pairs, nfeatures], in/out: the keyframe keypoint whose point each frame
        keypoint holds or -1, entries >= 0 on entry are occupied and kept; nmatches: torch.int32 [n_pairs] (nadditional);
        point_quality (by keyframe keypoint) / key_quality (by frame keypoint): torch.float32 [n_pairs, nfeatures] in/out or None.
        Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_pairs = pairs.shape[0]
        assert pairs.dtype.is_floating_point is False and pairs.element_size() == 4 and pairs.is_contiguous()
        assert assign.element_size() == 4 and assign.is_contiguous() and assign.numel() >= n_pairs * self.nfeatures and nmatches.numel() >= n_pairs
        assert select is None or (select.element_size() == 4 and select.is_contiguous() and select.numel() >= n_pairs)
        assert poses is None or (poses.is_contiguous() and poses.element_size() == 4 and poses.numel() == n_pairs * 12), "poses are per pair: [n_pairs, 12]"
        assert kf_points.is_contiguous() and kf_points.numel() * kf_points.element_size() >= n_rec * self.nfeatures * 80
        assert found is None or (found.element_size() == 1 and found.is_contiguous() and found.numel() >= n_pairs * self.nfeatures)
        for q in (point_quality, key_quality):
            assert q is None or (q.is_contiguous() and q.element_size() == 4 and q.numel() >= n_pairs * self.nfeatures)
        check(self._lib.ivf_tracker_search_reloc(self._h, records.data_ptr(), self.record_bytes, n_rec, pairs.data_ptr(), n_pairs,
                                                 None if select is None else select.data_ptr(),
                                                 None if poses is None else poses.data_ptr(), kf_points.data_ptr(),
                                                 None if found is None else found.data_ptr(), float(th), int(orb_dist),
                                                 int(bool(check_orientation)),
                                                 None if point_quality is None else point_quality.data_ptr(),
                                                 None if key_quality is None else key_quality.data_ptr(),
                                                 assign.data_ptr(), nmatches.data_ptr(), stream_ptr))

    def filter_assign(self, assign, mask=None, keep_when_set=True, found=None, stream_ptr=None):
        """The set bookkeeping of Tracking::Relocalization around search_reloc(), in place: assign[f, i] = -1 where (mask[f, i] != 0) !=
        keep_when_set (mask: torch.uint8 [n_frames, nfeatures] or None = nothing is dropped); then found[f, k] = 1 for every k still in
        assign[f], 0 elsewhere (found: torch.uint8 [n_frames, nfeatures] or None).  mask = solve_pnp()'s inlier, keep_when_set = True and
        found = sFound: Tracking.cc:2351-2361; mask = optimize_pose()'s outlier, keep_when_set = False: :2368-2370, :2398-2400.
        assign: torch.int32 [n_frames, nfeatures].  Asynchronous on the given stream."""
        n_frames = assign.numel() // self.nfeatures
        assert assign.element_size() == 4 and assign.is_contiguous() and assign.numel() == n_frames * self.nfeatures
        for m in (mask, found):
            assert m is None or (m.element_size() == 1 and m.is_contiguous() and m.numel() >= n_frames * self.nfeatures)
        check(self._lib.ivf_tracker_filter_assign(self._h, assign.data_ptr(), n_frames, None if mask is None else mask.data_ptr(),
                                                  int(bool(keep_when_set)), None if found is None else found.data_ptr(), stream_ptr))

    def optimize_pose(self, records, frames, xw, has_point, poses, outlier, ninliers, quality=None, n_rounds=4, chi2=None, stream_ptr=None):
        """Optimizer::PoseOptimization (ORB/src/Optimizer.cc:251-503) for n_frames frames in one kernel launch.  frames: torch.int32
        [n_frames] record indices; xw: torch.float32 [n_frames, nfeatures, 3] world position of the point each keypoint holds;
        has_point: torch.uint8 [n_frames, nfeatures]; quality: torch.float32 [n_frames, nfeatures] or None (= 1): the map point's quality
        score, which scales the edge's Huber width; poses: torch.float32 [n_frames, 12] in/out (mTcw -> the optimised pose);
        outlier: torch.uint8 [n_frames, nfeatures] (mvbOutlier); ninliers: torch.int32 [n_frames]; chi2: torch.float32
        [n_frames, nfeatures] or None (mvChi2 of the last round).  Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_frames = frames.numel()
        nf = self.nfeatures
        assert frames.element_size() == 4 and frames.is_contiguous() and poses.is_contiguous() and poses.element_size() == 4 and poses.numel() == n_frames * 12
        assert xw.is_contiguous() and xw.element_size() == 4 and xw.numel() >= n_frames * nf * 3
        assert has_point.element_size() == 1 and has_point.numel() >= n_frames * nf and outlier.element_size() == 1 and outlier.numel() >= n_frames * nf
        assert ninliers.element_size() == 4 and ninliers.numel() >= n_frames
        for q in (quality, chi2):
            assert q is None or (q.is_contiguous() and q.element_size() == 4 and q.numel() >= n_frames * nf)
        check(self._lib.ivf_tracker_optimize_pose(self._h, records.data_ptr(), self.record_bytes, n_rec, frames.data_ptr(), n_frames,
                                                  xw.data_ptr(), has_point.data_ptr(), None if quality is None else quality.data_ptr(),
                                                  int(n_rounds), poses.data_ptr(), outlier.data_ptr(), ninliers.data_ptr(),
                                                  None if chi2 is None else chi2.data_ptr(), stream_ptr))

    def update_local_map(self, map_view, frame_points, local_kf, n_local_kf, ref_kf, points, point_ids, point_offsets, n_local_points,
                         occupied, stream_ptr=None):
        """Tracking::UpdateLocalMap (ORB/src/Tracking.cc:2134-2270) for n_frames frames against one device-resident map, between the first
        optimize_pose() and search_local().  map_view: a MapView; frame_points: torch.int32 [n_frames, nfeatures] in/out, the map-point
        index every keypoint holds or -1 (a bad held point becomes -1); local_kf: torch.int32 [n_frames, max_local_keyframes] and
        n_local_kf: torch.int32 [n_frames], in/out like mvpLocalKeyFrames (kept for a frame without a vote); ref_kf: torch.int32
        [n_frames], written where there is a pKFmax; points: torch.uint8 view of LOCAL_POINT_DTYPE records [n_frames,
        max_points_per_frame] (max_points_per_frame = point_ids.shape[1]), point_ids: torch.int32 [n_frames, max_points_per_frame],
        point_offsets: torch.int32 [n_frames + 1] and occupied: torch.uint8 [n_frames, nfeatures], what search_local() takes;
        n_local_points: torch.int32 [n_frames], the true count.  Asynchronous on the given stream, no host read."""
        nf = self.nfeatures
        assert isinstance(map_view, MapView), "map_view is an iv_slam_amd.track.MapView"
        assert frame_points.dim() == 2 and frame_points.shape[1] == nf, "frame_points is [n_frames, nfeatures]"
        n_frames = int(frame_points.shape[0])
        assert local_kf.dim() == 2 and local_kf.shape[0] == n_frames and local_kf.shape[1] >= 1, "local_kf is [n_frames, max_local_keyframes]"
        assert point_ids.dim() == 2 and point_ids.shape[0] == n_frames and point_ids.shape[1] >= 1, "point_ids is [n_frames, max_points_per_frame]"
        max_lk, max_pts = int(local_kf.shape[1]), int(point_ids.shape[1])
        for x in (frame_points, local_kf, n_local_kf, ref_kf, point_ids, point_offsets, n_local_points):
            assert x.element_size() == 4 and x.is_contiguous() and not x.dtype.is_floating_point
        assert n_local_kf.numel() >= n_frames and ref_kf.numel() >= n_frames and n_local_points.numel() >= n_frames
        assert point_offsets.numel() >= n_frames + 1
        assert points.is_contiguous() and points.numel() * points.element_size() >= n_frames * max_pts * 80
        assert occupied.element_size() == 1 and occupied.is_contiguous() and occupied.numel() >= n_frames * nf
        check(self._lib.ivf_tracker_update_local_map(self._h, C.byref(map_view.c), frame_points.data_ptr(), n_frames, max_lk, max_pts,
                                                     local_kf.data_ptr(), n_local_kf.data_ptr(), ref_kf.data_ptr(), points.data_ptr(),
                                                     point_ids.data_ptr(), point_offsets.data_ptr(), n_local_points.data_ptr(),
                                                     occupied.data_ptr(), stream_ptr))

    def create_map_points(self, vocabulary, records, kf, neigh, poses, has_point, new_point, new_neigh, new_idx2, new_order, new_quality, n_new,
                          levelsup=4, key_quality=None, F12=None, kf_order=None, matches=None, stage=None, stream_ptr=None):
        """LocalMapping::CreateNewMapPoints (ORB/src/LocalMapping.cc:273-525), stereo / RGB-D branch, for n_kf keyframes at once: per
        neighbour in rank order the baseline gate, ComputeF12 (:609-626), ORBmatcher(0.6, false).SearchForTriangulation
        (ORB/src/ORBmatcher.cc:663-829) on feature vectors computed in the call, the triangulation and its gates (:352-497), and the new
        point's record (ORB/src/MapPoint.cc:247-376, min of the two key qualities :512-517).  vocabulary: an ORBVocabulary on the
        tracker's device; kf: torch.int32 [n_kf] record indices; neigh: torch.int32 [n_kf, max_neigh] (max_neigh = neigh.shape[1]),
        GetBestCovisibilityKeyFrames(10) in order, -1 padded, n_kf * max_neigh <= max_pairs; poses: torch.float32 [n_records, 12];
        has_point: torch.uint8 [n_records, nfeatures], read only; key_quality: torch.float32 [n_records, nfeatures] or None (= 1);
        F12: torch.float32 [n_kf, max_neigh, 9] or None (computed); kf_order: torch.int32 [n_records] or None (identity).  Outputs by
        keypoint of the current keyframe: new_point: torch.uint8 view of LOCAL_POINT_DTYPE records [n_kf, nfeatures]; new_neigh,
        new_idx2, new_order: torch.int32 [n_kf, nfeatures]; new_quality: torch.float32 [n_kf, nfeatures]; n_new: torch.int32 [n_kf];
        matches: torch.int32 and stage: torch.uint8 [n_kf, max_neigh, nfeatures] or None.  Slots are independent: each sees has_point
        as on entry.  Asynchronous on the given stream, no host read."""
        nf = self.nfeatures
        n_rec = records.numel() // self.record_bytes
        assert neigh.dim() == 2 and neigh.shape[1] >= 1, "neigh is [n_kf, max_neigh]"
        n_kf, max_neigh = int(neigh.shape[0]), int(neigh.shape[1])
        for x in (kf, neigh, new_neigh, new_idx2, new_order, n_new, kf_order, matches):
            assert x is None or (x.element_size() == 4 and x.is_contiguous() and not x.dtype.is_floating_point)
        assert kf.numel() == n_kf and n_new.numel() >= n_kf
        assert poses.is_contiguous() and poses.element_size() == 4 and poses.numel() == n_rec * 12, "poses are per RECORD: [n_records, 12]"
        assert has_point.element_size() == 1 and has_point.is_contiguous() and has_point.numel() >= n_rec * nf
        assert key_quality is None or (key_quality.is_contiguous() and key_quality.element_size() == 4 and key_quality.numel() >= n_rec * nf)
        assert F12 is None or (F12.is_contiguous() and F12.element_size() == 4 and F12.numel() == n_kf * max_neigh * 9), "F12 is [n_kf, max_neigh, 9]"
        assert kf_order is None or kf_order.numel() == n_rec, "kf_order is [n_records]"
        assert new_point.is_contiguous() and new_point.numel() * new_point.element_size() >= n_kf * nf * 80
        for x in (new_neigh, new_idx2, new_order):
            assert x.numel() >= n_kf * nf
        assert new_quality.is_contiguous() and new_quality.element_size() == 4 and new_quality.numel() >= n_kf * nf
        assert matches is None or matches.numel() >= n_kf * max_neigh * nf
        assert stage is None or (stage.element_size() == 1 and stage.is_contiguous() and stage.numel() >= n_kf * max_neigh * nf)
        opt = lambda x: None if x is None else x.data_ptr()
        check(self._lib.ivf_tracker_create_map_points(self._h, vocabulary._h, int(levelsup), records.data_ptr(), self.record_bytes, n_rec,
                                                      kf.data_ptr(), n_kf, neigh.data_ptr(), max_neigh, poses.data_ptr(), has_point.data_ptr(),
                                                      opt(key_quality), opt(F12), opt(kf_order), new_point.data_ptr(), new_neigh.data_ptr(),
                                                      new_idx2.data_ptr(), new_order.data_ptr(), new_quality.data_ptr(), n_new.data_ptr(),
                                                      opt(matches), opt(stage), stream_ptr))

    def merge_local(self, point_ids, point_offsets, assign, frame_points, stream_ptr=None):
        """ORBmatcher.cc:124 after search_local(): frame_points[f, i] = point_ids[point_offsets[f] + assign[f, i]] where assign >= 0.
        point_ids / point_offsets as update_local_map() wrote them; frame_points: torch.int32 [n_frames, nfeatures] in/out.  Asynchronous."""
        n_frames = frame_points.numel() // self.nfeatures
        assert frame_points.element_size() == 4 and frame_points.is_contiguous() and frame_points.numel() == n_frames * self.nfeatures
        assert point_offsets.element_size() == 4 and point_offsets.is_contiguous() and point_offsets.numel() >= n_frames + 1
        assert point_ids.element_size() == 4 and point_ids.is_contiguous()
        assert assign.element_size() == 4 and assign.is_contiguous() and assign.numel() >= n_frames * self.nfeatures
        check(self._lib.ivf_tracker_merge_local(self._h, point_ids.data_ptr(), point_offsets.data_ptr(), assign.data_ptr(), n_frames,
                                                frame_points.data_ptr(), stream_ptr))

    def points_from_map(self, map_view, frame_points, xw, has_point, quality=None, point_quality=None, stream_ptr=None):
        """optimize_pose()'s input over ALL the points a frame holds: xw[f, i] = GetWorldPos() of map point frame_points[f, i],
        has_point = 1 where there is one; quality: torch.float32 [n_frames, nfeatures] or None, the held point's entry of point_quality
        (torch.float32 [n_points], None = 1).  Asynchronous."""
        nf = self.nfeatures
        assert isinstance(map_view, MapView), "map_view is an iv_slam_amd.track.MapView"
        n_frames = frame_points.numel() // nf
        assert frame_points.element_size() == 4 and frame_points.is_contiguous() and frame_points.numel() == n_frames * nf
        assert xw.element_size() == 4 and xw.is_contiguous() and xw.numel() >= n_frames * nf * 3
        assert has_point.element_size() == 1 and has_point.numel() >= n_frames * nf
        assert quality is None or (quality.is_contiguous() and quality.element_size() == 4 and quality.numel() >= n_frames * nf)
        assert point_quality is None or (point_quality.is_contiguous() and point_quality.element_size() == 4 and point_quality.numel() >= map_view.c.n_points)
        check(self._lib.ivf_tracker_points_from_map(self._h, map_view.c.points, map_view.c.n_points,
                                                    None if point_quality is None else point_quality.data_ptr(), frame_points.data_ptr(),
                                                    n_frames, xw.data_ptr(), has_point.data_ptr(),
                                                    None if quality is None else quality.data_ptr(), stream_ptr))

    def close_local_map(self, map_view, outlier, frame_points, ninliers, only_tracking=False, stereo=True, stream_ptr=None):
        """The statistics loop of TrackLocalMap (ORB/src/Tracking.cc:1648-1677): ninliers[f] = held points optimize_pose() did not flag
        (with only_tracking False only those with Observations() > 0); with stereo an outlier's entry of frame_points becomes -1.
        outlier: torch.uint8 [n_frames, nfeatures]; frame_points: torch.int32 [n_frames, nfeatures] in/out; ninliers: torch.int32
        [n_frames].  The 30 / 50 decision is the caller's.  Asynchronous."""
        nf = self.nfeatures
        assert isinstance(map_view, MapView), "map_view is an iv_slam_amd.track.MapView"
        n_frames = frame_points.numel() // nf
        assert frame_points.element_size() == 4 and frame_points.is_contiguous() and frame_points.numel() == n_frames * nf
        assert outlier.element_size() == 1 and outlier.is_contiguous() and outlier.numel() >= n_frames * nf
        assert ninliers.element_size() == 4 and ninliers.is_contiguous() and ninliers.numel() >= n_frames
        check(self._lib.ivf_tracker_close_local_map(self._h, map_view.c.points, map_view.c.n_points, outlier.data_ptr(), n_frames,
                                                    int(bool(only_tracking)), int(bool(stereo)), frame_points.data_ptr(), ninliers.data_ptr(),
                                                    stream_ptr))

    def solve_pnp(self, records, frames, xw, has_point, draws, poses, inlier, ninliers, max_iterations=300, probability=0.99, min_inliers=10,
                  epsilon=0.5, th2=5.991, iterations=None, hyp_poses=None, hyp_ninliers=None, stream_ptr=None):
        """PnPsolver (ORB/src/PnPsolver.cc) as Tracking::Relocalization runs it (ORB/src/Tracking.cc:2315-2339) for n_frames frames at once:
        EPnP inside RANSAC, iterate() run to completion, Refine on the best inlier set.  frames: torch.int32 [n_frames] record indices;
        xw: torch.float32 [n_frames, nfeatures, 3] and has_point: torch.uint8 [n_frames, nfeatures] as points_from_keyframe() writes them;
        draws: torch.uint32-sized [n_frames, max_iterations, 4], the rand() values of the four samples of every iteration (pnp_draws());
        probability, min_inliers, epsilon, th2: SetRansacParameters' (0.99, 10, 0.5, 5.991 at Tracking.cc:2317), max_iterations 1..300;
        poses: torch.float32 [n_frames, 12], written only where a pose is returned; inlier: torch.uint8 [n_frames, nfeatures] (vbInliers);
        ninliers: torch.int32 [n_frames] (0: no pose, -1: bad record index); iterations: torch.int32 [n_frames] or None (mnIterations);
        hyp_poses: torch.float32 [n_frames, max_iterations, 12] and hyp_ninliers: torch.int32 [n_frames, max_iterations] or None: every
        hypothesis.  has_point & inlier is the has_point of the optimize_pose() that follows.  Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_frames = frames.numel()
        nf = self.nfeatures
        mi = int(max_iterations)
        assert frames.element_size() == 4 and frames.is_contiguous() and poses.is_contiguous() and poses.element_size() == 4 and poses.numel() == n_frames * 12
        assert xw.is_contiguous() and xw.element_size() == 4 and xw.numel() >= n_frames * nf * 3
        assert has_point.element_size() == 1 and has_point.numel() >= n_frames * nf and inlier.element_size() == 1 and inlier.numel() >= n_frames * nf
        assert draws.is_contiguous() and draws.element_size() == 4 and draws.numel() >= n_frames * mi * 4, "draws are [n_frames, max_iterations, 4]"
        assert ninliers.element_size() == 4 and ninliers.numel() >= n_frames
        assert iterations is None or (iterations.element_size() == 4 and iterations.numel() >= n_frames)
        assert hyp_poses is None or (hyp_poses.is_contiguous() and hyp_poses.element_size() == 4 and hyp_poses.numel() >= n_frames * mi * 12)
        assert hyp_ninliers is None or (hyp_ninliers.is_contiguous() and hyp_ninliers.element_size() == 4 and hyp_ninliers.numel() >= n_frames * mi)
        check(self._lib.ivf_tracker_solve_pnp(self._h, records.data_ptr(), self.record_bytes, n_rec, frames.data_ptr(), n_frames,
                                              xw.data_ptr(), has_point.data_ptr(), draws.data_ptr(), mi, float(probability), int(min_inliers),
                                              float(epsilon), float(th2), poses.data_ptr(), inlier.data_ptr(), ninliers.data_ptr(),
                                              None if iterations is None else iterations.data_ptr(),
                                              None if hyp_poses is None else hyp_poses.data_ptr(),
                                              None if hyp_ninliers is None else hyp_ninliers.data_ptr(), stream_ptr))

    def solve_sim3(self, records, pairs, poses, kf_xw, point_flags, match12, draws, sim3, inlier, ninliers, max_iterations=300, probability=0.99,
                   min_inliers=20, fix_scale=True, select=None, state=None, iterations=None, hyp_sim3=None, hyp_ninliers=None, stream_ptr=None):
        """Sim3Solver (ORB/src/Sim3Solver.cc) as LoopClosing::ComputeSim3 runs it (ORB/src/LoopClosing.cc:279-306) for n_pairs (current
        keyframe, candidate) record pairs at once: Horn's closed form on three point pairs inside RANSAC, from the state on entry to the
        first success or to mRansacMaxIts.  pairs: torch.int32 [n_pairs, 2] = (KF1, KF2) record indices; poses: torch.float32
        [n_records, 12] (Tcw); kf_xw: torch.float32 [n_records, nfeatures, 3] as points_from_keyframe() takes it; point_flags: torch.uint8
        [n_records, nfeatures], bit 0 = the keypoint holds a live map point; match12: torch.int32 [n_pairs, nfeatures] = the KF2 keypoint
        matched to KF1 keypoint i1 or -1 (vpMatched12); draws: torch.uint32-sized [n_pairs, max_iterations, 3], the rand() values of the
        three samples of every iteration (sim3_draws()); probability, min_inliers, max_iterations: SetRansacParameters' (0.99, 20, 300 at
        LoopClosing.cc:280), max_iterations 1..300; fix_scale: mbFixScale (true for stereo / RGB-D); select: torch.int32 [n_pairs] or None,
        0 leaves a pair out (ninliers -2); state: torch.int32 [n_pairs, 2] = {mnIterations, mnBestInliers} in/out or None ({0, 0}): a second
        call with the state of the first continues where the reference's next iterate() would.  sim3: torch.float32 [n_pairs, 16] = R12
        (9), t12 (3), s12, 3 zeros, written only on success; inlier: torch.uint8 [n_pairs, nfeatures] by i1 (vbInliers); ninliers:
        torch.int32 [n_pairs] (0: no transform, -1: bad record index, -2: not selected); iterations: torch.int32 [n_pairs] or None
        (mnIterations on return); hyp_sim3: torch.float32 [n_pairs, max_iterations, 16] and hyp_ninliers: torch.int32
        [n_pairs, max_iterations] or None: every hypothesis from the state's iteration to mRansacMaxIts.  (s12 R12, t12) is what ivf_search_by_sim3 takes next.
        Asynchronous on the given stream."""
        n_rec = records.numel() // self.record_bytes
        n_pairs = pairs.shape[0]
        nf = self.nfeatures
        mi = int(max_iterations)
        for x in (pairs, match12, ninliers, select, state, iterations, hyp_ninliers):
            assert x is None or (x.element_size() == 4 and x.is_contiguous() and not x.dtype.is_floating_point)
        assert poses.is_contiguous() and poses.element_size() == 4 and poses.numel() == n_rec * 12, "poses are per RECORD: [n_records, 12]"
        assert kf_xw.is_contiguous() and kf_xw.element_size() == 4 and kf_xw.numel() == n_rec * nf * 3, "kf_xw is [n_records, nfeatures, 3]"
        assert point_flags.element_size() == 1 and point_flags.is_contiguous() and point_flags.numel() >= n_rec * nf
        assert match12.numel() >= n_pairs * nf and ninliers.numel() >= n_pairs
        assert draws.is_contiguous() and draws.element_size() == 4 and draws.numel() >= n_pairs * mi * 3, "draws are [n_pairs, max_iterations, 3]"
        assert sim3.is_contiguous() and sim3.element_size() == 4 and sim3.numel() == n_pairs * 16, "sim3 is [n_pairs, 16]"
        assert inlier.element_size() == 1 and inlier.is_contiguous() and inlier.numel() >= n_pairs * nf
        assert select is None or select.numel() >= n_pairs
        assert state is None or state.numel() == n_pairs * 2, "state is [n_pairs, 2]"
        assert iterations is None or iterations.numel() >= n_pairs
        assert hyp_sim3 is None or (hyp_sim3.is_contiguous() and hyp_sim3.element_size() == 4 and hyp_sim3.numel() >= n_pairs * mi * 16)
        assert hyp_ninliers is None or hyp_ninliers.numel() >= n_pairs * mi
        opt = lambda x: None if x is None else x.data_ptr()
        check(self._lib.ivf_tracker_solve_sim3(self._h, records.data_ptr(), self.record_bytes, n_rec, pairs.data_ptr(), n_pairs, opt(select),
                                               poses.data_ptr(), kf_xw.data_ptr(), point_flags.data_ptr(), match12.data_ptr(), draws.data_ptr(), mi,
                                               float(probability), int(min_inliers), int(bool(fix_scale)), opt(state), sim3.data_ptr(),
                                               inlier.data_ptr(), ninliers.data_ptr(), opt(iterations), opt(hyp_sim3), opt(hyp_ninliers), stream_ptr))


def local_map_lds_keyframes():
    """update_local_map keeps a frame's vote row in LDS up to this many keyframes and in the handle's scratch beyond: the library's own limit"""
    return int(_lib.load().ivf_tracker_local_map_lds_keyframes())


class MapView:
    """ivf_map_view (include/ivfront.h) from tensors the caller keeps on the tracker's device: the map UpdateLocalMap walks, as flat
    tables.  points: torch.uint8 view of LOCAL_POINT_DTYPE records [n_points] (flags bit 0 = isBad(), bit 1 = Observations() > 0);
    obs_offsets [n_points + 1] / obs_kf: CSR of MapPoint::GetObservations() as keyframe indices; kf_point_offsets [n_keyframes + 1] /
    kf_points: CSR of KeyFrame::GetMapPointMatches() as map-point indices or -1; kf_neigh [n_keyframes, 10]:
    GetBestCovisibilityKeyFrames(10), -1 padded; kf_child_offsets [n_keyframes + 1] / kf_children: GetChilds(); kf_parent
    [n_keyframes]; kf_live: torch.uint8 [n_keyframes] or None (all live); kf_order: torch.int32 [n_keyframes] or None (identity), the
    order the host's std::map<KeyFrame*, int> iterates the keyframes in.  All index tensors are torch.int32 and contiguous.  The view
    keeps the tensors alive; an edit of the map (add, erase, SetBadFlag) is an edit of these tensors, or a new view after a resize."""

    def __init__(self, points, obs_offsets, obs_kf, kf_point_offsets, kf_points, kf_neigh, kf_child_offsets, kf_children, kf_parent,
                 kf_live=None, kf_order=None):
        n_points, n_kf = obs_offsets.numel() - 1, kf_parent.numel()
        for x in (obs_offsets, obs_kf, kf_point_offsets, kf_points, kf_neigh, kf_child_offsets, kf_children, kf_parent, kf_order):
            assert x is None or (x.element_size() == 4 and x.is_contiguous() and not x.dtype.is_floating_point), "index tables are contiguous int32"
        assert n_points >= 0 and points.is_contiguous() and points.numel() * points.element_size() == n_points * 80, "points / obs_offsets disagree"
        assert kf_point_offsets.numel() == n_kf + 1 and kf_child_offsets.numel() == n_kf + 1, "offset tables are [n_keyframes + 1]"
        assert kf_neigh.numel() == n_kf * 10, "kf_neigh is [n_keyframes, 10]"
        assert kf_live is None or (kf_live.element_size() == 1 and kf_live.is_contiguous() and kf_live.numel() == n_kf)
        assert kf_order is None or kf_order.numel() == n_kf, "kf_order is [n_keyframes]"
        self._keep = (points, obs_offsets, obs_kf, kf_point_offsets, kf_points, kf_neigh, kf_child_offsets, kf_children, kf_parent, kf_live, kf_order)
        c = _lib.MapViewC()
        for name, x in zip(("points", "obs_offsets", "obs_kf", "kf_point_offsets", "kf_points", "kf_neigh", "kf_child_offsets", "kf_children",
                            "kf_parent", "kf_live", "kf_order"), self._keep):
            setattr(c, name, None if x is None or x.numel() == 0 else x.data_ptr())
        c.n_points, c.n_keyframes = n_points, n_kf
        c.n_obs, c.n_kf_points, c.n_children = obs_kf.numel(), kf_points.numel(), kf_children.numel()
        self.c = c
        self.n_points, self.n_keyframes = n_points, n_kf


def ransac_draws(n, max_iterations, k, seed):
    """The sampling input of a RANSAC solver that draws k points per iteration: uint32 [n, max_iterations, k] values in [0, RAND_MAX] from
    numpy's generator (a host that wants the reference's own stream passes glibc rand() values instead)."""
    return np.random.default_rng(seed).integers(0, 2 ** 31, size=(int(n), int(max_iterations), int(k)), dtype=np.uint32)


def pnp_draws(n_frames, max_iterations, seed):
    """The sampling input of BatchTracker.solve_pnp: ransac_draws() with the four points of an EPnP hypothesis"""
    return ransac_draws(n_frames, max_iterations, 4, seed)


def sim3_draws(n_pairs, max_iterations, seed):
    """The sampling input of BatchTracker.solve_sim3: ransac_draws() with the three point pairs of a Horn hypothesis"""
    return ransac_draws(n_pairs, max_iterations, 3, seed)
