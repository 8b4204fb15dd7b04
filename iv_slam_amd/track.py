"""Batched, device-resident tracker step (ivf_tracker_* in include/ivfront.h): for every (last, cur) pair of gather records
the matcher part of Tracking::TrackWithMotionModel (ORB/src/Tracking.cc:1303-1330) -- UpdateLastFrame's stereo points,
ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, false) (ORB/src/ORBmatcher.cc:1372-1518), the retry with the wider
window -- in one launch sequence on the device.  torch tensors are only the device-memory plumbing."""
import ctypes as C
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import Bounds, TrackConfig, check

LOCAL_POINT_BYTES = _lib.LOCAL_POINT_DTYPE.itemsize                      # sizeof(ivf_local_point); _lib asserts the dtype's size
KF_NEIGH = 10                                                            # the neighbours a kf_neigh row holds: GetBestCovisibilityKeyFrames(10)
KF_NEIGH_IS = "kf_neigh is [n_keyframes, %d]" % KF_NEIGH
PNP_TAP_DOUBLES = 140                                                    # IVF_PNP_TAP_DOUBLES: the record of pnp_hypotheses() per hypothesis

# The kinds of tensor a pointer argument can be: (name, element size, floating point; None = either).
I32, F32, F64, U8 = ("int32", 4, False), ("float32", 4, True), ("float64", 8, True), ("uint8", 1, False)
ANY4 = ("4-byte", 4, None)                                               # draws: uint32 values in whatever 4-byte dtype holds them
BYTES = ("uint8 (bytes of records)", 1, False)                           # views of ivf_local_point / gather records: counted in bytes


def record_bytes(nfeatures):
    return int(_lib.load().ivf_track_record_bytes(int(nfeatures)))


def _given(x):
    if isinstance(x, torch.Tensor):
        return "%s %s on %s%s" % (x.dtype, tuple(x.shape), x.device, "" if x.is_contiguous() else ", not contiguous")
    return type(x).__name__ + (" on %s" % x.device if isinstance(x, MapView) else "")


def _require(ok, message, x):
    """an `assert` on the argument x that python -O keeps"""
    if not ok:
        raise AssertionError("%s, given %s" % (message, _given(x)))


def _tensor(name, x, ndim=None, what="a torch tensor"):
    """x for a method's shape arithmetic: a tensor, of ndim dimensions where that is given"""
    if not (isinstance(x, torch.Tensor) and ndim in (None, x.dim())):
        raise AssertionError("%s is %s, given %s" % (name, what, _given(x)))
    return x


def _ptr(device, name, x, kind, count=0, exact=False, optional=False, what=None):
    """The address the library receives for the argument `name`, and the one check before it: x is a tensor on `device`, contiguous,
    of the kind's element size and float / integer class, with at least `count` elements (exactly `count` where that count is a
    dimension the call states).  None passes as None where the argument is optional.  Looks at x's metadata only: no value is read,
    nothing synchronises; a size that only the device knows stays the library's to check."""
    if x is None and optional:
        return None
    kind_name, size, is_float = kind
    if (isinstance(x, torch.Tensor) and x.device == device and x.is_contiguous() and x.element_size() == size
            and is_float in (None, x.dtype.is_floating_point) and (x.numel() == count if exact else x.numel() >= count)):
        return x.data_ptr()
    raise AssertionError("%s: expected a contiguous %s tensor on %s with %s %d elements%s, given %s"
                         % (name, kind_name, device, "exactly" if exact else "at least", count, " (%s)" % what if what else "", _given(x)))


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
        self.device_id, self.device = device_id, torch.device("cuda", device_id)      # where every tensor of every call must live

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.ivf_tracker_destroy(self._h)
            self._h = None

    def _records(self, records):
        """(address, n_records) of a block of gather records"""
        n_rec = _tensor("records", records).numel() // self.record_bytes
        return _ptr(self.device, "records", records, BYTES, n_rec * self.record_bytes), n_rec

    def _pairs(self, pairs):
        """(address, n_pairs) of a pair table"""
        n_pairs = _tensor("pairs", pairs, 2, "[n_pairs, 2]").shape[0]
        return _ptr(self.device, "pairs", pairs, I32, n_pairs * 2, exact=True, what="pairs is [n_pairs, 2]"), n_pairs

    def _view(self, map_view):
        """the ivf_map_view of a MapView that lives where the tracker does"""
        _require(isinstance(map_view, MapView) and map_view.device == self.device, "map_view is an iv_slam_amd.track.MapView on the tracker's device", map_view)
        return map_view.c

    def run(self, records, pairs, assign, nmatches, poses=None, point_flags=None, point_quality=None, key_quality=None, stream_ptr=None):
        """records: torch.uint8 [n_records * record_bytes] (a packed block or the all-gathered buffer); pairs: torch.int32
        [n_pairs, 2] = (last, cur) record indices; assign: torch.int32 [n_pairs, nfeatures]; nmatches: torch.int32 [n_pairs];
        poses: torch.float32 [n_pairs, 2, 12] = per pair {LastFrame.mTcw, CurrentFrame.mTcw prior}, row-major 3x4, or None = zero
        motion; point_flags: torch.uint8 [n_records, nfeatures] or None; point_quality / key_quality: torch.float32
        [n_pairs, nfeatures] in/out (UpdateQualityScores on the device) or None.  Asynchronous on the given stream."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        (records_p, n_rec), (pairs_p, n_pairs) = self._records(records), self._pairs(pairs)
        check(self._lib.ivf_tracker_run(
            self._h, records_p, self.record_bytes, n_rec, pairs_p, n_pairs,
            p("poses", poses, F32, n_pairs * 24, exact=True, optional=True, what="poses are per PAIR: [n_pairs, 2, 12]"),
            p("point_flags", point_flags, U8, n_rec * nf, optional=True), p("point_quality", point_quality, F32, n_pairs * nf, optional=True),
            p("key_quality", key_quality, F32, n_pairs * nf, optional=True), p("assign", assign, I32, n_pairs * nf),
            p("nmatches", nmatches, I32, n_pairs), stream_ptr))

    def search_local(self, records, frames, points, point_offsets, max_points_per_frame, assign, nmatches, poses=None, occupied=None,
                     th=1.0, nn_ratio=0.8, cos_limit=0.5, point_quality=None, key_quality=None, stream_ptr=None):
        """Tracking::SearchLocalPoints (ORB/src/Tracking.cc:2088-2132) for n_frames frames at once: Frame::isInFrustum of every local
        map point, then ORBmatcher(nn_ratio).SearchByProjection(F, vpMapPoints, th).  frames: torch.int32 [n_frames] record indices;
        points: torch.uint8 view of LOCAL_POINT_DTYPE records (80 B each); point_offsets: torch.int32 [n_frames + 1] (CSR);
        poses: torch.float32 [n_frames, 12] (the pose of frame SLOT f) or None; occupied: torch.uint8 [n_frames, nfeatures] or None;
        assign: torch.int32 [n_frames, nfeatures] (index within the frame's point range or -1); nmatches: torch.int32 [n_frames];
        point_quality: torch.float32 indexed like points, key_quality: torch.float32 [n_frames, nfeatures] (both in/out) or None.
        Asynchronous on the given stream."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        (records_p, n_rec), n_frames = self._records(records), _tensor("frames", frames).numel()
        # points and point_quality hold point_offsets[n_frames] entries, which only the device knows: their size stays the library's to check
        check(self._lib.ivf_tracker_search_local(
            self._h, records_p, self.record_bytes, n_rec, p("frames", frames, I32, n_frames), n_frames,
            p("poses", poses, F32, n_frames * 12, exact=True, optional=True, what="poses are per frame SLOT: [n_frames, 12]"),
            p("points", points, BYTES), p("point_offsets", point_offsets, I32, n_frames + 1), int(max_points_per_frame),
            p("occupied", occupied, U8, n_frames * nf, optional=True), float(th), float(nn_ratio), float(cos_limit),
            p("point_quality", point_quality, F32, optional=True), p("key_quality", key_quality, F32, n_frames * nf, optional=True),
            p("assign", assign, I32, n_frames * nf), p("nmatches", nmatches, I32, n_frames), stream_ptr))

    def points_from_pairs(self, records, pairs, assign, xw, has_point, poses=None, stream_ptr=None):
        """The map points behind run()'s assignments: xw[p, i2] = Frame::UnprojectStereo(assign[p, i2]) of the LAST record of pair p under
        its last pose (ORB/src/Frame.cc:958-972), has_point[p, i2] = 1 where there is one.  pairs / poses / assign as run() took and
        wrote them; xw: torch.float32 [n_pairs, nfeatures, 3], has_point: torch.uint8 [n_pairs, nfeatures].  Asynchronous."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        (records_p, n_rec), (pairs_p, n_pairs) = self._records(records), self._pairs(pairs)
        check(self._lib.ivf_tracker_points_from_pairs(
            self._h, records_p, self.record_bytes, n_rec, pairs_p, n_pairs,
            p("poses", poses, F32, n_pairs * 24, exact=True, optional=True, what="poses are per PAIR: [n_pairs, 2, 12]"),
            p("assign", assign, I32, n_pairs * nf), p("xw", xw, F32, n_pairs * nf * 3), p("has_point", has_point, U8, n_pairs * nf), stream_ptr))

    def points_from_local(self, points, point_offsets, assign, xw, has_point, stream_ptr=None):
        """The map points behind search_local()'s assignments: xw[f, i] = points[point_offsets[f] + assign[f, i]].pos.  Asynchronous."""
        p, nf, n_frames = partial(_ptr, self.device), self.nfeatures, _tensor("point_offsets", point_offsets).numel() - 1
        check(self._lib.ivf_tracker_points_from_local(                             # points: sized on the device, as in search_local()
            self._h, p("points", points, BYTES), p("point_offsets", point_offsets, I32, n_frames + 1), p("assign", assign, I32, n_frames * nf),
            n_frames, p("xw", xw, F32, n_frames * nf * 3), p("has_point", has_point, U8, n_frames * nf), stream_ptr))

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
        p, nf = partial(_ptr, self.device), self.nfeatures
        (records_p, n_rec), (pairs_p, n_pairs) = self._records(records), self._pairs(pairs)
        check(self._lib.ivf_tracker_search_by_bow(
            self._h, vocabulary._h, int(levelsup), records_p, self.record_bytes, n_rec, pairs_p, n_pairs,
            p("select", select, I32, n_pairs, optional=True), p("point_flags", point_flags, U8, n_rec * nf, optional=True),
            float(nn_ratio), int(bool(check_orientation)), p("point_quality", point_quality, F32, n_pairs * nf, optional=True),
            p("key_quality", key_quality, F32, n_pairs * nf, optional=True), p("assign", assign, I32, n_pairs * nf),
            p("nmatches", nmatches, I32, n_pairs), stream_ptr))

    def points_from_keyframe(self, pairs, kf_xw, assign, xw, has_point, stream_ptr=None):
        """The map points behind search_by_bow()'s assignments: xw[p, i] = kf_xw[keyframe record of pair p, assign[p, i]], has_point = 1
        where there is one.  kf_xw: torch.float32 [n_records, nfeatures, 3] = GetWorldPos() of the point each keypoint of each record
        holds; pairs / assign as search_by_bow() took and wrote them.  Asynchronous."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        (pairs_p, n_pairs), n_rec = self._pairs(pairs), _tensor("kf_xw", kf_xw).numel() // (nf * 3)
        check(self._lib.ivf_tracker_points_from_keyframe(
            self._h, pairs_p, n_pairs, n_rec, p("kf_xw", kf_xw, F32, n_rec * nf * 3, exact=True, what="kf_xw is [n_records, nfeatures, 3]"),
            p("assign", assign, I32, n_pairs * nf), p("xw", xw, F32, n_pairs * nf * 3), p("has_point", has_point, U8, n_pairs * nf), stream_ptr))

    def bow_vectors(self, vocabulary, records, frames, bow_word, bow_value, bow_n, stream_ptr=None):
        """Frame::ComputeBoW's mBowVec (ORB/src/Frame.cc:683-694; TemplatedVocabulary.h:1126-1204 with TF_IDF / L1_NORM) for n_frames
        records at once, the first line of Tracking::Relocalization (ORB/src/Tracking.cc:2274) and what a keyframe brings to the database
        when it is inserted.  frames: torch.int32 [n_frames] record indices (any number of them); bow_word: torch.int32
        [n_frames, nfeatures], the words ascending, -1 beyond the count; bow_value: torch.float64 [n_frames, nfeatures]; bow_n:
        torch.int32 [n_frames], -1 for a record index outside the block.  Bit for bit what ORBVocabulary.transform gives on the same
        descriptors.  Asynchronous on the given stream."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        (records_p, n_rec), n_frames = self._records(records), _tensor("frames", frames).numel()
        check(self._lib.ivf_tracker_bow_vectors(
            self._h, vocabulary._h, records_p, self.record_bytes, n_rec, p("frames", frames, I32, n_frames), n_frames,
            p("bow_word", bow_word, I32, n_frames * nf), p("bow_value", bow_value, F64, n_frames * nf), p("bow_n", bow_n, I32, n_frames), stream_ptr))

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
        p, nf = partial(_ptr, self.device), self.nfeatures
        n_kf, n_frames = _tensor("kf_bow_n", kf_bow_n).numel(), _tensor("bow_n", bow_n).numel()
        max_cand = int(_tensor("cand", cand, 2, "[n_frames, max_candidates]").shape[1])
        _require(cand.shape[0] == n_frames and max_cand >= 1, "cand is [n_frames, max_candidates]", cand)
        check(self._lib.ivf_tracker_reloc_candidates(
            self._h, vocabulary._h, p("kf_bow_word", kf_bow_word, I32, n_kf * nf), p("kf_bow_value", kf_bow_value, F64, n_kf * nf),
            p("kf_bow_n", kf_bow_n, I32, n_kf), p("kf_live", kf_live, U8, n_kf, optional=True),
            p("kf_neigh", kf_neigh, I32, n_kf * KF_NEIGH, exact=True, what=KF_NEIGH_IS),
            p("kf_reloc_score", kf_reloc_score, F32, n_kf, optional=True), p("kf_record", kf_record, I32, n_kf), n_kf,
            p("bow_word", bow_word, I32, n_frames * nf), p("bow_value", bow_value, F64, n_frames * nf), p("bow_n", bow_n, I32, n_frames),
            p("frame_record", frame_record, I32, n_frames), n_frames, max_cand, p("cand", cand, I32, n_frames * max_cand, exact=True),
            p("ncand", ncand, I32, n_frames), p("pairs", pairs, I32, n_frames * max_cand * 2), p("select", select, I32, n_frames * max_cand),
            p("scores", scores, F32, n_frames * n_kf, optional=True), p("common", common, I32, n_frames * n_kf, optional=True), stream_ptr))

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
        p, nf = partial(_ptr, self.device), self.nfeatures
        (records_p, n_rec), (pairs_p, n_pairs) = self._records(records), self._pairs(pairs)
        check(self._lib.ivf_tracker_search_reloc(
            self._h, records_p, self.record_bytes, n_rec, pairs_p, n_pairs, p("select", select, I32, n_pairs, optional=True),
            p("poses", poses, F32, n_pairs * 12, exact=True, optional=True, what="poses are per pair: [n_pairs, 12]"),
            p("kf_points", kf_points, BYTES, n_rec * nf * LOCAL_POINT_BYTES), p("found", found, U8, n_pairs * nf, optional=True),
            float(th), int(orb_dist), int(bool(check_orientation)), p("point_quality", point_quality, F32, n_pairs * nf, optional=True),
            p("key_quality", key_quality, F32, n_pairs * nf, optional=True), p("assign", assign, I32, n_pairs * nf),
            p("nmatches", nmatches, I32, n_pairs), stream_ptr))

    def filter_assign(self, assign, mask=None, keep_when_set=True, found=None, stream_ptr=None):
        """The set bookkeeping of Tracking::Relocalization around search_reloc(), in place: assign[f, i] = -1 where (mask[f, i] != 0) !=
        keep_when_set (mask: torch.uint8 [n_frames, nfeatures] or None = nothing is dropped); then found[f, k] = 1 for every k still in
        assign[f], 0 elsewhere (found: torch.uint8 [n_frames, nfeatures] or None).  mask = solve_pnp()'s inlier, keep_when_set = True and
        found = sFound: Tracking.cc:2351-2361; mask = optimize_pose()'s outlier, keep_when_set = False: :2368-2370, :2398-2400.
        assign: torch.int32 [n_frames, nfeatures].  Asynchronous on the given stream."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        n_frames = _tensor("assign", assign).numel() // nf
        check(self._lib.ivf_tracker_filter_assign(
            self._h, p("assign", assign, I32, n_frames * nf, exact=True, what="assign is [n_frames, nfeatures]"), n_frames,
            p("mask", mask, U8, n_frames * nf, optional=True), int(bool(keep_when_set)), p("found", found, U8, n_frames * nf, optional=True), stream_ptr))

    def optimize_pose(self, records, frames, xw, has_point, poses, outlier, ninliers, quality=None, n_rounds=4, chi2=None, stream_ptr=None):
        """Optimizer::PoseOptimization (ORB/src/Optimizer.cc:251-503) for n_frames frames in one kernel launch.  frames: torch.int32
        [n_frames] record indices; xw: torch.float32 [n_frames, nfeatures, 3] world position of the point each keypoint holds;
        has_point: torch.uint8 [n_frames, nfeatures]; quality: torch.float32 [n_frames, nfeatures] or None (= 1): the map point's quality
        score, which scales the edge's Huber width; poses: torch.float32 [n_frames, 12] in/out (mTcw -> the optimised pose);
        outlier: torch.uint8 [n_frames, nfeatures] (mvbOutlier); ninliers: torch.int32 [n_frames]; chi2: torch.float32
        [n_frames, nfeatures] or None (mvChi2 of the last round).  Asynchronous on the given stream."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        (records_p, n_rec), n_frames = self._records(records), _tensor("frames", frames).numel()
        check(self._lib.ivf_tracker_optimize_pose(
            self._h, records_p, self.record_bytes, n_rec, p("frames", frames, I32, n_frames), n_frames, p("xw", xw, F32, n_frames * nf * 3),
            p("has_point", has_point, U8, n_frames * nf), p("quality", quality, F32, n_frames * nf, optional=True), int(n_rounds),
            p("poses", poses, F32, n_frames * 12, exact=True, what="poses are per frame: [n_frames, 12]"), p("outlier", outlier, U8, n_frames * nf),
            p("ninliers", ninliers, I32, n_frames), p("chi2", chi2, F32, n_frames * nf, optional=True), stream_ptr))

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
        p, nf = partial(_ptr, self.device), self.nfeatures
        n_frames = int(_tensor("frame_points", frame_points, 2, "[n_frames, nfeatures]").shape[0])
        max_lk = int(_tensor("local_kf", local_kf, 2, "[n_frames, max_local_keyframes]").shape[1])
        max_pts = int(_tensor("point_ids", point_ids, 2, "[n_frames, max_points_per_frame]").shape[1])
        _require(frame_points.shape[1] == nf, "frame_points is [n_frames, nfeatures]", frame_points)
        _require(local_kf.shape[0] == n_frames and max_lk >= 1, "local_kf is [n_frames, max_local_keyframes]", local_kf)
        _require(point_ids.shape[0] == n_frames and max_pts >= 1, "point_ids is [n_frames, max_points_per_frame]", point_ids)
        check(self._lib.ivf_tracker_update_local_map(
            self._h, C.byref(self._view(map_view)), p("frame_points", frame_points, I32, n_frames * nf, exact=True), n_frames, max_lk, max_pts,
            p("local_kf", local_kf, I32, n_frames * max_lk, exact=True), p("n_local_kf", n_local_kf, I32, n_frames), p("ref_kf", ref_kf, I32, n_frames),
            p("points", points, BYTES, n_frames * max_pts * LOCAL_POINT_BYTES), p("point_ids", point_ids, I32, n_frames * max_pts, exact=True),
            p("point_offsets", point_offsets, I32, n_frames + 1), p("n_local_points", n_local_points, I32, n_frames),
            p("occupied", occupied, U8, n_frames * nf), stream_ptr))

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
        p, nf = partial(_ptr, self.device), self.nfeatures
        records_p, n_rec = self._records(records)
        n_kf, max_neigh = map(int, _tensor("neigh", neigh, 2, "[n_kf, max_neigh]").shape)
        _require(max_neigh >= 1, "neigh is [n_kf, max_neigh]", neigh)
        check(self._lib.ivf_tracker_create_map_points(
            self._h, vocabulary._h, int(levelsup), records_p, self.record_bytes, n_rec, p("kf", kf, I32, n_kf, exact=True, what="kf is [n_kf]"), n_kf,
            p("neigh", neigh, I32, n_kf * max_neigh, exact=True), max_neigh,
            p("poses", poses, F32, n_rec * 12, exact=True, what="poses are per RECORD: [n_records, 12]"), p("has_point", has_point, U8, n_rec * nf),
            p("key_quality", key_quality, F32, n_rec * nf, optional=True),
            p("F12", F12, F32, n_kf * max_neigh * 9, exact=True, optional=True, what="F12 is [n_kf, max_neigh, 9]"),
            p("kf_order", kf_order, I32, n_rec, exact=True, optional=True, what="kf_order is [n_records]"),
            p("new_point", new_point, BYTES, n_kf * nf * LOCAL_POINT_BYTES), p("new_neigh", new_neigh, I32, n_kf * nf),
            p("new_idx2", new_idx2, I32, n_kf * nf), p("new_order", new_order, I32, n_kf * nf), p("new_quality", new_quality, F32, n_kf * nf),
            p("n_new", n_new, I32, n_kf), p("matches", matches, I32, n_kf * max_neigh * nf, optional=True),
            p("stage", stage, U8, n_kf * max_neigh * nf, optional=True), stream_ptr))

    def merge_local(self, point_ids, point_offsets, assign, frame_points, stream_ptr=None):
        """ORBmatcher.cc:124 after search_local(): frame_points[f, i] = point_ids[point_offsets[f] + assign[f, i]] where assign >= 0.
        point_ids / point_offsets as update_local_map() wrote them; frame_points: torch.int32 [n_frames, nfeatures] in/out.  Asynchronous."""
        p, nf = partial(_ptr, self.device), self.nfeatures
        n_frames = _tensor("frame_points", frame_points).numel() // nf
        # point_ids is update_local_map()'s [n_frames, max_points_per_frame >= 1], the width not told here: one entry per frame at least
        check(self._lib.ivf_tracker_merge_local(
            self._h, p("point_ids", point_ids, I32, n_frames), p("point_offsets", point_offsets, I32, n_frames + 1), p("assign", assign, I32, n_frames * nf), n_frames,
            p("frame_points", frame_points, I32, n_frames * nf, exact=True, what="frame_points is [n_frames, nfeatures]"), stream_ptr))

    def points_from_map(self, map_view, frame_points, xw, has_point, quality=None, point_quality=None, stream_ptr=None):
        """optimize_pose()'s input over ALL the points a frame holds: xw[f, i] = GetWorldPos() of map point frame_points[f, i],
        has_point = 1 where there is one; quality: torch.float32 [n_frames, nfeatures] or None, the held point's entry of point_quality
        (torch.float32 [n_points], None = 1).  Asynchronous."""
        p, nf, view = partial(_ptr, self.device), self.nfeatures, self._view(map_view)
        n_frames = _tensor("frame_points", frame_points).numel() // nf
        check(self._lib.ivf_tracker_points_from_map(
            self._h, view.points, view.n_points, p("point_quality", point_quality, F32, view.n_points, optional=True),
            p("frame_points", frame_points, I32, n_frames * nf, exact=True, what="frame_points is [n_frames, nfeatures]"), n_frames,
            p("xw", xw, F32, n_frames * nf * 3), p("has_point", has_point, U8, n_frames * nf),
            p("quality", quality, F32, n_frames * nf, optional=True), stream_ptr))

    def close_local_map(self, map_view, outlier, frame_points, ninliers, only_tracking=False, stereo=True, stream_ptr=None):
        """The statistics loop of TrackLocalMap (ORB/src/Tracking.cc:1648-1677): ninliers[f] = held points optimize_pose() did not flag
        (with only_tracking False only those with Observations() > 0); with stereo an outlier's entry of frame_points becomes -1.
        outlier: torch.uint8 [n_frames, nfeatures]; frame_points: torch.int32 [n_frames, nfeatures] in/out; ninliers: torch.int32
        [n_frames].  The 30 / 50 decision is the caller's.  Asynchronous."""
        p, nf, view = partial(_ptr, self.device), self.nfeatures, self._view(map_view)
        n_frames = _tensor("frame_points", frame_points).numel() // nf
        check(self._lib.ivf_tracker_close_local_map(
            self._h, view.points, view.n_points, p("outlier", outlier, U8, n_frames * nf), n_frames, int(bool(only_tracking)), int(bool(stereo)),
            p("frame_points", frame_points, I32, n_frames * nf, exact=True, what="frame_points is [n_frames, nfeatures]"),
            p("ninliers", ninliers, I32, n_frames), stream_ptr))

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
        p, nf, mi = partial(_ptr, self.device), self.nfeatures, int(max_iterations)
        (records_p, n_rec), n_frames = self._records(records), _tensor("frames", frames).numel()
        check(self._lib.ivf_tracker_solve_pnp(
            self._h, records_p, self.record_bytes, n_rec, p("frames", frames, I32, n_frames), n_frames, p("xw", xw, F32, n_frames * nf * 3),
            p("has_point", has_point, U8, n_frames * nf), p("draws", draws, ANY4, n_frames * mi * 4, what="draws are [n_frames, max_iterations, 4]"),
            mi, float(probability), int(min_inliers), float(epsilon), float(th2),
            p("poses", poses, F32, n_frames * 12, exact=True, what="poses are per frame: [n_frames, 12]"), p("inlier", inlier, U8, n_frames * nf),
            p("ninliers", ninliers, I32, n_frames), p("iterations", iterations, I32, n_frames, optional=True),
            p("hyp_poses", hyp_poses, F32, n_frames * mi * 12, optional=True), p("hyp_ninliers", hyp_ninliers, I32, n_frames * mi, optional=True),
            stream_ptr))

    def pnp_hypotheses(self, records, frames, xw, has_point, draws, taps, hyp_poses, hyp_ninliers, max_iterations=300, probability=0.99,
                       min_inliers=10, epsilon=0.5, th2=5.991, stream_ptr=None):
        """Testing hook (ivf_test_pnp_hypotheses): the hypotheses of solve_pnp() on the same inputs, without the bookkeeping and Refine
        after them.  hyp_poses: torch.float32 [n_frames, max_iterations, 12] and hyp_ninliers: torch.int32 [n_frames, max_iterations]
        as solve_pnp() writes them; taps: torch.float64 [n_frames, max_iterations, PNP_TAP_DOUBLES], one record per iteration below
        mRansacMaxIts (the layout: include/ivfront.h).  Asynchronous on the given stream."""
        p, nf, mi = partial(_ptr, self.device), self.nfeatures, int(max_iterations)
        (records_p, n_rec), n_frames = self._records(records), _tensor("frames", frames).numel()
        check(self._lib.ivf_test_pnp_hypotheses(
            self._h, records_p, self.record_bytes, n_rec, p("frames", frames, I32, n_frames), n_frames, p("xw", xw, F32, n_frames * nf * 3),
            p("has_point", has_point, U8, n_frames * nf), p("draws", draws, ANY4, n_frames * mi * 4, what="draws are [n_frames, max_iterations, 4]"),
            mi, float(probability), int(min_inliers), float(epsilon), float(th2),
            p("taps", taps, F64, n_frames * mi * PNP_TAP_DOUBLES, what="taps are [n_frames, max_iterations, %d]" % PNP_TAP_DOUBLES),
            p("hyp_poses", hyp_poses, F32, n_frames * mi * 12), p("hyp_ninliers", hyp_ninliers, I32, n_frames * mi), stream_ptr))

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
        [n_pairs, max_iterations] or None: every hypothesis from the state's iteration to mRansacMaxIts.  match12 is what LoopSearch.search_by_bow_keyframes
        writes; sim3, inlier and (ninliers > 0) are what LoopSearch.search_by_sim3 takes next (iv_slam_amd/loop.py).
        Asynchronous on the given stream."""
        p, nf, mi = partial(_ptr, self.device), self.nfeatures, int(max_iterations)
        (records_p, n_rec), (pairs_p, n_pairs) = self._records(records), self._pairs(pairs)
        check(self._lib.ivf_tracker_solve_sim3(
            self._h, records_p, self.record_bytes, n_rec, pairs_p, n_pairs, p("select", select, I32, n_pairs, optional=True),
            p("poses", poses, F32, n_rec * 12, exact=True, what="poses are per RECORD: [n_records, 12]"),
            p("kf_xw", kf_xw, F32, n_rec * nf * 3, exact=True, what="kf_xw is [n_records, nfeatures, 3]"),
            p("point_flags", point_flags, U8, n_rec * nf), p("match12", match12, I32, n_pairs * nf),
            p("draws", draws, ANY4, n_pairs * mi * 3, what="draws are [n_pairs, max_iterations, 3]"),
            mi, float(probability), int(min_inliers), int(bool(fix_scale)),
            p("state", state, I32, n_pairs * 2, exact=True, optional=True, what="state is [n_pairs, 2]"),
            p("sim3", sim3, F32, n_pairs * 16, exact=True, what="sim3 is [n_pairs, 16]"), p("inlier", inlier, U8, n_pairs * nf),
            p("ninliers", ninliers, I32, n_pairs), p("iterations", iterations, I32, n_pairs, optional=True),
            p("hyp_sim3", hyp_sim3, F32, n_pairs * mi * 16, optional=True), p("hyp_ninliers", hyp_ninliers, I32, n_pairs * mi, optional=True),
            stream_ptr))


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
        n_points, n_kf = _tensor("obs_offsets", obs_offsets).numel() - 1, _tensor("kf_parent", kf_parent).numel()
        n_obs, n_kf_points, n_children = _tensor("obs_kf", obs_kf).numel(), _tensor("kf_points", kf_points).numel(), _tensor("kf_children", kf_children).numel()
        _require(n_points >= 0, "obs_offsets is [n_points + 1]", obs_offsets)
        self.device = _tensor("points", points).device                       # every table lives where the points do

        def p(name, x, kind, count, **kw):                                   # an empty table reaches the library as NULL
            ptr = _ptr(self.device, name, x, kind, count, exact=True, **kw)
            return ptr if count else None
        self.c = _lib.MapViewC(
            points=p("points", points, BYTES, n_points * LOCAL_POINT_BYTES, what="points / obs_offsets disagree"),
            obs_offsets=p("obs_offsets", obs_offsets, I32, n_points + 1), obs_kf=p("obs_kf", obs_kf, I32, n_obs),
            kf_point_offsets=p("kf_point_offsets", kf_point_offsets, I32, n_kf + 1, what="offset tables are [n_keyframes + 1]"),
            kf_points=p("kf_points", kf_points, I32, n_kf_points),
            kf_live=p("kf_live", kf_live, U8, n_kf, optional=True), kf_neigh=p("kf_neigh", kf_neigh, I32, n_kf * KF_NEIGH, what=KF_NEIGH_IS),
            kf_child_offsets=p("kf_child_offsets", kf_child_offsets, I32, n_kf + 1, what="offset tables are [n_keyframes + 1]"),
            kf_children=p("kf_children", kf_children, I32, n_children), kf_parent=p("kf_parent", kf_parent, I32, n_kf),
            kf_order=p("kf_order", kf_order, I32, n_kf, optional=True, what="kf_order is [n_keyframes]"),
            n_points=n_points, n_keyframes=n_kf, n_obs=n_obs, n_kf_points=n_kf_points, n_children=n_children)
        self._keep = (points, obs_offsets, obs_kf, kf_point_offsets, kf_points, kf_neigh, kf_child_offsets, kf_children, kf_parent, kf_live, kf_order)
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
