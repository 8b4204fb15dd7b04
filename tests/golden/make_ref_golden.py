"""Regenerates tests/golden/ref_orb_mini.npz: `python tests/golden/make_ref_golden.py`, where the reference tree is present.

Unlike the other fixtures here (make_golden.py freezes the ORACLE's outputs), this one records what the REFERENCE's own
ORBextractor.cc computes -- compiled unmodified against oracle/cvshim/ (tests/ref_lib.py, `make -C oracle ref`) -- on the inputs
stored in mini_320x200.npz, plain and with the cost map (300 features, 1.2, 8 levels, 20/7).  It holds recorded results only:
keypoints, descriptors, per-level counts, CRCs of the pyramid and quality-pyramid planes, and the constructor tables.  The
OpenCV primitives under the reference's logic are the oracle's (default variant), so the file pins the extractor's logic, not
OpenCV's arithmetic."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_lib as R  # noqa: E402

PARAMS = (300, 1.2, 8, 20, 7)
TABLES = ("scale", "inv_scale", "sigma2", "inv_sigma2", "features_per_level", "umax")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def record(make, img, cost):
    """the recorded fields of one extraction by `make(*PARAMS, introspection)` (ref_lib.Extractor here; the tests pass the
    oracle's and the device's through the same function)"""
    e = make(*PARAMS, cost is not None)
    k, d = e(img, cost)
    out = dict(kps=k, desc=d, level_counts=np.array(e.level_counts(), np.int32),
               pyr_crc=np.array([crc(e.pyramid(l)) for l in range(PARAMS[2])], np.uint32),
               pyr_dims=np.array([e.pyramid(l).shape for l in range(PARAMS[2])], np.int32))
    if cost is not None:
        out["qpyr_crc"] = np.array([crc(e.quality_pyramid(l)) for l in range(PARAMS[2])], np.uint32)
    t = e.tables()
    out.update({"tab_" + n: t[n] for n in TABLES})
    return out


def main():
    if not R.available():
        sys.exit(R.SKIP_REASON)
    g = np.load(os.path.join(HERE, "mini_320x200.npz"))
    out = os.path.join(HERE, "ref_orb_mini.npz")
    np.savez_compressed(out, **{"plain_" + k: v for k, v in record(R.Extractor, g["left"], None).items()},
                        **{"intro_" + k: v for k, v in record(R.Extractor, g["left"], g["cost"]).items()})
    print(os.path.basename(out), os.path.getsize(out), "mini_320x200.npz", os.path.getsize(os.path.join(HERE, "mini_320x200.npz")))


if __name__ == "__main__":
    main()
