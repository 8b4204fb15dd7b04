"""GPU: blocks 15-17 and the decoder of the FCN per channel against the f64 reference (probe networks, tests/fcn_probe.py), and the full cost
map of every golden case / of edge inputs against the f64 reference.  Every device step is a child process with its own timeout.

Each probe step prints its measured distances (PROBE lines: worst |logit - f64|, as a fraction of the bar, handle creation time).  On an MI355X the
product library stands at 0.35-0.46 of the bar, the three-f16 decoder at 0.46-0.54, the fp6 expansion at up to 0.96, batch 1 and batched alike; a probe
item takes 40-70 s, a full-map item 3 s; the tables are in DESIGN.md section 7.t."""
import json
import os
import subprocess
import sys

import pytest

import fcn_common as FC

pytestmark = pytest.mark.gpu


def _child(args, env, timeout):
    from iv_slam_amd import _lib
    e = dict(os.environ); e["IVF_REPO"] = FC.ROOT
    if env:
        assert os.path.exists(_lib.EXPERIMENT_LIB_PATH), "libivfront_exp.so missing: make -C iv_slam_amd/csrc EXPERIMENT=1"
        e.update(env); e["IVFRONT_LIB"] = _lib.EXPERIMENT_LIB_PATH
    r = subprocess.run([sys.executable] + args, env=e, capture_output=True, text=True, timeout=timeout, cwd=FC.ROOT)
    print(r.stdout[-6000:])
    return r


VARIANTS = {
    "product": {},
    # the decoder's 3x3 as three f16 products: no fp6 quantum, q = 0
    "decoder-three-f16-products": {"IVF_FCN_DEC6": "0"},
    # the expansion's correction products of blocks 15 / 16 on the fp6 matrix instruction
    "fp6-expansion": {"IVF_FCN_FP6": "1"},
    # block 17 as two workgroups per tile (k_fcn_irbd4<false>) instead of k_fcn_irbd4h
    "block-17-two-workgroups": {"IVF_FCN_HALF4": "0"},
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("tag", ["kitti", "jackal_smallw"])
def test_probes_match_the_f64_reference(tag, variant):
    """All 80 probes x 3 configurations of a case, every pixel, batch 1 (split schedule) and 20 images (batched kernels), ivf_fcn_status clean;
    |logit - f64| <= 4 E + q per pixel (tests/fcn_probe.py)."""
    env = VARIANTS[variant]
    dec6 = "0" if env.get("IVF_FCN_DEC6") == "0" else "1"
    r = _child([os.path.join(FC.ROOT, "tests", "fcn_probe.py"), tag, dec6], env, 800)
    lines = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith("PROBE ")]
    assert r.returncode == 0 and len(lines) == 3, r.stdout[-3000:] + r.stderr[-3000:]
    for l in lines:
        assert l["ratio_refs"] <= 0.25 + 1e-9
        assert l["ratio_single"] <= 1.0 and l["ratio_batched"] <= 1.0, l


_FULL_SCRIPT = r"""
import sys, os
sys.path.insert(0, os.environ["IVF_REPO"]); sys.path.insert(0, os.path.join(os.environ["IVF_REPO"], "tests"))
import numpy as np, torch
import fcn_common as FC, iv_slam_amd as iv
from iv_slam_amd import fcn_weights
import fcn_oracle64
tag, kind = sys.argv[1], sys.argv[2]
g, W, bgr, out = FC.load_case(tag)
if kind == "zeros": bgr = np.zeros_like(bgr)
elif kind == "full": bgr = np.full_like(bgr, 255)
elif kind == "checker":
    yy, xx = np.mgrid[0:bgr.shape[0], 0:bgr.shape[1]]
    bgr = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
ref, _l, _t = fcn_oracle64.forward(W, bgr, out, keep=lambda n: False)
NB = 20
f = iv.IntrospectionFCN(fcn_weights.pack_blob(W), bgr.shape[:2], out, max_batch=NB)
u8, cost = f(bgr, want_f32=True)
dev = torch.device("cuda:0")
cf = torch.empty((NB,) + tuple(out), dtype=torch.float32, device=dev)
f.forward_device(torch.from_numpy(np.stack([bgr] * NB)).to(dev), cost_f32=cf); f.status()
cb = cf.cpu().numpy()
assert all(np.array_equal(cb[i], cb[0]) for i in range(1, NB))
assert np.array_equal(u8, (cost * np.float32(255.0)).astype(np.uint8))
print("FULL %.4g %.4g" % (np.abs(cost - ref).max(), np.abs(cb[0] - ref).max()))
"""


@pytest.mark.parametrize("tag,kind", [(t, "image") for t in ("kitti", "jackal", "jackal_full", "kitti_smallw", "jackal_smallw", "kitti_bigw")] +
                         [("kitti", k) for k in ("zeros", "full", "checker")])
def test_full_cost_map_matches_the_f64_reference(tag, kind):
    """Every pixel of the cost map (the golden checks look at every 6th), batch 1 and the batched kernels, at the suite's 3e-4; edge inputs on kitti:
    all-0, all-255 and a one-pixel checkerboard."""
    r = _child(["-c", _FULL_SCRIPT, tag, kind], {}, 300)
    assert r.returncode == 0 and "FULL" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    single, batched = (float(v) for v in r.stdout.split("FULL")[1].split()[:2])
    assert single < 3e-4 and batched < 3e-4
