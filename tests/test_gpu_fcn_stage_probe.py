"""GPU: the FCN's stem and blocks 1-14 per channel, pixel and phase against the f64 reference, through the probe networks of
tests/fcn_stage_probe.py (product library only).  Every channel-phase of every stage is read: all 16 phases of the two 256 x 256 stages (stem,
block 1), all 4 of the 128 x 128 stages (blocks 2, 3).

One device step per golden case: a fresh child process with its own timeout runs all fifteen stages on the case's shared prefix (batch 1: the
split schedule; 20 identical images: the batched kernels; ivf_fcn_status clean; batch slots bit-identical) and prints one PROBE line per stage and
an OVER line per probe above its bar.  The step runs ONCE per case, whatever its end: its result -- a time-out and a non-zero exit included -- is
kept, and each (case, stage) item asserts on that record without touching the GPU again.  So the first item of a case carries the child's time
(about half a minute) and the other fourteen none; and when the child ends early at stage k, stages k + 1 .. 14 fail with "no PROBE line": the FIRST
failing stage of a case is the one to read."""
import json
import os
import subprocess
import sys

import pytest

import fcn_common as FC
import fcn_stage_probe as SP

pytestmark = pytest.mark.gpu

_RESULTS = {}        # tag -> (return code or None after a time-out, {stage: PROBE dictionary}, [OVER lines], tail of the output)


def _case(tag):
    if tag in _RESULTS:
        return _RESULTS[tag]
    e = dict(os.environ); e["IVF_REPO"] = FC.ROOT
    e.pop("IVFRONT_LIB", None)                        # product library only
    args = [sys.executable, os.path.join(FC.ROOT, "tests", "fcn_stage_probe.py"), tag] + [str(k) for k in range(SP.NSTAGES)]
    _RESULTS[tag] = (None, {}, [], "the device step did not finish")          # whatever happens below, the step is not started again
    try:
        r = subprocess.run(args, env=e, capture_output=True, text=True, timeout=300, cwd=FC.ROOT)
        rc, out, err = r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired as t:
        dec = lambda b: b.decode("utf-8", "replace") if isinstance(b, bytes) else (b or "")
        rc, out, err = None, dec(t.stdout), dec(t.stderr) + "\nTIMED OUT after 300 s"
    print(out[-12000:])
    lines = {}
    for l in out.splitlines():
        if l.startswith("PROBE "):
            d = json.loads(l[6:]); lines[d["stage"]] = d
    over = [l for l in out.splitlines() if l.startswith("OVER ")]
    _RESULTS[tag] = (rc, lines, over, out[-2000:] + err[-3000:])
    return _RESULTS[tag]


@pytest.mark.parametrize("k", range(SP.NSTAGES))
@pytest.mark.parametrize("tag", ["kitti", "jackal_smallw"])
def test_stage_matches_the_f64_reference(tag, k):
    """|logit - f64| <= 4 E + q on every pixel of every probe of the stage, batch 1 and batched; the f32 restatements at <= 0.25 of the bar;
    the child ended by itself with every stage inside its bar (exit 0) or with some stage over it (exit 1), never by a signal or a time-out."""
    rc, lines, over, tail = _case(tag)
    mine = [l for l in over if l.startswith("OVER %s %d " % (tag, k))]
    assert k in lines, "no PROBE line for stage %d (exit %s; stages done: %s)\n" % (k, rc, sorted(lines)) + tail
    l = lines[k]
    print("PROBE " + json.dumps(l))
    assert l["probes"] == len(SP.groups(k))
    assert l["ratio_refs"] <= 0.25 + 1e-9
    assert l["ratio_single"] <= 1.0 and l["ratio_batched"] <= 1.0, "\n".join(mine[:40]) + "\n" + json.dumps(l)
    assert rc == (1 if over else 0) and "WORST" in tail, "the device step ended with exit %s\n" % rc + tail
