"""Probe networks for the FCN's stem and blocks 1-14: ordinary weight dictionaries (pack_blob) that make single channels of ANY stage's output
readable in the cost map, so that k_fcn_stem, k_fcn_irb, k_fcn_irb64 / k_fcn_irbd2, the split small-batch schedule and the tile-major layouts
between them are compared per channel and pixel with the f64 reference (oracle/fcn_oracle64.py).  tests/fcn_probe.py does this for blocks 15-17.

Stage k (0 = the stem, 1 .. 14 = the blocks) keeps the golden case's weights up to and including stage k; everything after it is a READER TAIL:
  * residual blocks after k are transparent (fcn_probe.transparent: projection BatchNorm gamma = beta = 0, an exact pass-through);
  * the non-residual blocks after k (of 1, 2, 4, 7, 11, 14, 17) are SELECTOR blocks carrying the G channels of one group: expansion row j has a single
    1 at the input channel it carries, BatchNorm (mean 0, var 1) gamma s_j, beta b_j with s x + b inside [0.75, 5.25] over the whole map (f64 tap; no
    ReLU6 ever clips), depthwise one tap of 1 with an identity BatchNorm, projection 1 / s_j at [j, j] and beta -b_j / s_j; all other rows are zero.
    Block 1 has no expansion: its depthwise layer's BatchNorm holds s and b;
  * stride-2 selector blocks (2 and 4) pick a phase with the depthwise tap (1 + p_y, 1 + p_x): out(i, j) = in(2 i + p_y, 2 j + p_x).  A 128 x 128 stage
    (blocks 2, 3) is read in 4 phases (o_y, o_x) < 2 through block 4, a 256 x 256 stage (stem, block 1) in 16 phases (o_y, o_x) < 4 through blocks
    2 and 4: the probe sees stage pixel (4 i + o_y, 4 j + o_x), block 2 taking the low bit of o and block 4 the high one;
  * the decoder is fcn_probe's: centre-tap +-1 selector rows, beta above the largest |x|, conv_last over the group scaled into logits of 0.5 +- 0.1,
    out size 64 x 64, logit recovered in double from the f32 cost.
Nothing in the tail needs to be exact: the f64 reference OF THE PROBE NETWORK defines the expected logits.  Outside the group the tail carries zeros,
so the decoder's fp6 scale blocks (fcn_probe.scale_block; the group sits in block-17 channels 0 .. G-1) see the group's own magnitudes only.

The references evaluate the tail on the carried channels alone (tail_logits): a row whose BatchNorm gamma and beta are zero is exactly 0 in every
precision and a zero weight contributes an exact 0, and every sum of the selector path has ONE non-zero term -- so the oracles' own primitives on
the sliced tensors give bit for bit what the f32 oracles give on the whole network, and the f64 one to 1e-14 (tests/test_fcn_stage_probe_cpu.py
checks that per stage), at a hundredth of the time.  conv_last, the one sum with several terms, runs unsliced on all 80 decoder rows.

The bar is DESIGN 7.t's, per probe and pixel:  4 E + q,  E = the larger distance of the two f32 restatements' logits from f64 through the same probe
network (prefix in f32 from the image, then the tail), q = 2^-15 |conv_last scale| sum over the group of the scale block's largest |x| at that pixel
(f64 tap of block 17's output).  Nothing in it comes from the device.
"""
import json
import os
import sys
import time

import numpy as np

import fcn_common as FC
from fcn_probe import transparent, trunc_f16, logits_from_cost, scale_block, TRANSPARENT_OK

SELECTORS = (1, 2, 4, 7, 11, 14, 17)
NSTAGES = 15
SUFF = (".weight", ".bias", ".running_mean", ".running_var")
# tiles of the kernel that writes stage k, (width, height) in stage pixels, from the comments in ivf_fcn.hip: k_fcn_stem 32 x 8 (stem and block 1's
# depthwise in one kernel), k_fcn_irb 32 x TH (TH = 2 at stride 2, 4 at stride 1), blocks 5-7 strips of 4 rows x 64 columns with half-row waves
# (seam at column 32), blocks 8-14 strips of 8 x 32 of the (y & 1, x & 1) sub-images: image rows 16 m + (0 | 1) start a strip.
TILE = {0: (32, 8), 1: (32, 8), 2: (32, 2), 3: (32, 4), 4: (32, 2), 5: (32, 4), 6: (32, 4), 7: (32, 4)}
# group size per stage: the largest of 16, 8, 4, 2, 1 at which tests/test_fcn_stage_probe_cpu.py holds on both cases -- with 16, fault (d) falls below 2 x the
# bar on each of blocks 1 and 4-14, and blocks 2 and 3 have 24 channels
GROUP = {k: 16 if k == 0 else 8 for k in range(NSTAGES)}


def stage_name(k):
    return "f0" if k == 0 else "block%d" % k


def stage_channels(k):
    from iv_slam_amd.fcn_weights import BLOCKS
    return 32 if k == 0 else BLOCKS[k - 1][1]


def stage_stride(k):
    """stage pixels per probe pixel and axis: 4 at 256 x 256, 2 at 128 x 128, 1 at 64 x 64"""
    return 4 if k <= 1 else 2 if k <= 3 else 1


def phases(k):
    n = stage_stride(k)
    return [(oy, ox) for oy in range(n) for ox in range(n)]


def groups(k, group=None, phase_list=None):
    """[(channels, phase)]: every channel-phase of stage k exactly once (phase_list: a subset of the phases)"""
    g = group or GROUP[k]
    c = stage_channels(k)
    assert c % g == 0
    return [(list(range(a, a + g)), ph) for ph in (phase_list or phases(k)) for a in range(0, c, g)]


def at_phase(x, k, phase):
    """[.., H, W] of stage k -> the [.., 64, 64] pixels a probe of that phase reads"""
    n = stage_stride(k)
    return x[..., phase[0]::n, phase[1]::n]


def sign_patterns(g):
    """candidate sign patterns (first sign +): all of them up to 4 channels, 16 Walsh rows beyond"""
    if g <= 4:
        return [tuple(1.0 if i == 0 or not (m >> (i - 1)) & 1 else -1.0 for i in range(g)) for m in range(2 ** (g - 1))]
    pats = {tuple(-1.0 if bin(m & i).count("1") & 1 else 1.0 for i in range(g)) for m in range(16)}
    return sorted(pats, reverse=True)


# ---- the three arithmetics: the oracles' own primitives on sliced tensors ----

class _Np:
    name = "numpy"

    def __init__(self):
        import fcn_oracle
        self.o = fcn_oracle

    def arr(self, x):
        return np.ascontiguousarray(x, np.float32)

    def conv(self, x, w, s=1, p=0, d=1, g=1):
        return self.o.conv2d(x, np.ascontiguousarray(w, np.float32), s, p, d, g)

    def bn(self, x, V, p, idx):
        return self.o.bn(x, {p + s: V[p + s][idx] for s in SUFF}, p)

    def relu6(self, x):
        return self.o.relu6(x)

    def relu(self, x):
        return np.maximum(x, np.float32(0))

    def bias(self, y, b):
        return y + b[None, :, None, None]

    def cat0(self, x):
        return np.concatenate([x, np.zeros_like(x[:, :1])], 1)

    def out(self, y):
        return np.asarray(y, np.float32)[0, 0].astype(np.float64)


class _T32:
    name = "torch"

    def __init__(self):
        import torch, fcn_oracle_torch
        self.t, self.o, self.dt = torch, fcn_oracle_torch, torch.float32

    def arr(self, x):
        t = self.t
        return (x if isinstance(x, t.Tensor) else t.from_numpy(np.ascontiguousarray(x))).to(self.dt).contiguous()

    def conv(self, x, w, s=1, p=0, d=1, g=1):
        return self.t.nn.functional.conv2d(x, self.arr(w), None, s, p, d, g)

    def bn(self, x, V, p, idx):
        return self.o._bn(x, {p + s: self.arr(V[p + s][idx]) for s in SUFF}, p)

    def relu6(self, x):
        return self.t.nn.functional.relu6(x)

    def relu(self, x):
        return self.t.nn.functional.relu(x)

    def bias(self, y, b):
        return y + self.arr(b).view(1, -1, 1, 1)

    def cat0(self, x):
        return self.t.cat([x, self.t.zeros_like(x[:, :1])], 1)

    def out(self, y):
        return y[0, 0].numpy().astype(np.float64)


class _T64(_T32):
    name = "f64"

    def __init__(self):
        import torch, fcn_oracle64
        self.t, self.o, self.dt = torch, fcn_oracle64, torch.float64

    def bn(self, x, V, p, idx):
        return self.o._bn(x, {p + s: V[p + s][idx] for s in SUFF}, p)

    def relu6(self, x):
        return self.o._relu6(x)


_ARITH = {}


def arith(name):
    if name not in _ARITH:
        _ARITH[name] = {"numpy": _Np, "torch": _T32, "f64": _T64}[name]()
    return _ARITH[name]


def _names(i):
    from iv_slam_amd.fcn_weights import BLOCKS
    p = "encoder.features.%d.conv" % i
    if BLOCKS[i - 1][2] == 1:
        return None, None, p + ".0", p + ".1", p + ".3", p + ".4"
    return p + ".0", p + ".1", p + ".3", p + ".4", p + ".6", p + ".7"


def run_selector(A, V, entry, x, hidden=None):
    """selector block `entry` = (i, cin, hid, out: channel index lists) on the carried channels x [1][G][h][w], in arithmetic A"""
    from iv_slam_amd.fcn_weights import BLOCKS
    i, cin, hid, out = entry
    _inp, _oup, _t, s, d, _res = BLOCKS[i - 1]
    ex, exbn, dw, dwbn, pj, pjbn = _names(i)
    y = x
    if ex is not None:
        y = A.relu6(A.bn(A.conv(y, V[ex + ".weight"][np.ix_(hid, cin)]), V, exbn, hid))
        if hidden is not None:
            hidden.append(y)
    y = A.relu6(A.bn(A.conv(y, V[dw + ".weight"][hid], s, d, d, len(hid)), V, dwbn, hid))
    if hidden is not None:
        hidden.append(y)
    return A.bn(A.conv(y, V[pj + ".weight"][np.ix_(out, hid)]), V, pjbn, out)


def tail_logits(A, V, plan, x, taps=None):
    """the reader tail and the probe decoder on stage k's carried channels x [1][G][h][w] -> logits [64][64] f64 (values of arithmetic A)"""
    x = A.arr(x)
    hidden = [] if taps is not None else None
    for entry in plan:
        x = run_selector(A, V, entry, x, hidden)
    g = x.shape[1]
    idx = list(range(g)) + [319]
    y = A.conv(A.cat0(x), V["decoder.cbr.0.weight"][:, idx], 1, 1)
    y = A.relu(A.bn(y, V, "decoder.cbr.1", list(range(80))))
    if taps is not None:
        taps["x17"], taps["hidden"], taps["decoder.cbr"] = x, hidden, y
    return A.out(A.bias(A.conv(y, V["decoder.conv_last.weight"]), V["decoder.conv_last.bias"]))


def build_tail(W, k, channels, phase, x64):
    """Weights of the probe network reading `channels` of stage k at `phase`, minus the decoder; x64 [1][G][H][W]: the f64 tap of those channels.
    Returns (V, plan, x17: the carried channels at block 17's output in f64 [1][G][64][64], margin: least distance of a tail hidden value from 0 / 6)."""
    from iv_slam_amd.fcn_weights import BLOCKS
    A = arith("f64")
    V = transparent(W, [r for r in TRANSPARENT_OK if r > k])
    cur, x = list(channels), A.arr(x64)
    g = len(cur)
    oy, ox = phase
    plan, margin = [], 6.0
    for i in SELECTORS:
        if i <= k:
            continue
        inp, oup, t, s, _d, _res = BLOCKS[i - 1]
        ex, exbn, dw, dwbn, pj, pjbn = _names(i)
        hid = list(cur) if t == 1 else list(range(g))
        out = list(range(g))
        assert g <= oup and len(set(cur)) == g
        lo, hi = x.amin((0, 2, 3)).numpy(), x.amax((0, 2, 3)).numpy()
        sc = np.minimum(4.5 / np.maximum(hi - lo, 1e-30), 1024.0).astype(np.float32)
        b = (0.75 - sc.astype(np.float64) * lo).astype(np.float32)
        for name in (ex, dw, pj):
            if name is not None:
                V[name + ".weight"] = np.zeros_like(W[name + ".weight"])
        for name in (exbn, dwbn, pjbn):
            if name is not None:
                n = W[name + ".weight"].shape[0]
                V[name + ".weight"], V[name + ".bias"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
                V[name + ".running_mean"], V[name + ".running_var"] = np.zeros(n, np.float32), np.ones(n, np.float32)
        ty, tx = 1, 1
        if s == 2:
            ty, tx, oy, ox = 1 + (oy & 1), 1 + (ox & 1), oy >> 1, ox >> 1
        for j in range(g):
            if ex is not None:
                V[ex + ".weight"][hid[j], cur[j], 0, 0] = 1.0
            V[dw + ".weight"][hid[j], 0, ty, tx] = 1.0
            V[pj + ".weight"][out[j], hid[j], 0, 0] = np.float32(1.0 / np.float64(sc[j]))
        first, second = (exbn, dwbn) if ex is not None else (dwbn, None)
        V[first + ".weight"][hid], V[first + ".bias"][hid] = sc, b
        if second is not None:
            V[second + ".weight"][hid] = 1.0
        V[pjbn + ".weight"][out] = 1.0
        V[pjbn + ".bias"][out] = (-b.astype(np.float64) / sc.astype(np.float64)).astype(np.float32)
        entry = (i, list(cur), hid, out)
        hidden = []
        x = run_selector(A, V, entry, x, hidden)
        margin = min([margin] + [min(float(h.min()), 6.0 - float(h.max())) for h in hidden])
        plan.append(entry)
        cur = out
    assert (oy, ox) == (0, 0) and tuple(x.shape[2:]) == (64, 64)
    return V, plan, x, margin


class StageContext:
    """One (golden case, stage k): stage k's output in the three precisions (from the case's shared prefix runs) and under the faults."""

    def __init__(self, case, k):
        self.case, self.k, self.tag = case, k, case.tag
        n = stage_name(k)
        self.x64, self.x_np, self.x_torch = case.taps64[n], case.taps_np[n], case.taps_torch[n]
        self.faults = {}
        self._signs = {}

    def sign_faults(self):
        """faults (a) and (b), by which choose_signs picks a group's sign pattern"""
        for name in ("a", "b"):
            if name not in self.faults and not (name == "b" and self.k == 0):
                self.faults[name] = self.case.fault(self.k, name)
        return {n: self.faults[n] for n in ("a", "b") if n in self.faults}

    def choose_signs(self, channels, phase):
        """the candidate pattern under which faults (a) / (b) stand highest over 4 E + q, estimated on stage k's own output (references only)"""
        key = (tuple(channels), phase)
        if key in self._signs:
            return self._signs[key]
        sel = lambda t: at_phase(np.asarray(t)[0, channels], self.k, phase).astype(np.float64)
        x = sel(self.x64)
        en, et = sel(self.x_np) - x, sel(self.x_torch) - x
        blk = np.array([scale_block(j) for j in range(len(channels))])
        q = 2.0 ** -15 * sum((blk == b).sum() * np.abs(x[blk == b]).max(0) for b in set(blk))
        fd = [sel(f) - x for f in self.sign_faults().values()]
        best, best_m = None, -1.0
        for pat in sign_patterns(len(channels)):
            s = np.array(pat)[:, None, None]
            E = max(np.abs((en * s).sum(0)).max(), np.abs((et * s).sum(0)).max())
            m = min(float((np.abs((d * s).sum(0)) / (4 * E + q + 1e-300)).max()) for d in fd)
            if m > best_m:
                best, best_m = pat, m
        self._signs[key] = best
        return best

    def probe(self, channels, phase, index=0):
        return StageProbe(self, channels, phase, index)


class Case:
    """A golden case: weights, image and ONE prefix run in each of the three precisions, shared by all stages."""

    def __init__(self, tag):
        import fcn_oracle, fcn_oracle_torch, fcn_oracle64
        self.tag = tag
        _g, self.W, self.bgr, _out = FC.load_case(tag)
        names = {stage_name(k) for k in range(NSTAGES)}
        _c, _l, self.taps64 = fcn_oracle64.forward(self.W, self.bgr, (64, 64), keep=lambda n: n in names, stop="block14")
        _c, _u, tn = fcn_oracle.forward(self.W, self.bgr, (64, 64), return_taps=True, all_taps=True, last=14)
        self.taps_np = {n: tn[n] for n in names}
        tt = {}
        fcn_oracle_torch.forward(fcn_oracle_torch.prepare(self.W), self.bgr, (64, 64), taps=tt, all_taps=True)
        self.taps_torch = {n: tt[n] for n in names}
        self._ctx = {}

    def stage(self, k):
        if k not in self._ctx:
            self._ctx[k] = StageContext(self, k)
        return self._ctx[k]

    def fault(self, k, name):
        """stage k's f64 output under fault (a): its input cut to f16 toward zero (the stem: its own output; block 1: block1.dw), or (b): block<k>.dw cut"""
        import fcn_oracle64
        if k == 0:
            assert name == "a"
            return trunc_f16(self.taps64["f0"])
        out, dwn = "block%d" % k, "block%d.dw" % k
        prev = stage_name(k - 1)
        if name == "b" or k == 1:
            src, mut = self.taps64[prev], (lambda n, t: trunc_f16(t) if n == dwn else t)
        else:
            src, mut = trunc_f16(self.taps64[prev]), None
        _c, _l, taps = fcn_oracle64.forward(self.W, None, (64, 64), mutate=mut, resume=(prev, src), keep=lambda n: n == out, stop=out)
        return taps[out]


class StageProbe:
    def __init__(self, ctx, channels, phase, index=0):
        self.ctx, self.channels, self.phase = ctx, list(channels), tuple(phase)
        k, g = ctx.k, len(channels)
        self.V, self.plan, x17, self.margin = build_tail(ctx.case.W, k, channels, phase, ctx.x64[:, channels])
        assert self.margin > 0.0, "a ReLU6 of the reader tail clips"
        pat = ctx.choose_signs(self.channels, self.phase)
        t = 1.0 if index % 2 == 0 else -1.0                   # conv_last's sign: odd probes read through negative weights
        x = x17[0].numpy()
        sel, sgn = list(range(g)) + [319] * (80 - g), [t * s for s in pat] + [1.0] * (80 - g)
        cw = np.zeros((80, 320, 3, 3), np.float32)
        for j in range(80):
            cw[j, sel[j], 1, 1] = sgn[j]
        absmax = np.abs(x).max((1, 2))
        beta = np.full(80, 0.25, np.float32)
        beta[:g] = (1.25 * absmax + 0.25).astype(np.float32)
        S = sum(t * (sgn[r] * x[r] + np.float64(beta[r])) for r in range(g))
        lo, hi = float(S.min()), float(S.max())
        self.scale = np.float32(0.18 / max(hi - lo, 1e-30)) if hi > lo else np.float32(1.0)
        self.bias = np.float32(0.5 - float(self.scale) * 0.5 * (hi + lo))
        lw = np.zeros((1, 80, 1, 1), np.float32)
        lw[0, :g, 0, 0] = t * self.scale
        V = self.V
        V["decoder.cbr.0.weight"] = cw
        V["decoder.cbr.1.weight"] = np.ones(80, np.float32); V["decoder.cbr.1.bias"] = beta
        V["decoder.cbr.1.running_mean"] = np.zeros(80, np.float32); V["decoder.cbr.1.running_var"] = np.ones(80, np.float32)
        V["decoder.conv_last.weight"] = lw; V["decoder.conv_last.bias"] = np.array([self.bias], np.float32)
        self.logits64 = self.f64_logits(ctx.x64)
        assert np.abs(self.logits64 - 0.5).max() < 0.1, "probe logits leave 0.5 +- 0.1"
        self.logits_np = tail_logits(arith("numpy"), V, self.plan, np.asarray(ctx.x_np)[:, channels])
        self.logits_torch = tail_logits(arith("torch"), V, self.plan, ctx.x_torch[:, channels])
        self.E = max(float(np.abs(self.logits_np - self.logits64).max()), float(np.abs(self.logits_torch - self.logits64).max()))
        blk = np.array([scale_block(j) for j in range(g)])
        amax = {b: np.abs(x[blk == b]).max(0) for b in set(blk)}                  # the scale block's largest |x| per pixel: the group alone
        self.q = 2.0 ** -15 * float(self.scale) * sum(amax[b] for b in blk)
        self.bar = 4.0 * self.E + self.q                       # [64][64]

    def f64_logits(self, x_stage):
        """the probe's tail and decoder in double on a given stage-k output [1][C][H][W]; no ReLU6 of the tail and not the decoder's ReLU may clip"""
        taps = {}
        logits = tail_logits(arith("f64"), self.V, self.plan, x_stage[:, self.channels], taps)
        assert float(taps["decoder.cbr"].min()) > 0.0, "the probe's ReLU clips"
        for h in taps["hidden"]:
            assert 0.0 < float(h.min()) and float(h.max()) < 6.0, "a ReLU6 of the reader tail clips"
        return logits

    def reads(self, x_stage):
        """does this probe read any value that differs between x_stage and the f64 tap?"""
        d = at_phase((x_stage[0, self.channels] - self.ctx.x64[0, self.channels]).numpy(), self.ctx.k, self.phase)
        return bool(np.any(d != 0.0))

    def worst(self, logits):
        """(largest |logits - f64| / bar over all pixels, largest |logits - f64|)"""
        d = np.abs(np.asarray(logits, np.float64) - self.logits64)
        return float((d / self.bar).max()), float(d.max())


def gpu_groups(k):
    """the device reads what the CPU proof covers: every channel-phase of the stage"""
    return groups(k)


def run_on_device(case, k, nb=20):
    """Every probe of (case, stage k) through ivf_fcn_forward (batch 1: the split schedule) and ivf_fcn_forward_device with `nb` identical images
    (the batched kernels), ivf_fcn_status clean, batch slots bit-identical.  Prints one PROBE line; returns its dictionary."""
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import fcn_weights
    t_all = time.time()
    dev = torch.device("cuda:0")
    ctx = case.stage(k)
    batch = torch.from_numpy(np.stack([case.bgr] * nb)).to(dev)
    cf = torch.empty((nb, 64, 64), dtype=torch.float32, device=dev)
    gl = gpu_groups(k)
    r = {"ratio_single": 0.0, "ratio_batched": 0.0, "dist_single": 0.0, "dist_batched": 0.0, "ratio_refs": 0.0, "create_s": 0.0, "bar_min": 1e9, "bar_max": 0.0}
    for gi, (ch, ph) in enumerate(gl):
        p = ctx.probe(ch, ph, gi)
        t0 = time.time()
        f = iv.IntrospectionFCN(fcn_weights.pack_blob(p.V), case.bgr.shape[:2], (64, 64), max_batch=nb)
        r["create_s"] += time.time() - t0
        _u8, cost = f(case.bgr, want_f32=True)
        f.forward_device(batch, cost_f32=cf); f.status()
        cb = cf.cpu().numpy()
        assert all(np.array_equal(cb[i], cb[0]) for i in range(1, nb)), "batch slots differ (same input)"
        for key, c in (("single", cost), ("batched", cb[0])):
            ratio, dist = p.worst(logits_from_cost(c))
            r["ratio_" + key] = max(r["ratio_" + key], ratio); r["dist_" + key] = max(r["dist_" + key], dist)
            if not ratio <= 1.0:
                print("OVER %s %d group %d channels %d..%d phase %d,%d %s: %.3g = %.2f x bar" % (case.tag, k, gi, ch[0], ch[-1], ph[0], ph[1], key, dist, ratio), flush=True)
        r["ratio_refs"] = max(r["ratio_refs"], p.worst(p.logits_np)[0], p.worst(p.logits_torch)[0])
        r["bar_min"] = min(r["bar_min"], float(p.bar.min())); r["bar_max"] = max(r["bar_max"], float(p.bar.max()))
        del f
    r = {"case": case.tag, "stage": k, "probes": len(gl), "group": GROUP[k], **r, "seconds": time.time() - t_all}
    print("PROBE " + json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    # one device step of tests/test_gpu_fcn_stage_probe.py: python tests/fcn_stage_probe.py <case> <stage> [<stage> ...]
    sys.path.insert(0, FC.ROOT)
    t0 = time.time()
    case = Case(sys.argv[1])
    print("PREFIX %s %.2f s" % (sys.argv[1], time.time() - t0), flush=True)
    res = [run_on_device(case, int(a)) for a in sys.argv[2:]]
    worst = max(max(r["ratio_single"], r["ratio_batched"]) for r in res)
    print("WORST %.4f" % worst)
    sys.exit(0 if worst <= 1.0 else 1)
