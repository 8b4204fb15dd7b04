"""Probe networks for FCN blocks 15-17: ordinary weight dictionaries (pack_blob) that make single channels of block 17's output readable
in the cost map, so that the kernels of those blocks are compared per channel with the f64 reference (oracle/fcn_oracle64.py).

A probe is a golden case's network with ONLY the decoder replaced (and, per configuration, residual blocks made transparent):
  * decoder.cbr.0 is a centre-tap selector: row j holds one +-1 at [j, c_j, 1, 1]; decoder.cbr.1 is gamma 1, mean 0, var 1 and a beta above the
    channel's largest |x| (f64 reference), so the ReLU never clips: decoder channel j = +-x[c_j] + beta_j;
  * conv_last is non-zero on the GROUP decoder rows of one group of GROUP block-17 channels, scaled and biased (from the f64 reference) so that
    every logit lies in 0.5 +- 0.1: the sigmoid never saturates and  logit = 0.5 + ln(c / (1 - c)) / 20  recovers it from the f32 cost map;
  * the handle is created with out_size = (64, 64): the output interpolation is the identity (src = x, l1 = 0).
Groups are 4 consecutive channels: 80 groups cover the 320 channels, and none straddles a scale block of the decoder's fp6 correction product
(k_fcn_conv3x3_f6 / _f6r take one power-of-two scale per pixel from the 16 channels {32 a + 8 b + j, 32 a + 16 + 8 b + j : j < 8}).
The sign pattern of a group is the one of the eight with the best fault resolution (choose_signs: references only).

Transparent residual block r: the projection BatchNorm's gamma and beta zeroed -> the branch is exactly 0, the block an exact pass-through
whose kernels still run.  CONFIGS: block 17 fed by the ordinary encoder / with 16 transparent / with 15 and 16 transparent -- a fault then
localises to k_fcn_irbd4<res> or to the 320-channel kernel.

The bar (ISSUE: defined from the references, never from the code under test), per probe and pixel:
    bar = 4 max(|logits_numpy_f32 - logits_f64|, |logits_torch_f32 - logits_f64|) + q
4 = 22-bit operands against f32's 24; the max runs over both restatements and all pixels.  q is the decoder's read-out quantum: x_lo 2^10 <= amax / 2
is rounded to e2m3 at a scale with amax / 2^sb in [4, 8), i.e. to steps of 2^sb / 4 <= amax / 16: at most amax 2^-15 per channel, amax the scale
block's largest |x| AT THAT PIXEL (f64 tap);  q = 2^-15 |conv_last scale| sum over the group of it.  q = 0 for the three-f16 decoder (IVF_FCN_DEC6=0).
"""
import itertools
import json
import os
import sys
import time

import numpy as np

import fcn_common as FC

GROUP = 4
NGROUPS = 320 // GROUP
CONFIGS = {"plain": (), "t16": (16,), "t15_16": (15, 16)}
TRANSPARENT_OK = (3, 5, 6, 8, 9, 10, 12, 13, 15, 16)
PATTERNS = [(1.0,) + p for p in itertools.product((1.0, -1.0), repeat=GROUP - 1)]


def scale_block(c):
    """index of the fp6 scale block (16 channels) of block-17 channel c"""
    return (c // 32) * 2 + (c % 16) // 8


def group_channels(gi):
    ch = list(range(GROUP * gi, GROUP * gi + GROUP))
    assert len({scale_block(c) for c in ch}) == 1
    return ch


def transparent(W, blocks):
    V = dict(W)
    for r in blocks:
        assert r in TRANSPARENT_OK, r
        for s in (".weight", ".bias"):
            k = "encoder.features.%d.conv.7%s" % (r, s)
            V[k] = np.zeros_like(W[k])
    return V


def trunc_f16(x):
    """f16 significand (11 bits), rounded toward zero, no lo half: what a lost split-f16 correction product leaves of an operand"""
    import torch
    m, e = torch.frexp(x)
    return torch.ldexp(torch.trunc(m * 2048.0) / 2048.0, e)


def logits_from_cost(cost_f32):
    c = np.asarray(cost_f32, np.float64)
    return 0.5 + np.log(c / (1.0 - c)) / 20.0


class Context:
    """One (golden case, configuration): the shared encoder run once through the three references, block 17's output under faults (a) and (b)."""

    def __init__(self, tag, config):
        import torch
        import fcn_oracle, fcn_oracle_torch, fcn_oracle64
        self.tag, self.config = tag, config
        g, W, bgr, _out = FC.load_case(tag)
        self.bgr = bgr
        self.W = transparent(W, CONFIGS[config])
        keep = lambda n: n in ("block14", "block17")
        _c, _l, taps = fcn_oracle64.forward(self.W, bgr, (64, 64), keep=keep)
        self.x14, self.x17 = taps["block14"], taps["block17"]
        _c, _u, tn = fcn_oracle.forward(self.W, bgr, (64, 64), return_taps=True)
        self.x17_np = tn["block17"]
        tt = {}
        fcn_oracle_torch.forward(fcn_oracle_torch.prepare(self.W), bgr, (64, 64), taps=tt)
        self.x17_torch = tt["block17"]
        x = self.x17[0].numpy()
        self.absmax = np.abs(x).max((1, 2))
        blk = np.array([scale_block(c) for c in range(320)])
        self.block_amax = np.stack([np.abs(x[blk == b]).max(0) for b in range(20)])          # [20][64][64]
        self.faulted = {"a": self.fault_x17(lambda n, t: trunc_f16(t) if n == "block16" else t)}
        if 15 not in CONFIGS[config]:         # a transparent block 15 discards its depthwise output: no probe reads fault (b)
            self.faulted["b"] = self.fault_x17(lambda n, t: trunc_f16(t) if n == "block15.dw" else t)
        self._signs = {}

    def fault_x17(self, mutate):
        """block 17's output with `mutate` injected downstream of block 14"""
        import fcn_oracle64
        _c, _l, taps = fcn_oracle64.forward(self.W, self.bgr, (64, 64), mutate=mutate, resume=("block14", self.x14), keep=lambda n: n == "block17")
        return taps["block17"]

    def choose_signs(self, gi):
        """the sign pattern (first sign +) under which faults (a) / (b) stand highest over 4 E + q, estimated on block 17's output"""
        if gi in self._signs:
            return self._signs[gi]
        ch = group_channels(gi)
        x = self.x17[0, ch].numpy()
        en, et = self.x17_np[0, ch] - x, self.x17_torch[0, ch].numpy() - x
        q = 2.0 ** -15 * GROUP * self.block_amax[scale_block(ch[0])]
        best, best_m = None, -1.0
        for pat in PATTERNS:
            s = np.array(pat)[:, None, None]
            E = max(np.abs((en * s).sum(0)).max(), np.abs((et * s).sum(0)).max())
            m = min(float((np.abs(((f[0, ch].numpy() - x) * s).sum(0)) / (4 * E + q)).max()) for f in self.faulted.values())
            if m > best_m:
                best, best_m = pat, m
        self._signs[gi] = best
        return best

    def probe(self, gi, dec6=True):
        return Probe(self, gi, dec6)


class Probe:
    def __init__(self, ctx, gi, dec6=True):
        import fcn_oracle, fcn_oracle_torch
        self.ctx, self.gi = ctx, gi
        ch = group_channels(gi)
        self.channels = ch
        pat = ctx.choose_signs(gi)
        t = 1.0 if gi % 2 == 0 else -1.0                      # conv_last's sign: odd groups read through negative weights
        rows = [(GROUP * gi + k) % 80 for k in range(GROUP)]
        sel = [(GROUP * j) % 320 for j in range(80)]          # rows outside the group: a selector too, conv_last zero
        sgn = [1.0] * 80
        for k, r in enumerate(rows):
            sel[r], sgn[r] = ch[k], t * pat[k]
        cw = np.zeros((80, 320, 3, 3), np.float32)
        for j in range(80):
            cw[j, sel[j], 1, 1] = sgn[j]
        beta = (1.25 * ctx.absmax[sel] + 0.25).astype(np.float32)
        x = ctx.x17[0].numpy()
        S = sum(t * (sgn[r] * x[sel[r]] + np.float64(beta[r])) for r in rows)
        lo, hi = float(S.min()), float(S.max())
        self.scale = np.float32(0.18 / (hi - lo))
        self.bias = np.float32(0.5 - float(self.scale) * 0.5 * (hi + lo))
        lw = np.zeros((1, 80, 1, 1), np.float32)
        for r in rows:
            lw[0, r, 0, 0] = t * self.scale
        V = dict(ctx.W)
        V["decoder.cbr.0.weight"] = cw
        V["decoder.cbr.1.weight"] = np.ones(80, np.float32); V["decoder.cbr.1.bias"] = beta
        V["decoder.cbr.1.running_mean"] = np.zeros(80, np.float32); V["decoder.cbr.1.running_var"] = np.ones(80, np.float32)
        V["decoder.conv_last.weight"] = lw; V["decoder.conv_last.bias"] = np.array([self.bias], np.float32)
        self.W = V
        self.logits64 = self.f64_logits(ctx.x17)
        assert np.abs(self.logits64 - 0.5).max() < 0.1, "probe logits leave 0.5 +- 0.1"
        _c, _u, tn = fcn_oracle.forward(V, None, (64, 64), return_taps=True, resume=(17, ctx.x17_np))
        tt = {}
        fcn_oracle_torch.forward(fcn_oracle_torch.prepare(V), None, (64, 64), taps=tt, resume=(17, ctx.x17_torch))
        self.logits_np = tn["logits"][0, 0].astype(np.float64)
        self.logits_torch = tt["logits"][0, 0].numpy().astype(np.float64)
        self.E = max(float(np.abs(self.logits_np - self.logits64).max()), float(np.abs(self.logits_torch - self.logits64).max()))
        self.q = (2.0 ** -15 * float(self.scale) * GROUP * ctx.block_amax[scale_block(ch[0])]) if dec6 else np.zeros((64, 64))
        self.bar = 4.0 * self.E + self.q                       # [64][64]

    def f64_logits(self, x17):
        """the probe's decoder in double on a given block-17 output, with the ReLU checked never to clip"""
        import fcn_oracle64
        _c, logits, taps = fcn_oracle64.forward(self.W, None, (64, 64), resume=("block17", x17), keep=lambda n: n == "decoder.cbr")
        assert float(taps["decoder.cbr"].min()) > 0.0, "the probe's ReLU clips"
        return logits

    def worst(self, logits):
        """(largest |logits - f64| / bar over all pixels, largest |logits - f64|)"""
        d = np.abs(np.asarray(logits, np.float64) - self.logits64)
        return float((d / self.bar).max()), float(d.max())


def run_on_device(tag, dec6=True, configs=tuple(CONFIGS), nb=20):
    """Every probe of a golden case through ivf_fcn_forward (batch 1: the split schedule) and ivf_fcn_forward_device with `nb` images (the
    batched kernels).  Returns per configuration the worst |logit - f64| / bar, the worst distance and the handle creation time."""
    import torch
    import iv_slam_amd as iv
    from iv_slam_amd import fcn_weights
    dev = torch.device("cuda:0")
    out = {}
    for config in configs:
        ctx = Context(tag, config)
        batch = torch.from_numpy(np.stack([ctx.bgr] * nb)).to(dev)
        cf = torch.empty((nb, 64, 64), dtype=torch.float32, device=dev)
        r = {"ratio_single": 0.0, "ratio_batched": 0.0, "dist_single": 0.0, "dist_batched": 0.0, "ratio_refs": 0.0, "create_s": 0.0, "bar_min": 1e9, "bar_max": 0.0}
        for gi in range(NGROUPS):
            p = ctx.probe(gi, dec6)
            t0 = time.time()
            f = iv.IntrospectionFCN(fcn_weights.pack_blob(p.W), ctx.bgr.shape[:2], (64, 64), max_batch=nb)
            r["create_s"] += time.time() - t0
            _u8, cost = f(ctx.bgr, want_f32=True)
            f.forward_device(batch, cost_f32=cf); f.status()
            cb = cf.cpu().numpy()
            assert all(np.array_equal(cb[i], cb[0]) for i in range(1, nb)), "batch slots differ (same input)"
            for key, c in (("single", cost), ("batched", cb[0])):
                ratio, dist = p.worst(logits_from_cost(c))
                r["ratio_" + key] = max(r["ratio_" + key], ratio); r["dist_" + key] = max(r["dist_" + key], dist)
                if ratio > 1.0:
                    print("OVER %s %s group %d (channels %d..%d) %s: %.3g = %.2f x bar" % (tag, config, gi, p.channels[0], p.channels[-1], key, dist, ratio), flush=True)
            r["ratio_refs"] = max(r["ratio_refs"], p.worst(p.logits_np)[0], p.worst(p.logits_torch)[0])
            r["bar_min"] = min(r["bar_min"], float(p.bar.min())); r["bar_max"] = max(r["bar_max"], float(p.bar.max()))
            del f
        out[config] = r
        print("PROBE " + json.dumps({"case": tag, "config": config, "dec6": bool(dec6), **r}), flush=True)
    return out


if __name__ == "__main__":
    # one device step of tests/test_gpu_fcn_probe.py: python tests/fcn_probe.py <case> <dec6: 0 | 1> [config ...]
    sys.path.insert(0, FC.ROOT)
    res = run_on_device(sys.argv[1], sys.argv[2] == "1", tuple(sys.argv[3:]) or tuple(CONFIGS))
    worst = max(max(r["ratio_single"], r["ratio_batched"]) for r in res.values())
    print("WORST %.4f" % worst)
    sys.exit(0 if worst <= 1.0 else 1)
