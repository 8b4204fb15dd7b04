"""CPU: the proof that the stage probes of tests/fcn_stage_probe.py (stem and blocks 1-14 read through a reader tail) resolve what the end-to-end
3e-4 bar cannot.  Per (case, stage), every pixel of every probe: the two f32 restatements stay at <= 0.25 of the bar, every injected fault stands
>= 2 x the bar above the f64 logits on every probe that reads it (both figures are DESIGN 7.t's).  Margins per stage: DESIGN 7.t.  No GPU."""
import numpy as np
import pytest

import fcn_common as FC
import fcn_stage_probe as SP

CASES = ["kitti", "jackal_smallw"]
# faults that a stage cannot show at 2 x the bar with any group size down to 1 (figures in DESIGN 7.t): {(stage): (fault names)}
LEFT_OUT = {}
_CASES = {}


def case_of(tag):
    if tag not in _CASES:
        _CASES[tag] = SP.Case(tag)
    return _CASES[tag]


def seam_candidates(k):
    """the four pixels around the tile corner nearest the image centre of the kernel that writes stage k (blocks 8-14: the rows either side of the
    strip boundary between sub-image rows 15 and 16, i.e. image rows 30 .. 33)"""
    side = 64 * SP.stage_stride(k)
    if k in SP.TILE:
        tw, th = SP.TILE[k]
        xs, ys = tw * round(side / 2 / tw), th * round(side / 2 / th)
        return [(y, x) for y in (ys - 1, ys) for x in (xs - 1, xs)]
    return [(y, x) for y in (30, 31, 32, 33) for x in (30, 31, 32, 33)]


def stage_faults(case, k):
    """{name: stage k's f64 output under the fault}: (a), (b) (fcn_stage_probe.Case.fault); (c) channel 1 zeroed in its last column and channel C - 2
    in its last row (a channel of the first and of the last group); (d) one pixel of one channel off by 2^-10 relative at an image corner and at a tile
    seam, the (channel, pixel) with the largest |x| among the candidates on the f64 tap."""
    ctx = case.stage(k)
    x = ctx.x64
    c, side = x.shape[1], x.shape[2]
    f = dict(ctx.sign_faults())
    t = x.clone(); t[0, 1, :, side - 1] = 0.0; f["c_col"] = t
    t = x.clone(); t[0, c - 2, side - 1, :] = 0.0; f["c_row"] = t
    corners = [(0, 0), (0, side - 1), (side - 1, 0), (side - 1, side - 1)]
    for name, cand in (("d_corner", corners), ("d_seam", seam_candidates(k))):
        cd, (yd, xd) = max(((ch, yx) for ch in range(c) for yx in cand), key=lambda a: abs(float(x[0, a[0], a[1][0], a[1][1]])))
        t = x.clone(); t[0, cd, yd, xd] *= 1.0 + 2.0 ** -10
        f[name] = t
    return f


def measure(case, k, group=None, phase_list=None):
    ctx = case.stage(k)
    faults = stage_faults(case, k)
    inside, margins, bars, tail_margin = 0.0, {}, [], 6.0
    gl = SP.groups(k, group, phase_list)
    for gi, (ch, ph) in enumerate(gl):
        p = ctx.probe(ch, ph, gi)
        inside = max(inside, p.worst(p.logits_np)[0], p.worst(p.logits_torch)[0])
        bars += [float(p.bar.min()), float(p.bar.max())]
        tail_margin = min(tail_margin, p.margin)
        for name, xf in faults.items():
            if p.reads(xf):
                margins.setdefault(name, []).append(p.worst(p.f64_logits(xf))[0])
    return inside, margins, (min(bars), max(bars)), tail_margin, len(gl)


def test_groups_cover_every_channel_phase_exactly_once():
    want = {0: 512, 1: 256, 2: 96, 3: 96, 4: 32, 5: 32, 6: 32, 7: 64, 8: 64, 9: 64, 10: 64, 11: 96, 12: 96, 13: 96, 14: 160}
    for k in range(SP.NSTAGES):
        seen = [(c, ph) for ch, ph in SP.groups(k) for c in ch]
        assert len(seen) == len(set(seen)) == want[k]
        assert set(seen) == {(c, ph) for c in range(SP.stage_channels(k)) for ph in SP.phases(k)}
        assert SP.gpu_groups(k) == SP.groups(k)          # the GPU module reads all of them
    # the phase arithmetic: a probe of phase (oy, ox) reads stage pixel (n i + oy, n j + ox)
    a = np.arange(256 * 256).reshape(256, 256)
    assert SP.at_phase(a, 0, (3, 1))[5, 7] == a[4 * 5 + 3, 4 * 7 + 1] and SP.at_phase(a[:128, :128], 2, (1, 0))[5, 7] == a[2 * 5 + 1, 2 * 7]


@pytest.mark.parametrize("k", range(SP.NSTAGES))
@pytest.mark.parametrize("tag", CASES)
def test_references_stay_inside_the_bar_and_faults_cross_it(tag, k):
    """Faults through the f64 reference (stage_faults): (a) stage k's input cut to f16 toward zero (the stem: its own output; block 1: block1.dw),
    (b) block<k>.dw cut the same way, (c) a channel zeroed in its last column / another in its last row, (d) one pixel off by 2^-10 relative at an image
    corner / at a tile seam.  Also: the sliced tail equals the f32 oracles on the whole probe network bit for bit (f64: to 1e-14), the transparent blocks are exact
    pass-throughs, no ReLU6 of the tail clips (asserted in StageProbe for the f64 tap and every fault)."""
    import fcn_oracle, fcn_oracle_torch, fcn_oracle64
    case = case_of(tag)
    ctx = case.stage(k)
    # one probe through the oracles proper, whole network: the reader tail reads pixel (n i + oy, n j + ox) of its channels and nothing else
    ch, ph = SP.groups(k)[-1]
    p = ctx.probe(ch, ph, 1)
    name = SP.stage_name(k)
    blocks = ["block%d" % i for i in range(max(k, 1), 18)]
    _c, l64, taps = fcn_oracle64.forward(p.V, None, (64, 64), resume=(name, ctx.x64), keep=lambda n: n in blocks)
    assert np.abs(l64 - p.logits64).max() < 1e-14          # conv_last's bias is added in another order: f64's own rounding
    for r in SP.TRANSPARENT_OK:
        if r > k:
            assert np.array_equal(taps["block%d" % r].numpy(), (ctx.x64 if r - 1 == k else taps["block%d" % (r - 1)]).numpy()), r
    x17 = taps["block17"][0].numpy()
    assert not x17[len(ch):].any()
    # block 17's carried channels are stage k's at the phase, up to the tail's 21 BatchNorm factors 1 / sqrt(1 + 1e-5) and f32 weights
    want = SP.at_phase(ctx.x64[0, ch].numpy(), k, ph)
    assert np.abs(x17[:len(ch)] - want).max() <= 2e-3 * max(1.0, np.abs(want).max())
    _c, _u, tn = fcn_oracle.forward(p.V, None, (64, 64), return_taps=True, resume=(k, ctx.x_np))
    assert np.array_equal(tn["logits"][0, 0].astype(np.float64), p.logits_np)
    tt = {}
    fcn_oracle_torch.forward(fcn_oracle_torch.prepare(p.V), None, (64, 64), taps=tt, resume=(k, ctx.x_torch))
    assert np.array_equal(tt["logits"][0, 0].numpy().astype(np.float64), p.logits_torch)

    inside, margins, bars, tail_margin, n = measure(case, k)
    print("STAGE %s %d: %d probes of %d, bar %.3g .. %.3g, f32 restatements at most %.3f x bar, tail ReLU6 margin %.3g; least fault / bar: " %
          (tag, k, n, SP.GROUP[k], bars[0], bars[1], inside, tail_margin) + ", ".join("(%s) %.2f" % (kk, min(v)) for kk, v in sorted(margins.items())))
    assert inside <= 0.25 + 1e-9 and tail_margin > 0.0
    want = {"a", "c_col", "c_row", "d_corner", "d_seam"} | ({"b"} if k > 0 else set())
    assert set(margins) == want
    assert len(margins["a"]) == n and all(len(margins[kk]) >= 1 for kk in margins)
    for kk, v in margins.items():
        if kk not in LEFT_OUT.get(k, ()):
            assert min(v) >= 2.0, "fault (%s) stands only %.2f x the bar above the reference on some probe" % (kk, min(v))


def test_a_wrong_library_fails_the_right_stage():
    """A cost map as a library with fault (a) in block 6 would return it (f64 logits -> f32 cost) fails Probe.worst at stage 6 and passes at stage 5."""
    case = case_of("kitti")
    bad = case.fault(6, "a")
    for k, x in ((5, case.taps64["block5"]), (6, bad)):
        ch, ph = SP.groups(k)[0]
        p = case.stage(k).probe(ch, ph, 0)
        z = p.f64_logits(x)
        cost = (1.0 / (1.0 + np.exp(-20.0 * (z - 0.5)))).astype(np.float32)
        ratio = p.worst(SP.logits_from_cost(cost))[0]
        assert (ratio > 1.0) if k == 6 else (ratio <= 1.0), (k, ratio)
