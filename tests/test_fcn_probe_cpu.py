"""CPU: the f64 FCN reference (oracle/fcn_oracle64.py) against the goldens and the f32 restatements, and the proof that the probe networks of
tests/fcn_probe.py resolve what the end-to-end 3e-4 bar cannot: the f32 restatements stay inside every probe's bar, injected faults of blocks
15-17 cross it by a factor >= 2.  No GPU."""
import numpy as np
import pytest

import fcn_common as FC
import fcn_probe as P

CASES = ["kitti", "jackal", "jackal_full", "kitti_smallw", "jackal_smallw", "kitti_bigw"]


@pytest.mark.parametrize("tag", CASES)
def test_f64_reference_matches_goldens_and_the_f32_restatements(tag):
    """The f32-vs-f64 distances printed here are the noise floor of every FCN bar in the suite ("f64 reference").
    Bound 2e-4 on the full cost map: the bound the two f32 restatements already keep against each other and the goldens (test_fcn_oracle.py)."""
    import fcn_oracle, fcn_oracle_torch, fcn_oracle64
    g, W, bgr, out_size = FC.load_case(tag)
    seen = []
    cost, logits, taps = fcn_oracle64.forward(W, bgr, out_size, mutate=lambda n, t: (seen.append(n), t)[1], keep=lambda n: n in ("block17", "decoder.cbr"))
    assert cost.dtype == np.float64 and logits.shape == (64, 64) and cost.shape == tuple(out_size)
    want = ["f0", "block1.dw", "block1"] + [n for i in range(2, 18) for n in ("block%d.expand" % i, "block%d.dw" % i, "block%d" % i)] + ["decoder.cbr", "logits"]
    assert seen == want
    FC.check_against_golden(g, cost.astype(np.float32), fcn_oracle64.cost_u8(cost), tol=2e-4)
    assert np.abs(logits - g["logits"]).max() < 5e-5
    assert np.abs(taps["block17"][0, ::16, ::8, ::8].numpy() - g["f17_sub"]).max() < 5e-4
    cn, _u, tn = fcn_oracle.forward(W, bgr, out_size, return_taps=True)
    tt = {}
    ct, _u = fcn_oracle_torch.forward(fcn_oracle_torch.prepare(W), bgr, out_size, taps=tt)
    d = {"cost_numpy": np.abs(cn - cost).max(), "cost_torch": np.abs(ct - cost).max(),
         "logits_numpy": np.abs(tn["logits"][0, 0] - logits).max(), "logits_torch": np.abs(tt["logits"][0, 0].numpy() - logits).max()}
    print("f32 vs f64, %s: " % tag + ", ".join("%s %.3g" % kv for kv in d.items()))
    assert max(d["cost_numpy"], d["cost_torch"]) < 2e-4 and max(d["logits_numpy"], d["logits_torch"]) < 5e-5


def test_mutate_and_resume_of_the_f64_reference():
    import fcn_oracle64
    g, W, bgr, out_size = FC.load_case("kitti")
    c0, l0, taps = fcn_oracle64.forward(W, bgr, out_size, keep=lambda n: n in ("block14", "block15.dw"))
    c1, l1, _t = fcn_oracle64.forward(W, bgr, out_size, resume=("block14", taps["block14"]), keep=lambda n: False)
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1)
    c2, l2, t2 = fcn_oracle64.forward(W, bgr, out_size, resume=("block14", taps["block14"]), mutate=lambda n, t: t * (1 + 1e-4) if n == "block15.dw" else t,
                                      keep=lambda n: n == "block15.dw")
    assert np.array_equal(t2["block15.dw"].numpy(), (taps["block15.dw"] * (1 + 1e-4)).numpy()) and 1e-6 < np.abs(l2 - l0).max() < 1e-2


def test_probe_groups_cover_all_channels_inside_scale_blocks():
    seen = sorted(c for gi in range(P.NGROUPS) for c in P.group_channels(gi))
    assert seen == list(range(320))
    # the scale blocks as k_fcn_conv3x3_f6 forms them: lane (pixel, kg) of K-step pair s2 holds channels 32 s2 + 16 st + 8 kg + j
    for s2 in range(10):
        for kg in range(2):
            assert {P.scale_block(32 * s2 + 16 * st + 8 * kg + j) for st in range(2) for j in range(8)} == {2 * s2 + kg}


@pytest.mark.parametrize("config", list(P.CONFIGS))
@pytest.mark.parametrize("tag", ["kitti", "jackal_smallw"])
def test_references_stay_inside_the_bar_and_faults_cross_it(tag, config):
    """Every pixel of every probe's 64 x 64 map.  Faults through the f64 reference's mutate hook:
      (a) block 17's input cut to an f16 toward zero (a lost correction product of its expansion);   (b) the same on block 15's depthwise output;
      (c) one channel of block 17's output zeroed in its last column;                                   (d) one corner pixel of one channel off by 2^-10 relative.
    Each must stand >= 2 x the bar above the f64 logits on every probe that reads the affected channel; the bar includes the product decoder's fp6 quantum."""
    ctx = P.Context(tag, config)
    if config != "plain":          # a transparent block is an exact pass-through
        import fcn_oracle64
        g, W, bgr, _o = FC.load_case(tag)
        _c, _l, taps = fcn_oracle64.forward(ctx.W, bgr, (64, 64), keep=lambda n: n in ("block14", "block15", "block16"))
        src = "block15" if config == "t16" else "block14"
        assert np.array_equal(taps["block16"].numpy(), taps[src].numpy())
    x = ctx.x17[0].numpy()
    # (c): a channel of the first and of the last group; (d): the channel / corner with the largest |x| of all corners (chosen on the f64 reference)
    corners = [(0, 0), (0, 63), (63, 0), (63, 63)]
    cd, (yd, xd) = max(((c, yx) for c in range(320) for yx in corners), key=lambda a: abs(x[a[0], a[1][0], a[1][1]]))

    def zero_last_column(c):
        def m(n, t):
            if n == "block17":
                t = t.clone(); t[0, c, :, 63] = 0.0
            return t
        return m

    def corner(n, t):
        if n == "block17":
            t = t.clone(); t[0, cd, yd, xd] *= 1.0 + 2.0 ** -10
        return t

    single = {"c%d" % c: (c, ctx.fault_x17(zero_last_column(c))) for c in (1, 318)}
    single["d"] = (cd, ctx.fault_x17(corner))
    inside, margins = 0.0, {}
    for gi in range(P.NGROUPS):
        p = ctx.probe(gi)
        inside = max(inside, p.worst(p.logits_np)[0], p.worst(p.logits_torch)[0])
        for name, xf in ctx.faulted.items():
            margins.setdefault(name, []).append(p.worst(p.f64_logits(xf))[0])
        for name, (c, xf) in single.items():
            if c in p.channels:
                margins.setdefault(name, []).append(p.worst(p.f64_logits(xf))[0])
    print("%s %s: f32 restatements at most %.3f x bar; faults / bar (least over the probes that read them): " % (tag, config, inside) +
          ", ".join("(%s) %.2f" % (k, min(v)) for k, v in sorted(margins.items())))
    assert inside <= 0.25 + 1e-9          # 4 E is part of the bar
    assert set(margins) == ({"a", "b", "c1", "c318", "d"} if "b" in ctx.faulted else {"a", "c1", "c318", "d"})
    assert len(margins["a"]) == P.NGROUPS and all(len(margins[k]) == 1 for k in margins if k[0] in "cd")
    for k, v in margins.items():
        assert min(v) >= 2.0, "fault (%s) stands only %.2f x the bar above the reference on some probe" % (k, min(v))
