"""fcn_oracle64.py -- the introspection FCN's layer list in IEEE double (TEST INFRASTRUCTURE ONLY).

The graph of oracle/fcn_oracle.py (preprocess, bilinear to 512 x 512, stem, 17 inverted-residual blocks, C1 decoder, bilinear to
the out size, sigmoid(20 (x - 0.5))), every operation in torch.float64 on host cores.  It is the yardstick the f32 restatements
(fcn_oracle.py, fcn_oracle_torch.py) and the device are measured against: its own rounding error (~1e-15 relative per operation)
is nine orders below anything the FCN tests resolve.

    cost, logits, taps = forward(W, bgr_u8, out_size)

  cost    [H][W] f64 at the out size
  logits  [64][64] f64: conv_last's output, before the final interpolation
  taps    {name: f64 tensor [1][C][h][w]}: "f0" (stem), "block<i>" (block output, after the residual add), "block<i>.expand" and
          "block<i>.dw" (after BatchNorm + ReLU6; block 1 has no expansion), "decoder.cbr", "logits"

  mutate(name, tensor) -> tensor   is applied at every tap, in graph order, and the graph continues from what it returns: the
                                   fault-injection hook of tests/test_fcn_probe_cpu.py
  resume = (name, tensor)          start from a recorded "block<i>" or "f0" tap instead of the image (the probe networks of tests/fcn_probe.py
                                   share their encoder: only the tail is recomputed).  mutate is NOT re-applied to the resumed tap.
  keep(name) -> bool               which taps to return (all by default; the early expansions are 50 MB each)
  stop = name                      return (None, None, taps) right after that tap instead of running on to the cost map
"""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
MAX_THREADS = 16
D = torch.float64


class _Stop(Exception):
    pass


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _bn(x, W, p, eps=1e-5):
    g, b, m, v = (_t(W[p + s]) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    inv = g / torch.sqrt(v + eps)
    return (x - m.view(1, -1, 1, 1)) * inv.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def _relu6(x):
    return torch.clamp(x, 0.0, 6.0)


def preprocess(bgr_u8):
    x = _t(np.asarray(bgr_u8)[:, :, ::-1]).permute(2, 0, 1)[None] / 255.0
    return (x - torch.tensor(MEAN, dtype=D).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=D).view(1, 3, 1, 1)


@torch.no_grad()
def forward(W, bgr_u8, out_size, enc_size=(512, 512), mutate=None, resume=None, keep=None, stop=None):
    from iv_slam_amd.fcn_weights import BLOCKS          # architecture table (data)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(nthreads, MAX_THREADS))
    try:
        taps = {}

        def tap(name, x):
            if mutate is not None:
                x = mutate(name, x)
            if keep is None or keep(name):
                taps[name] = x
            if name == stop:
                raise _Stop
            return x

        first = 1
        if resume is None:
            x = F.interpolate(preprocess(bgr_u8), size=tuple(enc_size), mode="bilinear", align_corners=False)
            x = _relu6(_bn(F.conv2d(x, _t(W["encoder.features.0.0.weight"]), None, 2, 1), W, "encoder.features.0.1"))
            x = tap("f0", x)
        else:
            name, x = resume
            assert name == "f0" or (name.startswith("block") and "." not in name), name
            first = 1 if name == "f0" else int(name[5:]) + 1
            x = x.to(D)
        for i, (inp, oup, t, s, d, res) in enumerate(BLOCKS, start=1):
            if i < first:
                continue
            p = "encoder.features.%d.conv" % i
            y = x
            if t == 1:
                y = tap("block%d.dw" % i, _relu6(_bn(F.conv2d(y, _t(W[p + ".0.weight"]), None, s, d, d, inp * t), W, p + ".1")))
                y = _bn(F.conv2d(y, _t(W[p + ".3.weight"])), W, p + ".4")
            else:
                y = tap("block%d.expand" % i, _relu6(_bn(F.conv2d(y, _t(W[p + ".0.weight"])), W, p + ".1")))
                y = tap("block%d.dw" % i, _relu6(_bn(F.conv2d(y, _t(W[p + ".3.weight"]), None, s, d, d, inp * t), W, p + ".4")))
                y = _bn(F.conv2d(y, _t(W[p + ".6.weight"])), W, p + ".7")
            x = tap("block%d" % i, x + y if res else y)
        y = tap("decoder.cbr", F.relu(_bn(F.conv2d(x, _t(W["decoder.cbr.0.weight"]), None, 1, 1), W, "decoder.cbr.1")))
        y = F.conv2d(y, _t(W["decoder.conv_last.weight"]), _t(W["decoder.conv_last.bias"]))
        y = tap("logits", y)
        logits = y[0, 0].numpy().copy()
        y = F.interpolate(y, size=tuple(out_size), mode="bilinear", align_corners=False)
        cost = torch.sigmoid(20.0 * (y - 0.5))[0, 0].numpy().copy()
        return cost, logits, taps
    except _Stop:
        return None, None, taps
    finally:
        torch.set_num_threads(nthreads)


def cost_u8(cost):
    """(cost * 255.0).to(uint8) of the call contract: truncation"""
    return np.floor(np.asarray(cost, np.float64) * 255.0).astype(np.uint8)
