"""tools/export_fcn_weights.py on the artefact formats the reference ships / produces: a TorchScript archive traced and saved the way
IF/training/export_model_light.py:114-121 does (what stereo_kitti.cc:236 `torch::jit::load`s), a whole-module state_dict, and
separate encoder / decoder checkpoints (models_light.py:57-60, 81-84).  The module is rebuilt from the reference IntrospectionModule's
state_dict layout recorded in tests/golden/fcn_state_dict_layout.json (names, shapes, dtypes, parameter or buffer, in the reference's
order, num_batches_tracked included; tests/golden/make_fcn_layout.py), so every file below carries the reference's own keys."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(ROOT, "tests", "golden", "fcn_state_dict_layout.json")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def layout_module(W):
    """an nn.Module whose state_dict has the recorded layout, floats from W; forward only has to be traceable"""
    import torch

    class Node(torch.nn.Module):
        def forward(self, x):
            return x

    class Root(torch.nn.Module):
        def forward(self, x):
            return x * self.decoder.conv_last.weight.mean() + self.decoder.conv_last.bias

    root = Root()
    for name, shape, dtype, kind in json.load(open(LAYOUT)):
        *path, leaf = name.split(".")
        mod = root
        for p in path:
            if not hasattr(mod, p):
                mod.add_module(p, Node())
            mod = getattr(mod, p)
        t = torch.zeros(shape, dtype=getattr(torch, dtype)) if name.endswith("num_batches_tracked") else torch.from_numpy(W[name].copy())
        assert tuple(t.shape) == tuple(shape) and str(t.dtype) == "torch." + dtype, name
        if kind == "parameter":
            mod.register_parameter(leaf, torch.nn.Parameter(t, requires_grad=False))
        else:
            mod.register_buffer(leaf, t)
    return root.eval()


@pytest.fixture(scope="module")
def model_and_weights():
    from iv_slam_amd import fcn_weights
    W = fcn_weights.make_seeded_weights(11)
    m = layout_module(W)
    assert [k for k in m.state_dict()] == [e[0] for e in json.load(open(LAYOUT))]
    return m, W


def test_torchscript_archive_state_dict_and_split_checkpoints(model_and_weights, tmp_path):
    import torch
    import export_fcn_weights as X
    from iv_slam_amd import fcn_weights
    m, W = model_and_weights
    want = fcn_weights.pack_blob(W)
    # (1) TorchScript archive, traced and saved as export_model_light.py does
    torch.manual_seed(0)
    with torch.no_grad():
        sm = torch.jit.trace(m, torch.rand(1, 3, 96, 128))
    pt = str(tmp_path / "iv_model_light.pt")
    sm.save(pt)
    out = str(tmp_path / "w1.bin")
    X.main([pt, out])
    assert np.array_equal(np.fromfile(out, np.float32), want)
    # (2) whole-module state_dict, bare and wrapped
    pth = str(tmp_path / "model.pth")
    torch.save(m.state_dict(), pth)
    assert np.array_equal(X.export(str(tmp_path / "w2.bin"), model=pth), want)
    torch.save({"state_dict": m.state_dict(), "epoch": 3}, pth)
    assert np.array_equal(X.export(str(tmp_path / "w3.bin"), model=pth), want)
    # (3) separate encoder / decoder checkpoints (bare keys), one of them from DataParallel ("module." prefix)
    e = str(tmp_path / "encoder_epoch_1.pth"); d = str(tmp_path / "decoder_epoch_1.pth")
    torch.save(m.encoder.state_dict(), e)
    torch.save({"module." + k: v for k, v in m.decoder.state_dict().items()}, d)
    X.main(["--encoder", e, "--decoder", d, str(tmp_path / "w4.bin")])
    assert np.array_equal(np.fromfile(str(tmp_path / "w4.bin"), np.float32), want)


def test_mismatching_checkpoints_fail_loudly(model_and_weights, tmp_path):
    import torch
    import export_fcn_weights as X
    m, _ = model_and_weights
    sd = dict(m.state_dict())
    del sd["encoder.features.7.conv.3.weight"]
    p = str(tmp_path / "short.pth"); torch.save(sd, p)
    with pytest.raises(X.WeightFormatError, match="missing"):
        X.export(str(tmp_path / "x.bin"), model=p)
    sd = dict(m.state_dict()); sd["decoder.cbr.0.weight"] = sd["decoder.cbr.0.weight"][:, :100]
    torch.save(sd, p)
    with pytest.raises(X.WeightFormatError, match="shape"):
        X.export(str(tmp_path / "x.bin"), model=p)
    sd = dict(m.state_dict()); sd["decoder.ppm.0.weight"] = torch.zeros(3)
    torch.save(sd, p)
    with pytest.raises(X.WeightFormatError, match="unexpected"):
        X.export(str(tmp_path / "x.bin"), model=p)
    # encoder and decoder paths swapped (the reference's own Jackal config does this and loads with strict=False: SURVEY D-15)
    e = str(tmp_path / "e.pth"); d = str(tmp_path / "d.pth")
    torch.save(m.encoder.state_dict(), e); torch.save(m.decoder.state_dict(), d)
    with pytest.raises(X.WeightFormatError):
        X.export(str(tmp_path / "x.bin"), encoder=d, decoder=e)
    with pytest.raises(SystemExit):
        X.main(["--encoder", e, str(tmp_path / "x.bin")])
