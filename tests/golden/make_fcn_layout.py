"""Records tests/golden/fcn_state_dict_layout.json: the state_dict layout of the reference's IntrospectionModule
(mobilenetv2dilated encoder + c1_deepsup decoder, IF/networks/models_light), as the reference's own Python model builds it.
Only names, shapes, dtypes and whether each entry is a parameter or a buffer are recorded -- no weights, nothing of the
reference's code -- so that tests/test_export_weights.py can rebuild a module with exactly that layout without the reference.

    python tests/golden/make_fcn_layout.py <the reference's introspection_function directory>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    from networks.models_light import models_light as ML, mobilenet  # the reference, read-only
    enc = ML.MobileNetV2Dilated(mobilenet.mobilenetv2(pretrained=False), 8)
    dec = ML.C1DeepSup(num_class=1, fc_dim=320, regression_mode=True, inference_mode=True, out_size=(96, 128))
    m = ML.IntrospectionModule(enc, dec, (512, 512), logistic_func=True).eval()
    params = {k for k, _ in m.named_parameters()}
    layout = [[k, list(v.shape), str(v.dtype).replace("torch.", ""), "parameter" if k in params else "buffer"]
              for k, v in m.state_dict().items()]
    out = os.path.join(HERE, "fcn_state_dict_layout.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in layout) + "\n]\n")
    print("wrote %s: %d entries" % (out, len(layout)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
