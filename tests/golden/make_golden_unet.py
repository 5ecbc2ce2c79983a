#!/usr/bin/env python3
"""Generate tests/golden/g21_unet.json and g21_unet.npz by RUNNING THE REFERENCE's U-Net generators and its SequentialNetwork on the
CPU of the build container.  The reference is imported through make_golden.import_reference; none of its source is copied, only
inputs, key lists and its results are stored.  Re-run:  python tests/golden/make_golden_unet.py  -- both files come out bit for bit
(fixed seeds, sorted JSON, and the archive is written with a fixed time stamp).

g21_unet.json
    "state_dicts"   label -> case key -> [[key, shape], ...] in the reference's state-dict order, at the parameters of
                    tests/unet_restatement.py CASES
    "defaults"      label -> [[key, shape], ...] at the reference's default constructor parameters (3 -> 3 channels)
    "sequential"    the structure of SequentialNetwork.state_dict() for a U-Net + embedding pair: the top-level keys in order, the
                    "net" entry, and per member its keys, type, frozen flag, network_params and model_state keys
g21_unet.npz
    <case key>_x / <case key>_y   the input (unet_restatement.case_input) and the reference's output in eval mode

The channel widths are the reference's, so no weights are stored: unet_restatement.fill gives every parameter and buffer, here and
in the tests.  The embedding network of the pair is a stand-in module registered under the label "cirnet" (the reference builds its
own from torchvision, which the container does not have); SequentialNetwork.state_dict() does not look inside a member's model.
"""
import json
import os
import sys

import numpy as np
import torch

from make_golden import HERE, import_reference
from make_golden_train import save_npz

sys.path.insert(0, os.path.dirname(HERE))
from unet_restatement import CASES, case_input, case_key, fill  # noqa: E402


def keys_and_shapes(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


class _Embedding(torch.nn.Module):
    def __init__(self, **params):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3)
        self.meta = {"in_channels": 3, "out_channels": 4, "mean": [0.485, 0.456, 0.406], "std": [0.229, 0.224, 0.225]}

    def forward(self, x):
        return self.conv(x).mean(dim=(2, 3)).t()


def sequential_structure():
    from mdir.components.model import network as registry
    from mdir.learning import network as RN
    registry.MODEL_LABELS["cirnet"] = _Embedding
    unet_params = {"architecture": "orig_unet", "in_channels": 3, "out_channels": 3, "nested_levels": 2, "min_channels": 4}
    cir_params = {"architecture": "cirnet", "cir_architecture": "alexnet", "local_whitening": False, "pooling": "gem",
                  "regional": False, "whitening": False, "pretrained": False}
    import copy
    unet = RN.SingleNetwork(registry.initialize_model(copy.deepcopy(unet_params)),
                            RN.SingleNetwork.NetworkParams(unet_params, {"wrappers": "", "data": {"transforms": "pil2np | totensor"}}),
                            "cpu", frozen=True)
    cir = RN.CirNetwork(registry.initialize_model(copy.deepcopy(cir_params)),
                        RN.SingleNetwork.NetworkParams(cir_params, {"wrappers": "", "data": {}}), "cpu", frozen=True)
    state = RN.SequentialNetwork({"unet": unet, "cirnet": cir}, ["unet", "cirnet"], device="cpu", frozen=True).state_dict()
    out = {"keys": list(state), "net": state["net"], "members": {}}
    for name in state["net"]["sequence"]:
        entry = state[name]
        out["members"][name] = {"keys": list(entry), "type": entry["type"], "frozen": entry["frozen"],
                                "network_params": entry["network_params"], "model_state_keys": list(entry["model_state"])}
    return out


def main():
    import_reference()
    from mdir.components.model import network as registry
    doc, arrays = {"state_dicts": {}, "defaults": {}, "sequential": None}, {}
    for label, cases in CASES.items():
        args = {} if label == "identity" else {"in_channels": 3, "out_channels": 3}
        doc["defaults"][label] = keys_and_shapes(registry.MODEL_LABELS[label](**args))
        doc["state_dicts"][label] = {}
        for k, (params, _) in enumerate(cases):
            net = fill(registry.MODEL_LABELS[label](**args, **params)).eval()
            doc["state_dicts"][label][case_key(label, k)] = keys_and_shapes(net)
            x = case_input(label, k)
            with torch.no_grad():
                y = net(torch.from_numpy(x)).numpy()
            assert np.isfinite(y).all() and np.abs(y).max() > 1e-3, (label, k, np.abs(y).max())
            arrays[case_key(label, k) + "_x"], arrays[case_key(label, k) + "_y"] = x, y
    doc["sequential"] = sequential_structure()
    with open(os.path.join(HERE, "g21_unet.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    path = os.path.join(HERE, "g21_unet.npz")
    save_npz(path, arrays)
    print("wrote %s: %d arrays, %d bytes; json %d bytes" % (path, len(arrays), os.path.getsize(path),
                                                            os.path.getsize(os.path.join(HERE, "g21_unet.json"))))


if __name__ == "__main__":
    main()
