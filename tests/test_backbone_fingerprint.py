"""Seeded construction of every Bottleneck-ResNet model keeps its fingerprint: the ordered state_dict keys with their shapes and the
float64 sum of every tensor, against tests/golden/backbone_fingerprint.json (recorded before the two backbones got their common
skeleton, deeplab.BottleneckResNet).  Registration order, key names and the order in which construction draws from the generator
are what a checkpoint and a seeded run depend on; any of them moving shows here.  No GPU: the models are built on the host.

`python tests/test_backbone_fingerprint.py` rewrites the fixture from the code as it stands."""
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_fingerprint.json")
CASES = [("deeplabv3plus_resnet50", 8), ("deeplabv3plus_resnet50", 16), ("deeplabv3plus_resnet101", 8), ("deeplabv3plus_resnet101", 16),
         ("deeplabv3_resnet50", 8), ("deeplabv3_resnet50", 16), ("fasterrcnn_resnet101", None)]


def _name(case):
    return case[0] if case[1] is None else "%s_os%d" % case


def fingerprint(pkg, case):
    """[[key, shape, float64 sum], ...] in state_dict order (numpy's pairwise sum over the logical element order: one thread, one order)."""
    arch, os_ = case
    torch.manual_seed(0)
    model = pkg.det_model.fasterrcnn_resnet101() if os_ is None else pkg.deeplab.MODELS[arch](num_classes=21, output_stride=os_)
    return [[k, list(v.shape), float(np.sum(v.detach().contiguous().numpy().reshape(-1).astype(np.float64)))]
            for k, v in model.state_dict().items()]


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_seeded_construction_keeps_its_fingerprint(pkg, case):
    with open(GOLDEN) as f:
        want = json.load(f)[_name(case)]
    got = fingerprint(pkg, case)
    assert [r[:2] for r in got] == [r[:2] for r in want]              # keys, their order, shapes
    assert got == want                                                # ... and every tensor's sum, exactly


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    pkg_ = importlib.import_module("cv_a-fan_amd")
    with open(GOLDEN, "w") as f:
        json.dump({_name(c): fingerprint(pkg_, c) for c in CASES}, f, separators=(",", ":"))
        f.write("\n")
