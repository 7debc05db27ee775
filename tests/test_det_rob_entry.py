"""eval_rob_ori.py without a GPU: its parser against the names and defaults recorded from the reference's own parser
(tests/golden/det_rob_args.json), the PGD defaults, the refusals before any device work, and convert_dict (model.py:420-437 as
written: every occurrence of the digit is replaced) on a hand-written key list."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.eval_rob_ori")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


BASE = ["-s", "voc2007", "-b", "resnet101", "model-1.pth"]


def test_parser_equals_the_references(entry, pkg):
    ref = json.load(open(os.path.join(GOLDEN, "det_rob_args.json")))
    assert len(ref) == 17 and ref[-1] == {"dest": "checkpoint", "flags": [], "default": None}
    assert [r["dest"] for r in ref[:6]] == ["steps", "gamma", "eps", "randinit", "clip", "convert"]
    assert _table(entry.get_argparser(full=False)) == ref          # same options, same order, same defaults
    full = _table(entry.get_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == entry.ADDITIONS == ("synthetic", "dtype", "layout")
    eval_ref = json.load(open(os.path.join(GOLDEN, "det_eval_args.json")))
    assert ref[6:] == eval_ref                                     # eval.py's flags behind the PGD settings
    with pytest.raises(SystemExit):
        entry.get_argparser().parse_args(["-s", "voc2007", "-b", "resnet101"])          # the checkpoint is required


def test_pgd_defaults(entry):
    o = entry.get_argparser().parse_args(BASE)
    assert (o.steps, o.gamma, o.eps) == (10, 0.5, 2) and isinstance(o.steps, int)
    assert (o.randinit, o.clip, o.convert) == (False, False, False)
    assert (o.synthetic, o.dtype, o.layout, o.checkpoint, o.data_dir) == (0, "bf16", "nhwc", "model-1.pth", "./data")
    o = entry.get_argparser().parse_args(["--steps", "3", "--gamma", "1", "--eps", "4", "--randinit", "--clip", "--convert"] + BASE)
    assert (o.steps, o.gamma, o.eps, o.randinit, o.clip, o.convert) == (3, 1.0, 4.0, True, True, True)


@pytest.mark.parametrize("argv, word", [(["-s", "voc2007", "-b", "resnet18"], "BasicBlock"), (["-s", "voc2007", "-b", "resnet50"], "ResNet-101 is pinned"),
                                        (["-s", "coco2017", "-b", "resnet101"], "pycocotools"),
                                        (["-s", "voc2007-cat-dog", "-b", "resnet101"], "cat / dog subset")])
def test_refusals_come_before_any_device_work(entry, pkg, argv, word, tmp_path, capsys):
    with pytest.raises(NotImplementedError, match=word):
        entry.main(argv + [str(tmp_path / "model-1.pth")])
    assert os.listdir(tmp_path) == []                              # no results directory either
    assert "steps" + "." * (80 - len("steps") - 2) + "10" in capsys.readouterr().out       # print_args ran first


def test_convert_dict_as_written(pkg):
    keys = ["features.0.weight", "features.1.running_mean", "features.4.2.conv1.weight", "features.5.3.bn2.bias", "features.6.5.conv2.weight",
            "features.6.16.bn1.weight", "features.6.6.conv3.weight", "rpn._features.0.weight", "detection._hidden.0.conv1.weight",
            "features.1.num_batches_tracked"]
    src = {k: i for i, k in enumerate(keys)}
    out = pkg.det_entry.convert_dict(src)
    assert list(out.items()) == [
        ("features.conv1.weight", 0), ("features.bn1.running_mean", 1), ("features.layer1.2.conv1.weight", 2),
        ("features.layer2.3.bn2.bias", 3), ("features.layer3.5.conv2.weight", 4),
        ("features.layer3.1layer3.bn1.weight", 5),                 # block 16: mangled (every "6" is replaced), dropped by the overlap rule
        ("features.layer3.layer3.conv3.weight", 6),                # block 6: mangled
        ("rpn._features.0.weight", 7),                             # left alone
        ("detection._hidden.0.conv1.weight", 8), ("features.bn1.num_batches_tracked", 9)]
    model_keys = set(pkg.det_model.Model(pkg.det_model.ResNet101(layers=(1, 1, 7, 1)), 21).state_dict().keys())
    kept = [k for k in out if k in model_keys]
    assert "features.conv1.weight" in kept and "features.layer3.5.conv2.weight" in kept and "features.bn1.running_mean" in kept
    assert not any("layer3.layer3" in k or "1layer3" in k for k in kept)
