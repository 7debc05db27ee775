"""train_baseline_advtrain.py without a GPU: its parser against the names and defaults recorded from the reference's own parser
(tests/golden/det_adv_args.json, tools/gen_det_adv_golden.py) — which has no --pertub_idx —, the additions, the checkpoint directory
for all four start / clip combinations, the banner, every refusal by its word — raised before anything is created on disk —, the
trainer's settings checked in its constructor, and the loud failure on a host."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN

BASE = ["-s", "voc2007", "-b", "resnet101"]


@pytest.fixture(scope="module")
def adv(pkg):
    return importlib.import_module("cv_a-fan_amd.train_baseline_advtrain")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


def test_parser_equals_the_references(adv, pkg):
    ref = json.load(open(os.path.join(GOLDEN, "det_adv_args.json")))
    assert len(ref) == 30 and "pertub_idx" not in [r["dest"] for r in ref]
    assert _table(adv.get_argparser()) == ref                     # same options, same order, same defaults
    assert _table(pkg.det_entry.get_adv_argparser()) == ref
    full = _table(adv.get_full_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == adv.ADDITIONS == ("synthetic", "dtype", "layout", "seed", "noise")
    with pytest.raises(SystemExit):
        adv.get_full_argparser().parse_args(["-b", "resnet101"])              # -s is required
    with pytest.raises(SystemExit):
        adv.get_full_argparser().parse_args(BASE + ["--pertub_idx", "3"])     # the image attack has no layer index
    with pytest.raises(SystemExit):
        adv.get_full_argparser().parse_args(BASE + ["--noise", "other"])
    o = adv.get_full_argparser().parse_args(BASE)
    assert o.noise == pkg.det_entry.ADV_NOISE_DEFAULT and o.noise in ("host", "device")
    assert adv.get_full_argparser().parse_args(BASE + ["--noise", "device"]).noise == "device"
    assert adv.get_full_argparser().parse_args(BASE + ["--noise", "host"]).noise == "host"


@pytest.mark.parametrize("flags, tail", [([], ""), (["--randinit"], "_rand"), (["--clip"], "_clip"), (["--randinit", "--clip"], "_rand_clip")])
def test_checkpoint_directory(adv, pkg, flags, tail, tmp_path, capsys):
    o = adv.get_full_argparser().parse_args(BASE + flags)
    assert adv.exp_name(o) == "s1g0.5e2" + tail
    assert adv.checkpoints_dir(o) == os.path.join("./outputs", "ckpt-s1g0.5e2" + tail + "-voc2007-resnet101")
    o = adv.get_full_argparser().parse_args(BASE + flags + ["--steps", "3", "--gamma", "1.0", "--eps", "4.0", "-o", str(tmp_path)])
    d = os.path.join(str(tmp_path), "ckpt-s3g1.0e4.0" + tail + "-voc2007-resnet101")
    assert adv.checkpoints_dir(o) == d and not os.path.exists(d)              # naming creates nothing
    assert capsys.readouterr().out == ""
    assert pkg.det_entry.adv_checkpoints_dir(o, create=True) == d and os.path.isdir(d)
    assert capsys.readouterr().out == "create dir:[{}]\n".format(d)
    assert pkg.det_entry.adv_checkpoints_dir(o, create=True) == d
    assert capsys.readouterr().out == ""                                       # the line only when the directory is created


def test_settings_and_banner(adv, pkg):
    de = pkg.det_entry
    o = adv.get_full_argparser().parse_args(BASE + ["--randinit", "--clip", "--batch_size=8", "--noise", "device"])
    assert de.adv_settings(o) == dict(steps=1, eps=2, gamma=0.5, randinit=True, clip=True, noise="device")
    assert de.config(o)["batch_size"] == 8
    lines = de.adv_banner(o)
    assert lines[0] == lines[3] == "-" * 100 and lines[1] == "INFO: PID   : [{}]".format(os.getpid())
    assert lines[2] == "EXP: Dataset:[voc2007] ADV Training Step:[1] Gamma:[0.5] Eps:[2] Randinit:[True] Clip:[True]"


@pytest.mark.parametrize("argv, exc, word", [
    (["-s", "voc2007", "-b", "resnet18"], NotImplementedError, "BasicBlock"),
    (["-s", "voc2007", "-b", "resnet50"], NotImplementedError, "ResNet-101 is pinned"),
    (["-s", "coco2017", "-b", "resnet101"], NotImplementedError, "pycocotools"),
    (["-s", "coco2017-animal", "-b", "resnet101"], NotImplementedError, "pycocotools"),
    (["-s", "voc2007-cat-dog", "-b", "resnet101"], NotImplementedError, "cat / dog subset"),
    (BASE + ["--steps", "-1"], ValueError, "--steps -1"),
])
def test_refusals(adv, argv, exc, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(exc, match=word):
        adv.main(argv + ["--synthetic", "4"])
    assert os.listdir(tmp_path) == []


def test_trainer_settings_are_checked_before_any_work(pkg):
    dt = pkg.det_trainer
    assert dt.DetTrainer.PHASES == ("sat", "final", "base", "adv")
    with pytest.raises(ValueError, match="phases"):
        dt.DetTrainer(None, phases="advtrain")
    with pytest.raises(ValueError, match="noise"):
        dt.DetTrainer(None, phases="adv", adv={"noise": "gpu"})
    for steps in (-1, 1.5, None):
        with pytest.raises(ValueError, match="steps"):
            dt.DetTrainer(None, phases="adv", adv={"steps": steps})
    with pytest.raises(ValueError, match="unknown settings"):
        dt.DetTrainer(None, phases="adv", adv={"pertub_idx": 3})


def test_entry_fails_loudly_without_a_gpu(adv, monkeypatch, tmp_path, capsys):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        adv.main(BASE + ["--synthetic", "4", "--randinit"])
    assert os.listdir(tmp_path) == []
    assert "randinit" in capsys.readouterr().out              # (print_args came first, as in the reference)
