"""main_advtrain.py without a GPU: its parser is the reference's (tests/golden/seg_args.json) plus the additions, with main_aug_final.py's
defaults for the shared ones and --noise device; the checkpoint paths under adv_training/; every refusal comes before the GPU is asked
for and leaves nothing on disk; and the loud failure on a host."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.main_advtrain")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


def test_parser_equals_the_references_plus_the_additions(entry, pkg):
    ref = json.load(open(os.path.join(GOLDEN, "seg_args.json")))
    assert _table(entry.get_argparser()) == ref                   # same options, same order, same defaults
    full = _table(entry.get_full_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == entry.ADDITIONS == ("dtype", "layout", "synthetic", "max_side", "graph", "noise")
    aug = importlib.import_module("cv_a-fan_amd.main_aug_final")
    shared = {a["dest"]: a for a in _table(aug.get_full_argparser())[len(ref):]}
    for a in full[len(ref):-1]:
        assert a == shared[a["dest"]], a                             # main_aug_final.py's flags and defaults
    assert full[-1] == {"dest": "noise", "flags": ["--noise"], "default": "device"}
    assert tuple(a["dest"] for a in _table(aug.get_full_argparser())[len(ref):]) == aug.ADDITIONS == entry.ADDITIONS[:-1]   # untouched
    o = entry.get_full_argparser().parse_args(["E"])
    assert (o.steps_pgd, o.eps_pgd, o.gamma_pgd, o.randinit_pgd, o.clip_pgd, o.noise) == (1, 2, 0.5, False, False, "device")
    assert entry.get_full_argparser().parse_args(["E", "--noise", "host"]).noise == "host"
    with pytest.raises(SystemExit):
        entry.get_full_argparser().parse_args(["E", "--noise", "cpu"])
    assert entry.NUM_CLASSES == {"voc": 21, "cityscapes": 19}


def test_checkpoint_paths_are_under_adv_training(entry):
    o = entry.get_full_argparser().parse_args(["E", "--dataset", "cityscapes"])
    assert entry.ckpt_path(o) == "adv_training/E/latest_deeplabv3plus_resnet50_cityscapes_os16.pth"
    assert entry.ckpt_path(o, "best") == "adv_training/E/best_deeplabv3plus_resnet50_cityscapes_os16.pth"
    o = entry.get_full_argparser().parse_args(["advtrain_voc2012_resnet50_bs4_seed66", "--model", "deeplabv3_resnet101", "--output_stride", "8"])
    assert entry.ckpt_path(o) == "adv_training/advtrain_voc2012_resnet50_bs4_seed66/latest_deeplabv3_resnet101_voc_os8.pth"


def _no_gpu_question(monkeypatch):
    import torch

    def asked():
        raise AssertionError("torch.cuda.is_available was asked before the refusal")
    monkeypatch.setattr(torch.cuda, "is_available", asked)


@pytest.mark.parametrize("extra, exc, word", [
    (["--loss_type", "focal_loss"], NotImplementedError, "focal_loss"), (["--separable_conv"], NotImplementedError, "separable"),
    (["--model", "deeplabv3plus_mobilenet"], NotImplementedError, "mobilenet"), (["--model", "deeplabv3_mobilenet"], NotImplementedError, "mobilenet"),
    (["--save_val_results"], NotImplementedError, "save_val_results"),
    (["--batch_size", "8"], ValueError, r"main_advtrain\.py:184"), (["--batch_size", "2"], ValueError, r"main_advtrain\.py:184"),
    ([], ValueError, r"--batch_size 16.*main_advtrain\.py:184")])                    # (the parser's default is 16)
def test_refusals_come_before_any_device_work(entry, extra, exc, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _no_gpu_question(monkeypatch)
    args = ["E", "--synthetic", "8"] + ([] if "--batch_size" in extra or not extra else ["--batch_size", "4"]) + extra
    with pytest.raises(exc, match=word):
        entry.main(args)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("mode", ["--test_only", "--eval_pgd"])
def test_the_evaluations_refuse_the_same_flags_but_take_any_batch_size(entry, mode, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _no_gpu_question(monkeypatch)
    with pytest.raises(NotImplementedError, match="mobilenet"):
        entry.main(["E", mode, "ck.pth", "--model", "deeplabv3_mobilenet"])
    p = entry.get_full_argparser()
    entry.check_unbuilt(p.parse_args(["E", mode, "ck.pth"]))                          # batch size 16: no training loop to stall
    entry.check_unbuilt(p.parse_args(["E", "--batch_size", "4", "--enable_vis", "--dataset", "cityscapes"]))
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["--test_only", "ck.pth"], ["--eval_pgd", "ck.pth"], ["--dataset", "cityscapes", "--noise", "host"]])
def test_entry_fails_loudly_without_a_gpu(entry, monkeypatch, tmp_path, extra):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        entry.main(["E", "--synthetic", "4", "--batch_size", "4"] + extra)
    assert os.listdir(tmp_path) == []


def test_trainer_and_start_exist(pkg):
    import inspect
    st = pkg.seg_trainer
    assert issubclass(st.SegAdvTrainer, st.SegBaseTrainer) and callable(st.seg_adv_phases) and st.SegAdvTrainer._small == ("loss",)
    assert inspect.signature(pkg.pgd.start).parameters["noise"].default == "host"
    assert inspect.signature(pkg.seg_attack_algo.adv_input).parameters["noise"].default == "host"
    assert inspect.signature(st.SegAdvTrainer.__init__).parameters["noise"].default == "device"
