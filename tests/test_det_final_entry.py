"""train_aug_final.py and train_baseline.py without a GPU: both parsers against the names and defaults recorded from the reference's
own parsers (tests/golden/det_final_args.json, det_base_args.json, tools/gen_det_final_golden.py), the experiment string and the
checkpoint directories for the README's command, every refusal by its word — raised before anything is created on disk — and the
loud failure on a host."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN

BASE = ["-s", "voc2007", "-b", "resnet101"]
README = BASE + ["--batch_size=8", "--mix_layer", "0011", "--pertub_idx_se", "2", "--gamma_se", "1.0", "--gamma_sd", "0.1",
                 "--sd_adv_loss_weight", "0.3", "--only_roi_sd"]


@pytest.fixture(scope="module")
def final(pkg):
    return importlib.import_module("cv_a-fan_amd.train_aug_final")


@pytest.fixture(scope="module")
def base(pkg):
    return importlib.import_module("cv_a-fan_amd.train_baseline")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


@pytest.mark.parametrize("which, fixture, count", [("final", "det_final_args.json", 38), ("base", "det_base_args.json", 31)])
def test_parsers_equal_the_references(final, base, which, fixture, count):
    entry = {"final": final, "base": base}[which]
    ref = json.load(open(os.path.join(GOLDEN, fixture)))
    assert len(ref) == count
    assert _table(entry.get_argparser()) == ref                   # same options, same order, same defaults
    full = _table(entry.get_full_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == entry.ADDITIONS == ("synthetic", "dtype", "layout", "seed")
    with pytest.raises(SystemExit):
        entry.get_full_argparser().parse_args(["-b", "resnet101"])            # -s is required


def test_the_sat_program_keeps_its_parser(pkg):
    de = pkg.det_entry
    ref = json.load(open(os.path.join(GOLDEN, "det_args.json")))
    assert _table(de.get_argparser()) == ref and _table(de.get_full_argparser())[:len(ref)] == ref


def test_experiment_names_and_directories(final, base, pkg):
    o = final.get_full_argparser().parse_args(README)
    assert final.exp_name(o) == "s1se_2_sd_roi_g1.0e2_MIX0011"
    assert final.checkpoints_dir(o) == os.path.join("./outputs", "ckpt-s1se_2_sd_roi_g1.0e2_MIX0011-voc2007-resnet101")
    cfg = pkg.det_entry.config(o)
    assert cfg["batch_size"] == 8 and cfg["rpn_pre_nms_top_n"] == 12000
    s = pkg.det_entry.final_settings(o)
    assert s == dict(pertub_idx_se=2, mix_layer="0011", gamma_se=1.0, gamma_sd=0.1, sd_adv_loss_weight=0.3, only_roi_sd=True, mix_sd=False,
                     noise_sd=0, randinit=False, clip=False)
    o = final.get_full_argparser().parse_args(BASE + ["--mix_layer", "1100", "--pertub_idx_se", "3", "--randinit", "--clip", "--steps", "2",
                                                      "--eps", "4.0", "-o", "/tmp/x"])
    assert final.checkpoints_dir(o) == "/tmp/x/ckpt-s2se_3_sd_roi_g0.5e4.0_MIX1100_rand_clip-voc2007-resnet101"
    o = base.get_full_argparser().parse_args(BASE)
    assert base.checkpoints_dir(o) == os.path.join("./outputs", "checkpoints-voc2007-resnet101_baseline")
    lines = pkg.det_entry.final_banner(final.get_full_argparser().parse_args(README), "D")
    assert lines[2:6] == ["EXP: [SE + SAT + MIX + SD] Dataset: [voc2007]",
                          "SE : Layer:[2]  MIX:[0011]  Gamma:[1.0]  Eps:[2]  Randinit:[False] Clip:[False]",
                          "SD : Layer:[roi]  MIX:[False]  Gamma:[0.1]  AdvWeight:[0.3] Noise:[0] ROI:[True]", "DIR:[D]"]


OK_FINAL = ["--mix_layer", "0011", "--pertub_idx_se", "2"]


@pytest.mark.parametrize("argv, exc, word", [
    (["-s", "voc2007", "-b", "resnet18"] + OK_FINAL, NotImplementedError, "BasicBlock"),
    (["-s", "voc2007", "-b", "resnet50"] + OK_FINAL, NotImplementedError, "ResNet-101 is pinned"),
    (["-s", "coco2017", "-b", "resnet101"] + OK_FINAL, NotImplementedError, "pycocotools"),
    (["-s", "voc2007-cat-dog", "-b", "resnet101"] + OK_FINAL, NotImplementedError, "cat / dog subset"),
    (BASE + ["--mix_layer", "0011"], ValueError, "--pertub_idx_se None.*first forward"),
    (BASE + ["--mix_layer", "0011", "--pertub_idx_se", "0"], ValueError, "--pertub_idx_se 0"),
    (BASE + ["--mix_layer", "0011", "--pertub_idx_se", "4"], ValueError, "--pertub_idx_se 4"),
    (BASE + ["--pertub_idx_se", "2"], ValueError, "--mix_layer None.*train_aug_final.py:67"),
    (BASE + ["--pertub_idx_se", "2", "--mix_layer", "011"], ValueError, "--mix_layer 011: four 0/1 digits"),
    (BASE + ["--pertub_idx_se", "2", "--mix_layer", "0021"], ValueError, "--mix_layer 0021: four 0/1 digits"),
    (BASE + OK_FINAL + ["--pertub_idx_sd", "rpn"], ValueError, "--pertub_idx_sd rpn: only 'roi'"),
])
def test_final_refusals(final, argv, exc, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(exc, match=word):
        final.main(argv + ["--synthetic", "4"])
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("argv, word", [(["-s", "voc2007", "-b", "resnet18"], "BasicBlock"), (["-s", "voc2007", "-b", "resnet50"], "ResNet-101 is pinned"),
                                        (["-s", "coco2017-car", "-b", "resnet101"], "pycocotools"),
                                        (["-s", "voc2007-cat-dog", "-b", "resnet101"], "cat / dog subset")])
def test_base_refusals(base, argv, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match=word):
        base.main(argv + ["--synthetic", "4"])
    assert os.listdir(tmp_path) == []


def test_clip_is_the_references_name_error_not_a_refusal(pkg):
    o = pkg.det_entry.get_full_argparser(pkg.det_entry.get_final_argparser()).parse_args(BASE + OK_FINAL + ["--clip"])
    pkg.det_entry.check_unbuilt_final(o)                           # passes: the NameError is rpn_roi_PGD's, in the first iteration
    assert pkg.det_entry.final_settings(o)["clip"] is True


def test_trainer_settings_are_checked_before_any_work(pkg):
    dt = pkg.det_trainer
    with pytest.raises(ValueError, match="phases"):
        dt.DetTrainer(None, phases="other")
    with pytest.raises(ValueError, match="pertub_idx_se"):
        dt.DetTrainer(None, phases="final", final={"mix_layer": "0011"})
    with pytest.raises(ValueError, match="mix_layer"):
        dt.DetTrainer(None, phases="final", final={"pertub_idx_se": 2, "mix_layer": "2"})


@pytest.mark.parametrize("which", ["final", "base"])
def test_entries_fail_loudly_without_a_gpu(final, base, which, monkeypatch, tmp_path):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    entry, argv = (final, BASE + OK_FINAL) if which == "final" else (base, BASE)
    with pytest.raises(RuntimeError, match="MI355X"):
        entry.main(argv + ["--synthetic", "4"])
    assert os.listdir(tmp_path) == []
