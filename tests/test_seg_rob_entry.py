"""main_seg_rob.py without a GPU: its parser against the reference's flag names and defaults (tests/golden/seg_args.json), its loud
failure on a host, and the checkpoint loader's overlap rule (Segmentation/main_advtrain.py:156-161)."""
import importlib
import json
import os

import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

SHARED = ("eval_pgd", "steps_pgd", "gamma_pgd", "eps_pgd", "randinit_pgd", "clip_pgd", "data_root", "dataset", "model", "output_stride",
          "crop_val", "val_batch_size", "crop_size", "gpu_id", "random_seed", "year")


@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.main_seg_rob")


def test_parser_is_the_references(entry):
    ref = {a["dest"]: a for a in json.load(open(os.path.join(GOLDEN, "seg_args.json")))}
    table = [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in entry.get_argparser()._actions
             if a.dest != "help"]
    assert tuple(a["dest"] for a in table) == SHARED + entry.ADDITIONS == SHARED + ("dtype", "layout", "synthetic", "max_side")
    for a in table[:len(SHARED)]:
        assert a == ref[a["dest"]], a["dest"]
    o = entry.get_argparser().parse_args(["--eval_pgd", "ck.pth"])
    assert (o.dtype, o.layout, o.synthetic, o.max_side) == ("bf16", "nhwc", 0, 0)
    train = importlib.import_module("cv_a-fan_amd.main_aug_final").get_full_argparser().parse_args(["E"])
    assert all(getattr(o, k) == getattr(train, k) for k in entry.ADDITIONS)      # the additions default as the training entry's
    assert all(getattr(o, k) == getattr(train, k) for k in SHARED if k != "eval_pgd")


@pytest.mark.parametrize("argv", [[], ["--eval_pgd", ""]])
def test_a_checkpoint_is_required(entry, argv, capsys):
    with pytest.raises(SystemExit) as e:
        entry.get_argparser().parse_args(argv)
    assert e.value.code == 2 and "--eval_pgd" in capsys.readouterr().err


def test_entry_fails_loudly_without_a_gpu(entry, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        entry.main(["--eval_pgd", "ck.pth", "--synthetic", "4", "--crop_val", "--crop_size", "33", "--max_side", "48"])
    assert not os.listdir(tmp_path)


def test_mobilenet_raises(entry):
    with pytest.raises(NotImplementedError, match="mobilenet"):
        entry.main(["--eval_pgd", "ck.pth", "--model", "deeplabv3_mobilenet"])


def test_overlap_loader(entry, tmp_path, capsys):
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4))
    keys = list(model.state_dict())
    assert len(keys) == 7
    kept = model.state_dict()["1.running_var"].clone()
    ck = {"0.weight": torch.full((4, 3, 1, 1), 2.0), "1.running_mean": torch.full((4,), 3.0), "not.in.the.model": torch.zeros(2)}
    path = str(tmp_path / "ck.pth")
    torch.save({"model_state": ck, "cur_itrs": 5}, path)
    assert entry.load_overlap(model, path) == (2, 7)
    assert capsys.readouterr().out == "Overlap:[2/7]\n"
    now = model.state_dict()
    assert torch.equal(now["0.weight"], ck["0.weight"]) and torch.equal(now["1.running_mean"], ck["1.running_mean"])
    assert torch.equal(now["1.running_var"], kept) and "not.in.the.model" not in now


def test_training_entry_names_the_program(pkg):
    train = importlib.import_module("cv_a-fan_amd.main_aug_final")
    with pytest.raises(NotImplementedError, match="main_seg_rob.py"):
        train.main(["E", "--mix_layer", "11", "--pertub_idx_sd", "aspp", "--eval_pgd", "ck.pth"])
