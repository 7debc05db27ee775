"""main_aug_final.py without a GPU: its parser against the names and defaults recorded from the reference's own parser
(tests/golden/seg_args.json), the experiment string, the flags with nothing behind them, and the loud failure on a host."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.main_aug_final")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


def test_parser_equals_the_references(entry):
    ref = json.load(open(os.path.join(GOLDEN, "seg_args.json")))
    assert len(ref) == 52
    assert _table(entry.get_argparser()) == ref                   # same options, same order, same defaults
    full = _table(entry.get_full_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == entry.ADDITIONS == ("dtype", "layout", "synthetic", "max_side", "graph")
    o = entry.get_full_argparser().parse_args(["EXP01"])
    assert (o.dtype, o.layout, o.synthetic, o.max_side, o.graph) == ("bf16", "nhwc", 0, 0, 1)
    assert o.total_itrs == 30e3 and o.crop_size == 513 and o.lr == 0.01 and o.batch_size == 16


def test_exp_string_and_checkpoint_path(entry):
    o = entry.get_full_argparser().parse_args(["EXP01", "--pertub_idx_sd", "aspp", "--gamma_se", "0.01", "--gamma_sd", "0.4",
                                               "--adv_loss_weight_sd", "0.3", "--mix_layer", "11"])
    assert entry.exp_name(o) == "voc_EXP01_selayer_3_sdlayer_aspp_gamma_se0.01_gamma_sd0.4_advweight0.3MIX11"
    o.exp = entry.exp_name(o)
    assert entry.ckpt_path(o) == ("checkpoints/voc_EXP01_selayer_3_sdlayer_aspp_gamma_se0.01_gamma_sd0.4_advweight0.3MIX11/"
                                  "latest_deeplabv3plus_resnet50_voc_os16.pth")
    o = entry.get_full_argparser().parse_args(["x"])
    assert entry.exp_name(o) == "voc_x_selayer_3_sdlayer__gamma_se0.5_gamma_sd0.5_advweight0.5MIX"


def test_print_args_format(entry, capsys):
    o = entry.get_full_argparser().parse_args(["E"])
    entry.print_args(o)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "exp" + "." * 76 + "E" and all(len(l) == 80 for l in lines[:-1] if l) and lines[-1] == ""


@pytest.mark.parametrize("extra, word", [(["--test_only", "ck.pth"], "validation"), (["--eval_pgd", "ck.pth"], "validation"),
                                         (["--save_val_results"], "validation"), (["--dataset", "cityscapes"], "ExtColorJitter"),
                                         (["--model", "deeplabv3_mobilenet"], "mobilenet")])
def test_unbuilt_flags_raise(entry, extra, word, capsys):
    with pytest.raises(NotImplementedError, match=word):
        entry.main(["E", "--mix_layer", "11", "--pertub_idx_sd", "aspp"] + extra)


def test_entry_fails_loudly_without_a_gpu(entry, monkeypatch, tmp_path):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        entry.main(["E", "--mix_layer", "11", "--pertub_idx_sd", "aspp", "--synthetic", "4"])
    assert not os.path.exists(tmp_path / "checkpoints")


def test_load_voc_names_what_is_missing(pkg, tmp_path):
    pytest.importorskip("PIL")
    with pytest.raises(FileNotFoundError, match="no download"):
        pkg.seg_data.load_voc(str(tmp_path), "2012", "train")
