"""main_seg_rob.main on the GPU: the reference's lines in the reference's order (Segmentation/main_advtrain.py:151-168), the scores of
seg_eval.pgd_validate, and — without steps — main_seg_val.main's scores on the same checkpoint and split."""
import importlib
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALARS = ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU")
COMMON = ["--synthetic", "4", "--max_side", "48", "--crop_val", "--crop_size", "33"]


@pytest.fixture(scope="module")
def checkpoint(pkg, tmp_path_factory):
    torch.manual_seed(0)
    m = pkg.deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=21, output_stride=16)
    state = m.state_dict()
    state["left.over.from.another.model"] = torch.zeros(3)
    path = str(tmp_path_factory.mktemp("rob") / "ck.pth")
    torch.save({"model_state": state}, path)
    return path, len(state) - 1


def test_main_prints_the_references_lines_and_returns_the_scores(pkg, gpu, checkpoint, tmp_path, monkeypatch, capsys):
    entry = importlib.import_module("cv_a-fan_amd.main_seg_rob")
    monkeypatch.chdir(tmp_path)
    ck, n_keys = checkpoint
    capsys.readouterr()
    score = entry.main(["--eval_pgd", ck] + COMMON + ["--steps_pgd", "2", "--clip_pgd"])
    out = capsys.readouterr().out
    settings = "Attack Settings: Step[2] Gamma[0.5] Eps[2] Randinit[False] Clip[True]"
    lines = ["Test Attack :[%s]" % ck, settings, "Overlap:[%d/%d]" % (n_keys, n_keys), "Dataset: voc, Val set: 4", settings, "Overall Acc: "]
    at, pos = [], 0
    for l in lines:
        pos = out.index(l, pos)
        at.append(pos)
        pos += len(l)
    assert out.count(settings) == 2
    assert set(score) == set(SCALARS) | {"Class IoU"} and all(math.isfinite(float(score[k])) for k in SCALARS)
    assert pkg.seg_eval.StreamSegMetrics.to_str(score) in out
    printed = {k: float(re.search(r"^%s: ([0-9.naninf-]+)$" % k, out, flags=re.M).group(1)) for k in SCALARS}
    assert all(abs(printed[k] - float(score[k])) <= 5.0000001e-7 for k in SCALARS)     # "%f": six decimals


def test_without_steps_the_scores_are_main_seg_vals(pkg, gpu, checkpoint, tmp_path, monkeypatch, capsys):
    rob = importlib.import_module("cv_a-fan_amd.main_seg_rob")
    val = importlib.import_module("cv_a-fan_amd.main_seg_val")
    monkeypatch.chdir(tmp_path)
    ck, _ = checkpoint
    clean = torch.load(ck, map_location="cpu")
    clean["model_state"].pop("left.over.from.another.model")          # (main_seg_val's restore is strict)
    torch.save(clean, "clean.pth")
    expected = val.main(["--ckpt", "clean.pth"] + COMMON)
    score = rob.main(["--eval_pgd", ck] + COMMON + ["--steps_pgd", "0"])
    capsys.readouterr()
    for k in SCALARS:
        assert float(score[k]) == float(expected[k]), k
    assert all((math.isnan(v) and math.isnan(score["Class IoU"][c])) or v == score["Class IoU"][c] for c, v in expected["Class IoU"].items())
