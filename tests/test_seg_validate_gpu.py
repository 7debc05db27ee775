"""seg_eval.validate, main_seg_val.main and the validation step of main_aug_final.main on the GPU.  validate() scores the classifier's
low-resolution logits in one launch per batch; the expected value takes the SAME model's full-resolution route — the reference's:
resized logits, max(dim=1)[1].cpu().numpy(), numpy's _fast_hist and the reference formulas (tests/seg_eval_refs.py).  The matrix is
equal exactly; the scores agree to rel 1e-12 (same float64 formulas on the same matrix)."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import seg_eval_refs as E

pytestmark = pytest.mark.gpu

SCALARS = ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU")
SPLIT = dict(seed=1, min_side=36, max_side=48, classes=21)            # what main_seg_val --synthetic 4 --max_side 48 draws


@pytest.fixture(scope="module")
def split(pkg):
    return pkg.seg_data.SyntheticSegSplit(4, **SPLIT)


@pytest.fixture(scope="module")
def models(pkg, gpu):
    torch.manual_seed(0)
    out = {}
    for name, dtype, cl in (("bf16-nhwc", torch.bfloat16, True), ("fp32-nchw", torch.float32, False)):
        m = pkg.deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=21, output_stride=16)
        out[name] = m.set_compute_dtype(dtype).set_channels_last(cl).to(gpu).eval()
    return out


def _loader(pkg, split, gpu, crop_val):
    return pkg.seg_data.SegDeviceLoader(split.images, split.labels, 2, gpu, False, 33, crop_val=crop_val)


def _full_resolution_route(model, loader):
    hist = np.zeros((21, 21), np.int64)
    with torch.no_grad():
        for images, labels in loader:
            outputs = model({"x": images, "adv": None, "out_idx": 0, "flag": "clean"})
            assert tuple(outputs.shape) == (images.shape[0], 21) + tuple(images.shape[2:])
            hist += E.fast_hist(21, labels.cpu().numpy(), outputs.detach().max(dim=1)[1].cpu().numpy())
    return hist


class _Opts:
    save_val_results = False


@pytest.mark.parametrize("crop_val", [True, False], ids=["crop_val", "native"])
@pytest.mark.parametrize("config", ["bf16-nhwc", "fp32-nchw"])
def test_validate_equals_the_full_resolution_route(pkg, gpu, models, split, config, crop_val):
    model = models[config]
    loader = _loader(pkg, split, gpu, crop_val)
    assert len(loader) == (2 if crop_val else 4)
    ref = _full_resolution_route(model, loader)
    assert ref.sum() > 0
    stats = {k: v.clone() for k, v in model.state_dict().items()}
    metrics = pkg.seg_eval.StreamSegMetrics(21, gpu)
    metrics.update([np.zeros((2, 2), np.int64)], [np.zeros((2, 2), np.int64)])      # validate() resets what was there
    before = pkg.ops.CALLS["seg_confusion"]
    score, samples = pkg.seg_eval.validate(_Opts(), model, loader, gpu, metrics, ret_samples_ids=[0])
    assert samples == [] and pkg.ops.CALLS["seg_confusion"] - before == len(loader)
    assert model.training is False
    now = model.state_dict()
    assert all(torch.equal(v, now[k]) for k, v in stats.items())       # running statistics (and everything else): bit-unchanged
    assert np.array_equal(metrics.confusion_matrix, ref.astype(np.float64))
    exp = E.scores(ref)
    for k, e in zip(SCALARS, exp[:4]):
        assert float(score[k]) == pytest.approx(float(e), rel=1e-12, abs=0.0), k
    for c, e in enumerate(exp[4]):
        assert (math.isnan(e) and math.isnan(score["Class IoU"][c])) or score["Class IoU"][c] == pytest.approx(e, rel=1e-12, abs=0.0)
    # the caller's mode is the caller's: a model left in train() comes back in train()
    model.train()
    try:
        with pytest.raises(NotImplementedError):
            pkg.seg_eval.validate(type("O", (), {"save_val_results": True})(), model, loader, gpu, metrics)
        assert model.training is True
    finally:
        model.eval()


def test_update_logits_routes(pkg, gpu):
    """What update_logits does with each kind of logits: low-resolution fp32 (one launch), full-resolution fp32 (the same launch at equal
    sizes), bf16 (resized, then the launch), more classes than the kernel holds (torch's max and the host count)."""
    gen = torch.Generator().manual_seed(9)
    lo = torch.randn((2, 21, 9, 9), generator=gen).to(gpu).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 21, (2, 33, 33), generator=gen)
    t[torch.rand(t.shape, generator=gen) < 0.1] = 255
    t = t.to(gpu)
    full = pkg.ops.upsample_bilinear(lo, (33, 33))
    ref = E.fast_hist(21, t.cpu().numpy(), full.max(dim=1)[1].cpu().numpy())
    for out, labels in ((pkg.deeplab.LowResLogits(lo, (33, 33)), t), (full, t), (pkg.deeplab.LowResLogits(lo, (33, 33)), t.int())):
        m = pkg.seg_eval.StreamSegMetrics(21)
        before = pkg.ops.CALLS["seg_confusion"]
        m.update_logits(out, labels)
        assert pkg.ops.CALLS["seg_confusion"] == before + 1 and np.array_equal(m.confusion_matrix, ref)
    m.update_logits(full, t)
    m.update(t.cpu().numpy(), full.max(dim=1)[1].cpu())                 # device and host parts add up
    assert np.array_equal(m.confusion_matrix, 3.0 * ref)
    lb = lo.bfloat16()
    ref_b = E.fast_hist(21, t.cpu().numpy(), pkg.deeplab.interpolate(lb, (33, 33)).max(dim=1)[1].cpu().numpy())
    m = pkg.seg_eval.StreamSegMetrics(21)
    before = pkg.ops.CALLS["seg_confusion"]
    m.update_logits(pkg.deeplab.LowResLogits(lb, (33, 33)), t)
    assert pkg.ops.CALLS["seg_confusion"] == before + 1 and np.array_equal(m.confusion_matrix, ref_b)
    wide = torch.randn((1, 40, 5, 5), generator=gen).to(gpu)
    tw = torch.randint(0, 40, (1, 10, 10), generator=gen).to(gpu)
    m = pkg.seg_eval.StreamSegMetrics(40)
    m.update_logits(pkg.deeplab.LowResLogits(wide, (10, 10)), tw)
    assert pkg.ops.CALLS["seg_confusion"] == before + 1
    assert np.array_equal(m.confusion_matrix, E.fast_hist(40, tw.cpu().numpy(), pkg.deeplab.interpolate(wide, (10, 10)).max(dim=1)[1].cpu().numpy()))


def test_main_seg_val_scores_a_checkpoint(pkg, gpu, models, split, tmp_path, monkeypatch, capsys):
    entry = importlib.import_module("cv_a-fan_amd.main_seg_val")
    monkeypatch.chdir(tmp_path)
    model = models["bf16-nhwc"]
    torch.save({"model_state": model.state_dict()}, "ck.pth")
    expected, _ = pkg.seg_eval.validate(_Opts(), model, _loader(pkg, split, gpu, True), gpu, pkg.seg_eval.StreamSegMetrics(21, gpu))
    capsys.readouterr()
    score = entry.main(["--synthetic", "4", "--crop_val", "--crop_size", "33", "--max_side", "48", "--ckpt", "ck.pth",
                        "--val_batch_size", "2"])
    out = capsys.readouterr().out
    assert "Model restored from ck.pth" in out and "[!] Retrain" not in out and "Dataset: voc, Val set: 4" in out
    assert out.index("Model restored from") < out.index("Val set: 4") < out.index("Overall Acc")
    printed = {k: float(re.search(r"^%s: ([0-9.naninf-]+)$" % k, out, flags=re.M).group(1)) for k in SCALARS}
    for k in SCALARS:                                                  # "%f": six decimals
        assert abs(printed[k] - float(expected[k])) <= 5.0000001e-7, k
        assert float(score[k]) == float(expected[k]), k
    assert pkg.seg_eval.StreamSegMetrics.to_str(expected) in out
    entry.main(["--synthetic", "4", "--crop_val", "--crop_size", "33", "--max_side", "48", "--ckpt", "absent.pth", "--dtype", "fp32",
                "--layout", "nchw"])
    out = capsys.readouterr().out
    assert "[!] Retrain" in out and "Model restored" not in out and "Mean IoU: " in out


EXP = "voc_T_selayer_3_sdlayer_aspp_gamma_se0.5_gamma_sd0.5_advweight0.5MIX11"


def test_training_loop_validates_and_keeps_the_best(pkg, gpu, tmp_path, monkeypatch, capsys):
    entry = importlib.import_module("cv_a-fan_amd.main_aug_final")
    monkeypatch.chdir(tmp_path)
    splits = {"train": pkg.seg_data.SyntheticSegSplit(8, seed=2, min_side=36, max_side=48),
              "val": pkg.seg_data.SyntheticSegSplit(4, seed=3, min_side=36, max_side=48)}
    asked = []

    def load_voc(root, year="2012", image_set="train"):
        asked.append(image_set)
        return splits[image_set].images, splits[image_set].labels

    monkeypatch.setattr(pkg.seg_data, "load_voc", load_voc)
    losses = []
    step = pkg.seg_trainer.SegTrainer.step

    def spy(self, images, labels):
        assert self.model.training
        r = step(self, images, labels)
        losses.append(r["loss"])
        return r

    monkeypatch.setattr(pkg.seg_trainer.SegTrainer, "step", spy)
    before = pkg.ops.CALLS["seg_confusion"]
    entry.main(["T", "--model", "deeplabv3plus_resnet50", "--batch_size", "2", "--total_itrs", "3", "--val_interval", "2",
                "--crop_size", "33", "--crop_val", "--val_batch_size", "2", "--mix_layer", "11", "--pertub_idx_sd", "aspp"])
    out = capsys.readouterr().out
    assert asked == ["train", "val"] and "Dataset: voc, Train set: 8, Val set: 4" in out and "validation skipped" not in out
    assert pkg.ops.CALLS["seg_confusion"] - before == 2                 # 4 images in batches of 2, once
    latest = os.path.join("checkpoints", EXP, "latest_deeplabv3plus_resnet50_voc_os16.pth")
    best = os.path.join("checkpoints", EXP, "best_deeplabv3plus_resnet50_voc_os16.pth")
    i_latest, i_val, i_best = out.index(f"Model saved as {latest}"), out.index("validation..."), out.index(f"Model saved as {best}")
    assert i_latest < i_val < out.index("Overall Acc: ") < out.index("Mean Acc: ") < out.index("FreqW Acc: ") < out.index("Mean IoU: ") < i_best
    miou = float(re.search(r"^Mean IoU: ([0-9.]+)$", out, flags=re.M).group(1))
    ck = torch.load(best, map_location="cpu")
    assert set(ck) == {"cur_itrs", "model_state", "optimizer_state", "scheduler_state", "best_score"} and ck["cur_itrs"] == 2
    assert ck["best_score"] > 0 and abs(ck["best_score"] - miou) <= 5.0000001e-7
    assert torch.load(latest, map_location="cpu")["best_score"] == 0.0  # (saved before the validation, as the reference does)
    assert "syd: Setting: Layer:[aspp] Gamma:[0.5] Best IOU:[%s]" % ck["best_score"] in out
    # iteration 3 ran after the eval pass, in train mode, with a finite loss
    assert len(losses) == 3 and all(math.isfinite(float(l)) for l in losses)
