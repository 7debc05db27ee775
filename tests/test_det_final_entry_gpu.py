"""train_aug_final.py and train_baseline.py through det_entry.train on the GPU: the loop on the small detection network of
tests/test_det_entry_gpu.py over DetDeviceLoader on a synthetic split — the learning rate of every step, the checkpoints and their
keys, the log lines, and a run resumed with -r and a seed that ends on the uninterrupted run's weights bit for bit.  And the
documented path end to end on Faster-RCNN / ResNet-101 at image side 128: train_aug_final.py for one step at batch 2, then eval.py
on the checkpoint it wrote."""
import importlib
import os

import numpy as np
import pytest
import torch

from test_det_entry_gpu import _cfg, _TinyDet

pytestmark = pytest.mark.gpu

FINAL = dict(pertub_idx_se=2, mix_layer="0011", gamma_se=1.0, gamma_sd=0.1, sd_adv_loss_weight=0.3, only_roi_sd=True, mix_sd=True,
             noise_sd=0.01, randinit=True)


def _run(pkg, gpu, phases, cfg, out_dir, resume=None):
    de, dd = pkg.det_entry, pkg.det_data
    split = dd.SyntheticDetSplit(10, seed=6, min_side=40, max_side=60)
    loader = dd.DetDeviceLoader(split.images, split.boxes, split.classes, cfg["batch_size"], gpu, True, cfg["image_min_side"],
                                cfg["image_max_side"], seed=11)
    torch.manual_seed(5)
    model = _TinyDet().to(gpu).train()
    os.makedirs(out_dir, exist_ok=True)
    factory = de.trainer_factory(phases, FINAL if phases == "final" else None)
    out = de.train(model, loader, cfg, str(out_dir), de.Log(os.path.join(str(out_dir), "train.log")), resume, seed=11, trainer=factory)
    return out, model


@pytest.mark.parametrize("phases", ["final", "base"])
def test_loop_checkpoints_and_resume(pkg, gpu, tmp_path, capsys, phases):
    de = pkg.det_entry
    cfg = _cfg(de, num_steps_to_finish=3)
    out, model = _run(pkg, gpu, phases, cfg, tmp_path / "a")
    assert out["step"] == 3 and out["trainer"].phases == phases
    losses = torch.stack(out["losses"]).cpu().numpy()
    assert losses.shape == (3,) and np.isfinite(losses).all()
    assert out["lrs"] == [de.warmup_multistep_lr(t, 0.01, [2], 0.1, 0.3333, 4) for t in range(3)]
    assert float(out["trainer"].optimizer.arena.lr[0]) == np.float32(out["lrs"][2])
    for step in (2, 3):
        ck = torch.load(tmp_path / "a" / f"model-{step}.pth", map_location="cpu", weights_only=False)
        assert set(ck) == {"state_dict", "step", "optimizer_state_dict", "scheduler_state_dict"} and ck["step"] == step
        assert set(ck["state_dict"]) == set(model.state_dict()) and ck["scheduler_state_dict"]["last_epoch"] == step
    assert not os.path.exists(tmp_path / "a" / "model-1.pth")
    text = capsys.readouterr().out
    log = open(tmp_path / "a" / "train.log").read()
    for line in ("[Step 2] Avg. Loss = ", "Model has been saved to " + str(tmp_path / "a" / "model-2.pth"),
                 "Model has been saved to " + str(tmp_path / "a" / "model-3.pth"), "Done"):
        assert line in text and line in log
    assert "LR = {:.8f}".format(de.warmup_multistep_lr(2, 0.01, [2], 0.1, 0.3333, 4)) in log and "samples/sec; ETA" in log

    # -r model-2.pth with the seed, one more step: the uninterrupted run's weights, bit for bit
    out2, model2 = _run(pkg, gpu, phases, cfg, tmp_path / "b", resume=str(tmp_path / "a" / "model-2.pth"))
    assert out2["step"] == 3 and out2["lrs"] == out["lrs"][2:]
    sd, sd2 = model.state_dict(), model2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert torch.equal(out["losses"][2], out2["losses"][0])
    assert torch.equal(out["trainer"].arena.momentum_buf, out2["trainer"].arena.momentum_buf)
    ck0 = torch.load(tmp_path / "a" / "model-2.pth", map_location="cpu", weights_only=False)["state_dict"]
    assert not all(torch.equal(ck0[k], sd[k].cpu()) for k in sd)                  # (the third step moved the weights)


SMALL = ["--image_min_side", "128", "--image_max_side", "160", "--anchor_sizes", "[64]", "--rpn_pre_nms_top_n", "200", "--rpn_post_nms_top_n", "64"]


def test_documented_path_train_then_evaluate(pkg, gpu, tmp_path, capsys):
    final = importlib.import_module("cv_a-fan_amd.train_aug_final")
    ev = importlib.import_module("cv_a-fan_amd.eval")
    before = dict(pkg.ops.CALLS)
    out = final.main(["-s", "voc2007", "-b", "resnet101", "--synthetic", "8", "--batch_size", "2", "--num_steps_to_finish", "1",
                      "--num_steps_to_display", "1", "--seed", "3", "-o", str(tmp_path), "--mix_layer", "0011", "--pertub_idx_se", "2",
                      "--gamma_se", "1.0", "--gamma_sd", "0.1", "--sd_adv_loss_weight", "0.3", "--only_roi_sd"] + SMALL)
    torch.cuda.synchronize()
    assert out["step"] == 1 and np.isfinite(float(out["losses"][0])) and out["trainer"].phases == "final"
    assert pkg.ops.CALLS["conv_fwd"] > before["conv_fwd"] and pkg.ops.CALLS["vendor_conv"] == 0
    d = tmp_path / "ckpt-s1se_2_sd_roi_g1.0e2_MIX0011-voc2007-resnet101"
    assert os.path.exists(d / "model-1.pth") and os.path.exists(d / "train.log")
    text = capsys.readouterr().out
    for line in ("EXP: [SE + SAT + MIX + SD] Dataset: [voc2007]", "SE : Layer:[2]  MIX:[0011]  Gamma:[1.0]  Eps:[2]  Randinit:[False] Clip:[False]",
                 "SD : Layer:[roi]  MIX:[False]  Gamma:[0.1]  AdvWeight:[0.3] Noise:[0] ROI:[True]", "DIR:[{}]".format(d), "Found 8 samples",
                 "[Step 1] Avg. Loss = ", "Model has been saved to", "Done", "FINISL!"):
        assert line in text, line
    log = open(d / "train.log").read()
    assert "BATCH_SIZE = 2" in log and "\tmix_layer = 0011" in log and "[Step 1] Avg. Loss = " in log
    del out
    mean_ap, detail = ev.main(["-s", "voc2007", "-b", "resnet101", "--synthetic", "4"] + SMALL + [str(d / "model-1.pth")])
    assert 0.0 <= mean_ap <= 1.0 and len(detail.splitlines()) == 20
    assert "Load Weight:[" in capsys.readouterr().out


def test_baseline_program_one_step(pkg, gpu, tmp_path, capsys):
    base = importlib.import_module("cv_a-fan_amd.train_baseline")
    out = base.main(["-s", "voc2007", "-b", "resnet101", "--synthetic", "8", "--batch_size", "2", "--num_steps_to_finish", "1",
                     "--num_steps_to_display", "1", "--seed", "3", "-o", str(tmp_path)] + SMALL)
    torch.cuda.synchronize()
    assert out["step"] == 1 and np.isfinite(float(out["losses"][0])) and out["trainer"].phases == "base"
    d = tmp_path / "checkpoints-voc2007-resnet101_baseline"
    assert os.path.exists(d / "model-1.pth") and os.path.exists(d / "train.log")
    text = capsys.readouterr().out
    for line in ("Training Baseline ! DATASET:[voc2007] DIR:[./data]", "Found 8 samples", "[Step 1] Avg. Loss = ", "Done"):
        assert line in text, line
