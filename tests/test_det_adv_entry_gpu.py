"""train_baseline_advtrain.py through det_entry.train on the GPU: the loop on the small detection network of
tests/test_det_entry_gpu.py over DetDeviceLoader on a synthetic split with trainer=DetTrainer(phases="adv", ...) — the learning rate
of every step, the checkpoints and their (the reference's four) keys, the log lines, and a run with host noise and a seed resumed
with -r that ends on the uninterrupted run's weights bit for bit.  And the program itself for one step on Faster-RCNN / ResNet-101
at image side 128: the reference's stdout lines, the directory it names, the checkpoint."""
import importlib
import os

import numpy as np
import pytest
import torch

from test_det_entry_gpu import _cfg, _TinyDet

pytestmark = pytest.mark.gpu

ADV = dict(steps=2, eps=2.0, gamma=0.5, randinit=True, clip=True, noise="host")


def _run(pkg, gpu, cfg, out_dir, resume=None):
    de, dd = pkg.det_entry, pkg.det_data
    split = dd.SyntheticDetSplit(10, seed=6, min_side=40, max_side=60)
    loader = dd.DetDeviceLoader(split.images, split.boxes, split.classes, cfg["batch_size"], gpu, True, cfg["image_min_side"],
                                cfg["image_max_side"], seed=11)
    torch.manual_seed(5)
    model = _TinyDet().to(gpu).train()
    os.makedirs(out_dir, exist_ok=True)
    trainer = pkg.det_trainer.DetTrainer(model, lr=cfg["learning_rate"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                                         phases="adv", adv=ADV)
    out = de.train(model, loader, cfg, str(out_dir), de.Log(os.path.join(str(out_dir), "train.log")), resume, seed=11, trainer=trainer)
    assert out["trainer"] is trainer
    return out, model


def test_loop_checkpoints_and_resume(pkg, gpu, tmp_path, capsys):
    de = pkg.det_entry
    cfg = _cfg(de, num_steps_to_finish=3)
    before = pkg.ops.CALLS["det_batch_resize"]
    out, model = _run(pkg, gpu, cfg, tmp_path / "a")
    assert out["step"] == 3 and out["trainer"].phases == "adv" and pkg.ops.CALLS["det_batch_resize"] - before == 3
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
    for line in ("Start training with 1 GPUs (2 batches per GPU)", "[Step 2] Avg. Loss = ",
                 "Model has been saved to " + str(tmp_path / "a" / "model-2.pth"),
                 "Model has been saved to " + str(tmp_path / "a" / "model-3.pth"), "Done"):
        assert line in text and line in log, line
    assert "LR = {:.8f}".format(de.warmup_multistep_lr(2, 0.01, [2], 0.1, 0.3333, 4)) in log and "samples/sec; ETA" in log

    # -r model-2.pth with host noise and the seed, one more step: the uninterrupted run's weights, bit for bit
    out2, model2 = _run(pkg, gpu, cfg, tmp_path / "b", resume=str(tmp_path / "a" / "model-2.pth"))
    assert out2["step"] == 3 and out2["lrs"] == out["lrs"][2:]
    assert "Model has been restored from file: " + str(tmp_path / "a" / "model-2.pth") in capsys.readouterr().out
    sd, sd2 = model.state_dict(), model2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert torch.equal(out["losses"][2], out2["losses"][0])
    assert torch.equal(out["trainer"].arena.momentum_buf, out2["trainer"].arena.momentum_buf)
    ck0 = torch.load(tmp_path / "a" / "model-2.pth", map_location="cpu", weights_only=False)["state_dict"]
    assert not all(torch.equal(ck0[k], sd[k].cpu()) for k in sd)                  # (the third step moved the weights)


SMALL = ["--image_min_side", "128", "--image_max_side", "160", "--anchor_sizes", "[64]", "--rpn_pre_nms_top_n", "200", "--rpn_post_nms_top_n", "64"]


@pytest.mark.parametrize("noise", ["host", "device"])
def test_program_one_step(pkg, gpu, tmp_path, capsys, noise):
    adv = importlib.import_module("cv_a-fan_amd.train_baseline_advtrain")
    before = dict(pkg.ops.CALLS)
    out = adv.main(["-s", "voc2007", "-b", "resnet101", "--synthetic", "8", "--batch_size", "2", "--num_steps_to_finish", "1",
                    "--num_steps_to_display", "1", "--seed", "3", "-o", str(tmp_path), "--randinit", "--clip", "--noise", noise] + SMALL)
    torch.cuda.synchronize()
    tr = out["trainer"]
    assert out["step"] == 1 and np.isfinite(float(out["losses"][0])) and tr.phases == "adv"
    assert tr.adv == dict(steps=1, eps=2, gamma=0.5, randinit=True, clip=True, noise=noise) and tr.noise_ahead is None    # (a seed: no draw ahead)
    assert pkg.ops.CALLS["conv_fwd"] > before["conv_fwd"] and pkg.ops.CALLS["vendor_conv"] == 0
    d = tmp_path / "ckpt-s1g0.5e2_rand_clip-voc2007-resnet101"
    assert os.path.exists(d / "model-1.pth") and os.path.exists(d / "train.log")
    ck = torch.load(d / "model-1.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"state_dict", "step", "optimizer_state_dict", "scheduler_state_dict"} and ck["step"] == 1
    text = capsys.readouterr().out
    for line in ("create dir:[{}]".format(d), "INFO: PID   : [{}]".format(os.getpid()),
                 "EXP: Dataset:[voc2007] ADV Training Step:[1] Gamma:[0.5] Eps:[2] Randinit:[True] Clip:[True]", "DATASET:[voc2007] DIR:[./data]",
                 "Found 8 samples", "Start training with 1 GPUs (2 batches per GPU)", "[Step 1] Avg. Loss = ", "Model has been saved to",
                 "Done", "=" * 100 + "\nFINISL!\n" + "=" * 100):
        assert line in text, line
    assert text.index("randinit") < text.index("INFO: PID") < text.index("EXP: Dataset") < text.index("DATASET:[voc2007]")
    log = open(d / "train.log").read()
    assert "BATCH_SIZE = 2" in log and "\trandinit = True" in log and "\tnoise = " + noise in log and "[Step 1] Avg. Loss = " in log
