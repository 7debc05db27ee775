"""Detection evaluation on the GPU: the eval-mode forward with the one-launch detection tail against the per-class loop (all four
tensors, bf16 channels-last and fp32 NCHW), det_eval.Evaluator on a stand-in model that returns the ground truth (AP 1 for every class
present, 0 for the others) and on a small Faster-RCNN with the tail on and off, and eval.py --synthetic end to end from a checkpoint."""
import importlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _small_model(pkg, gpu, dtype, nhwc):
    dm = pkg.det_model
    torch.manual_seed(11)
    m = dm.Model(dm.ResNet101(layers=(1, 1, 1, 1)), 21, rpn_post_nms_top_n=300)
    for b in m.modules():
        if isinstance(b, dm.Bottleneck):
            b.bn3.weight.data.mul_(0.2)
    m.detection._proposal_class.weight.data.mul_(40.0)                 # an untrained head gives ~1 / 21 everywhere: sharpen it past 0.05
    return m.set_compute_dtype(dtype).set_channels_last(nhwc).to(gpu).eval()


def _forward(pkg, monkeypatch, m, x, on, min_prob=None):
    monkeypatch.setattr(pkg.det_model.Model, "CLASS_NMS", on)
    d = {"x": x, "adv": None, "out_idx": None, "flag": "clean"}
    if min_prob is not None:
        d["min_prob"] = min_prob
    with torch.no_grad():
        out = m(d)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype, nhwc", [(torch.bfloat16, True), (torch.float32, False)])
def test_eval_forward_equals_the_loop(pkg, gpu, monkeypatch, dtype, nhwc):
    m = _small_model(pkg, gpu, dtype, nhwc)
    x = torch.rand(1, 3, 96, 128, generator=torch.Generator().manual_seed(3)).to(gpu)
    calls = []
    real = pkg.det_model.class_nms
    monkeypatch.setattr(pkg.det_model, "class_nms", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    on = _forward(pkg, monkeypatch, m, x, True)
    assert len(calls) == 1
    off = _forward(pkg, monkeypatch, m, x, False)
    assert len(calls) == 1
    for a, b in zip(on, off):
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    assert on[0].shape[0] > 0 and on[0].shape == (on[2].shape[0], 4) and on[1].dtype == torch.int and on[3].dtype == torch.long
    assert set(on[1].tolist()) <= set(range(1, 21)) and set(on[3].tolist()) == {0}
    on5, off5 = _forward(pkg, monkeypatch, m, x, True, 0.05), _forward(pkg, monkeypatch, m, x, False, 0.05)
    for a, b in zip(on5, off5):
        assert torch.equal(a, b)
    assert 0 < on5[0].shape[0] <= on[0].shape[0] and bool((on5[2] > 0.05).all())


def _split_and_loader(pkg, gpu, n=8):
    s = pkg.det_data.SyntheticDetSplit(n, seed=4, min_side=60, max_side=64)
    loader = pkg.det_data.DetDeviceLoader(s.images, s.boxes, s.classes, 1, gpu, False, 96., 128.)
    return s, loader


class _Oracle:
    """Speaks Model's eval protocol and returns each image's ground truth — the annotation's own boxes times the image's scale, moved
    by less than a third of a pixel — with confidences near 0.9, all different."""

    def __init__(self, split, loader, device):
        self.gt, self.ids, self.scale, self.device, self.k = split.ground_truth(), split.image_ids, loader.scale, device, 0
        self.rng = np.random.default_rng(0)

    def eval(self):
        return self

    def forward(self, d):
        classes, _, boxes = self.gt[self.ids[self.k]]
        g = len(classes)
        b = boxes.astype(np.float32) * self.scale[self.k] + self.rng.uniform(-0.3, 0.3, (g, 4)).astype(np.float32)
        p = (0.9 + 0.001 * (self.k * 8 + np.arange(g))).astype(np.float32)
        self.k += 1
        return (torch.from_numpy(b).to(self.device), torch.from_numpy(classes).to(torch.int), torch.from_numpy(p).to(self.device),
                torch.zeros(g, dtype=torch.long))


def test_evaluator_scores_the_ground_truth_one(pkg, gpu, tmp_path):
    s, loader = _split_and_loader(pkg, gpu)
    ev = pkg.det_eval.Evaluator(loader, (s.image_ids, s.ground_truth()), str(tmp_path))
    mean_ap, detail = ev.evaluate(_Oracle(s, loader, gpu))
    present = sorted(set(int(c) for cc in s.classes for c in cc))
    assert 0 < len(present) < 20
    for c in range(1, 21):
        name = pkg.det_eval.LABEL_TO_CATEGORY_DICT[c]
        assert "{:d}: {:s} AP = {:.4f}\n".format(c, name, 1.0 if c in present else 0.0) in detail
    assert mean_ap == pytest.approx(len(present) / 20, abs=1e-12)
    assert len([f for f in os.listdir(tmp_path) if f.startswith("comp3_det_test_")]) == 20
    with pytest.raises(ValueError, match="batch size"):
        pkg.det_eval.Evaluator(pkg.det_data.DetDeviceLoader(s.images, s.boxes, s.classes, 2, gpu, False, 96., 128.), (s.image_ids, s.ground_truth()))


def test_evaluator_is_the_same_with_the_tail_on_and_off(pkg, gpu, monkeypatch):
    s, loader = _split_and_loader(pkg, gpu)
    m = _small_model(pkg, gpu, torch.bfloat16, True)
    ev = pkg.det_eval.Evaluator(loader, (s.image_ids, s.ground_truth()))
    monkeypatch.setattr(pkg.det_model.Model, "CLASS_NMS", True)
    det_on = ev.detect(m)
    on = pkg.det_eval.evaluate(ev.ground_truth, *det_on)
    monkeypatch.setattr(pkg.det_model.Model, "CLASS_NMS", False)
    det_off = ev.detect(m)
    assert det_on == det_off and len(det_on[0]) > 0 and min(det_on[3]) > 0.05
    assert on == ev.evaluate(m) and len(on[1].splitlines()) == 20


def test_loader_takes_an_image_without_a_box_in_eval_mode(pkg, gpu):
    s = pkg.det_data.SyntheticDetSplit(3, seed=2, min_side=60, max_side=64)
    boxes, classes = list(s.boxes), list(s.classes)
    boxes[1], classes[1] = np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
    loader = pkg.det_data.DetDeviceLoader(s.images, boxes, classes, 1, gpu, False, 96., 128.)
    batches = list(loader)
    torch.cuda.synchronize()
    assert [tuple(b[1].shape) for b in batches] == [(1, len(boxes[0]), 4), (1, 0, 4), (1, len(boxes[2]), 4)]
    assert batches[1][0].shape[:2] == (1, 3) and bool(torch.isfinite(batches[1][0]).all())


def test_program_on_a_synthetic_split(pkg, gpu, tmp_path, capsys):
    entry = importlib.import_module("cv_a-fan_amd.eval")
    de = pkg.det_entry
    small = ["--image_min_side", "96", "--image_max_side", "128", "--anchor_sizes", "[64]", "--rpn_pre_nms_top_n", "200", "--rpn_post_nms_top_n", "64"]
    args = entry.get_full_argparser().parse_args(["-s", "voc2007", "-b", "resnet101"] + small + ["x.pth"])
    cfg = dict(de.DEFAULTS)
    cfg.update(pkg.det_eval.config(args))
    torch.manual_seed(2)
    model = de.build_model(args, cfg, 21)
    model.detection._proposal_class.weight.data.mul_(40.0)
    os.makedirs(tmp_path / "ckpt")
    path = de.save_checkpoint(str(tmp_path / "ckpt"), 7, model, torch.optim.SGD(model.parameters(), lr=0.001), cfg)
    del model
    before = pkg.ops.CALLS["det_batch_resize"]
    mean_ap, detail = entry.main(["-s", "voc2007", "-b", "resnet101", "--synthetic", "8"] + small + [path])
    assert pkg.ops.CALLS["det_batch_resize"] - before == 8 and pkg.ops.CALLS["vendor_conv"] == 0
    assert 0.0 <= mean_ap <= 1.0 and len(detail.splitlines()) == 20
    text = capsys.readouterr().out
    results = [d for d in os.listdir(tmp_path / "ckpt") if d.startswith("results-")]
    assert len(results) == 1 and "-model-7-" in results[0]
    files = os.listdir(tmp_path / "ckpt" / results[0])
    assert sorted(files) == sorted(["eval.log"] + [f"comp3_det_test_{pkg.det_eval.LABEL_TO_CATEGORY_DICT[c]}.txt" for c in range(1, 21)])
    log = open(tmp_path / "ckpt" / results[0] / "eval.log").read()
    for line in ("Found 8 samples", "Start evaluating with 1 GPU (1 batch per GPU)", "mean AP = {:.4f}".format(mean_ap), "1: aeroplane AP = ",
                 "20: tvmonitor AP = ", "RPN_POST_NMS_TOP_N = 64"):
        assert line in text and line in log, line
    assert "Load Weight:[" in text
    assert sum(os.path.getsize(tmp_path / "ckpt" / results[0] / f) for f in files if f.startswith("comp3")) > 0       # some detection passed 0.05
