"""Detection layer-wise SAT evaluation on the GPU: det_eval.SatLayerEvaluator, det_attack_algo.sat_layer_point(s), det_ops.PGD's `start`
and eval_sat_layers.py --synthetic end to end.

Small model and split of tests/test_det_rob_gpu.py: Faster-RCNN on ResNet101(layers=(1, 1, 1, 1)), bf16 channels-last, SyntheticDetSplit
of 4 images at 96 x 128.

  * steps = 0, sat_layer = 0, no mix gives Evaluator.detect's lists; sat_layer = 0 after two steps too, sat_layer = 4 does not;
  * steps = 2 --clip hands the eval forward a feature within eps / 255 (+ one fp32 ulp, then the bf16 cast) of the clean one, equal to a
    direct PGD + sat_layer_point from the same generator state;
  * SAT_POINTS_FUSED on and off give equal lists, with one / no sat_points launch per attacked image;
  * table=True gives, for each of the ten settings, the single-setting run's lists from the same generator state, with ONE attack per
    image (pgd.step calls are counted);
  * an image stripped of its boxes is scored from its clean feature and counted;
  * golden parity (tests/golden/det_sat_layers_tiny_{clip3,rand_clip3}.npz, tools/gen_det_sat_golden.py: the reference's PGD,
    get_sample_points and reversed mix_feature on oracle.TinyDetNet, fp32, the composed path): every stored step is redone from the
    golden's iterate and generator state through PGD(..., steps=1, start=...); signs and iterates are equal wherever |golden g| > thr
    = 2 x the reference's own fp32-against-float64 gradient difference, at most 1 % of a case's elements lie under thr; unmixed points
    equal pt/j bit for bit; mixed points satisfy |device - mixed64/j| <= max(4 * mdiff/j, 8 * 2^-24 * max |mixed64/j|), mdiff the
    reference's own fp32-against-float64 difference: the factor 4 and the floor of eight half-ulps of the largest value cover the six
    rounded operations per element and a different summation order over at most 32 channels; a swapped role, a biased variance or a
    missing eps moves values by 1e-3 or more.  Prints "DETSAT worst |device - mixed64| / bound" per case: 0.35 .. 0.46 on an
    MI355X (max |device g - golden g| 3.5e-10 .. 1.2e-9 per step against thr 4.4e-10 .. 1.8e-9; one element under thr in one case);
  * eval_sat_layers.main on a synthetic split, with and without --table: the results directory and its 21 files, the log lines,
    0 <= mean AP <= 1, no vendor convolution."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

EPS, GAMMA, STEPS, IDX = 2.0, 0.5, 2, 2


def _small_model(pkg, gpu):
    dm = pkg.det_model
    torch.manual_seed(11)
    m = dm.Model(dm.ResNet101(layers=(1, 1, 1, 1)), 21, rpn_post_nms_top_n=300)
    for b in m.modules():
        if isinstance(b, dm.Bottleneck):
            b.bn3.weight.data.mul_(0.2)
    m.detection._proposal_class.weight.data.mul_(40.0)
    return m.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(gpu).eval()


def _split_and_loader(pkg, gpu, strip=None):
    s = pkg.det_data.SyntheticDetSplit(4, seed=4, min_side=60, max_side=64)
    boxes, classes = list(s.boxes), list(s.classes)
    if strip is not None:
        boxes[strip], classes[strip] = np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
    loader = pkg.det_data.DetDeviceLoader(s.images, boxes, classes, 1, gpu, False, 96., 128.)
    return s, loader


@pytest.fixture(scope="module")
def model(pkg, gpu):
    return _small_model(pkg, gpu)


@pytest.fixture(scope="module")
def split(pkg, gpu):
    s, loader = _split_and_loader(pkg, gpu)
    return loader, (s.image_ids, s.ground_truth())


def _sat(pkg, split, **kw):
    loader, gt = split
    kw = dict(dict(steps=STEPS, eps=EPS, gamma=GAMMA, pertub_idx=IDX, clip=True), **kw)
    return pkg.det_eval.SatLayerEvaluator(loader, gt, **kw)


class _Capture:
    """Wraps model.forward: keeps the entering feature of every eval-mode call."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __enter__(self):
        fwd = self.model.forward

        def forward(d, *a, **k):
            if not self.model.training:
                assert d["flag"] == "tail" and d["out_idx"] == IDX and d["min_prob"] == 0.05
                self.seen.append(d["adv"].detach().clone())
            return fwd(d, *a, **k)
        self.model.forward = forward
        return self

    def __exit__(self, *exc):
        del self.model.forward
        return False


def test_steps_zero_and_sat_layer_zero_are_the_clean_evaluation(pkg, gpu, model, split):
    loader, gt = split
    clean = pkg.det_eval.Evaluator(loader, gt).detect(model)
    assert len(clean[0]) > 0
    ev = _sat(pkg, split, steps=0, sat_layer=0)
    assert ev.detect(model) == clean and (ev.attacked, ev.unattacked) == (4, 0) and not model.training
    ev = _sat(pkg, split, sat_layer=0)
    assert ev.detect(model) == clean
    assert _sat(pkg, split, sat_layer=4).detect(model) != clean
    assert not model.training


def test_two_clipped_steps_stay_within_the_ball(pkg, gpu, model, split):
    loader, gt = split
    ev = _sat(pkg, split, sat_layer=4)
    state = torch.get_rng_state()
    with _Capture(model) as cap:
        out = ev.detect(model)
    assert (ev.attacked, ev.unattacked) == (4, 0) and len(cap.seen) == 4 and len(out) == 4
    torch.set_rng_state(state)
    aa = pkg.det_attack_algo
    moved = 0.0
    for seen, (image, bb, lb, _) in zip(cap.seen, loader):
        with torch.enable_grad():
            fm = model.train().forward({"x": image, "adv": None, "out_idx": IDX, "flag": "head"}, bb, lb).detach()
            adv = aa.PGD(fm, image, y={"bb": bb, "lb": lb}, model=model, steps=STEPS, eps=EPS / 255, gamma=GAMMA / 255, idx=IDX, clip=True)
        assert adv.requires_grad and adv.dtype == torch.float32
        direct = aa.sat_layer_point(fm, adv, 4, False, torch.bfloat16)
        assert seen.dtype == torch.bfloat16 and seen.shape == fm.shape and torch.equal(seen, direct)
        c = fm.float()
        d = (seen.float() - c).abs()
        bound = EPS / 255 + c.abs() * 2.0 ** -23 + 2.0 ** -126          # the fp32 iterate: the ball + one ulp of the projection's bounds
        bound = bound + (c.abs() + bound) * 2.0 ** -8                   # then the bf16 cast of a value that large
        assert bool((d <= bound).all())
        moved = max(moved, float(d.max()))
    assert moved >= GAMMA / 255 * 0.5
    model.eval()


def test_switch_on_and_off_give_equal_lists(pkg, gpu, model, split, monkeypatch):
    aa = pkg.det_attack_algo
    state = torch.get_rng_state()
    out = {}
    for on in (True, False):
        monkeypatch.setattr(aa, "SAT_POINTS_FUSED", on)
        torch.set_rng_state(state)
        before = pkg.ops.CALLS["sat_points"]
        ev = _sat(pkg, split, sat_layer=2, mix=True)
        out[on] = ev.detect(model)
        assert pkg.ops.CALLS["sat_points"] - before == (ev.attacked if on else 0) and ev.attacked == 4
    assert out[True] == out[False] and len(out[True][0]) > 0


@pytest.fixture(scope="module")
def table_run(pkg, gpu, model, split):
    seen = []
    real = pkg.pgd.step
    pkg.pgd.step = lambda *a, **k: (seen.append(1), real(*a, **k))[1]
    try:
        state = torch.get_rng_state()
        before = pkg.ops.CALLS["sat_points"]
        ev = _sat(pkg, split, steps=1, table=True)
        rows = ev.detect(model)
        launches = pkg.ops.CALLS["sat_points"] - before
    finally:
        pkg.pgd.step = real
    assert (ev.attacked, ev.unattacked) == (4, 0)
    assert len(seen) == 1 * ev.attacked                       # ONE attack per image serves the ten settings
    assert launches == ev.attacked                            # ... and one launch its ten points
    assert list(rows) == list(pkg.det_eval.SAT_TABLE) and len(rows) == 10
    return state, rows


@pytest.mark.parametrize("sat_layer", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("mix", [False, True])
def test_table_rows_equal_the_single_setting_runs(pkg, gpu, model, split, table_run, sat_layer, mix):
    state, rows = table_run
    keep = torch.get_rng_state()
    torch.set_rng_state(state)
    single = _sat(pkg, split, steps=1, sat_layer=sat_layer, mix=mix).detect(model)
    torch.set_rng_state(keep)
    assert single == rows[(sat_layer, mix)] and len(single[0]) > 0
    if sat_layer >= 1:                                      # (point 0 re-normalised onto its own statistics is the clean map again in bf16)
        assert single != rows[(0, False)]


def test_table_evaluate_returns_one_metric_per_setting(pkg, gpu, model, split, tmp_path):
    loader, gt = split
    ev = pkg.det_eval.SatLayerEvaluator(loader, gt, str(tmp_path), steps=1, eps=EPS, gamma=GAMMA, pertub_idx=IDX, sat_layer=3, mix=True, clip=True,
                                        table=True)
    out = ev.evaluate(model)
    assert list(out) == list(pkg.det_eval.SAT_TABLE)
    assert all(0.0 <= ap <= 1.0 and len(detail.splitlines()) == 20 for ap, detail in out.values())
    assert len(os.listdir(tmp_path)) == 20                    # the files of the constructor's own setting


def test_an_image_without_boxes_is_scored_from_its_clean_feature(pkg, gpu, model, capsys):
    s, loader = _split_and_loader(pkg, gpu, strip=1)
    gt = (s.image_ids, s.ground_truth())
    ev = pkg.det_eval.SatLayerEvaluator(loader, gt, steps=STEPS, eps=EPS, gamma=GAMMA, pertub_idx=IDX, sat_layer=4, clip=True)
    with _Capture(model) as cap:
        ev.detect(model)
    assert (ev.attacked, ev.unattacked) == (3, 1)
    for k, (image, bb, lb, _) in enumerate(loader):
        with torch.enable_grad():
            fm = model.train().forward({"x": image, "adv": None, "out_idx": IDX, "flag": "head"}, bb, lb).detach()
        assert torch.equal(cap.seen[k].float(), fm.float()) == (k == 1)
    model.eval()
    assert "Scored 1 images without a non-difficult object from their clean feature" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ golden parity on TinyDetNet, fp32
def _tiny(pkg, orc, gpu):
    torch.manual_seed(11)
    model = orc.TinyDetNet(roi_align=pkg.det_ops.roi_align)
    return model.to(gpu).train()


@pytest.mark.parametrize("idx", [1, 2])
@pytest.mark.parametrize("case", ["clip3", "rand_clip3"])
def test_pgd_and_points_match_the_references(pkg, orc, gpu, case, idx, monkeypatch):
    g = golden("det_sat_layers_tiny_" + case)
    k = f"{case}_i{idx}/"
    s = json.loads(str(g[k + "settings"]))
    assert s["idx"] == idx and s["clip"] and s["steps"] == 3
    aa = pkg.det_attack_algo
    model = _tiny(pkg, orc, gpu)
    x, bb, lb, fm = (torch.from_numpy(g[k + n]).to(gpu) for n in ("x", "bboxes", "labels", "fm"))
    y = {"bb": bb, "lb": lb}
    with torch.no_grad():
        head = model.train().forward({"x": x, "adv": None, "out_idx": idx, "flag": "head"}, bb, lb)
    assert float((head - fm).abs().max()) <= 1e-5 * float(fm.abs().max())          # (the golden's own map is what is attacked below)
    iters, grads, thr, gdiff = g[k + "iter"], g[k + "grad"], g[k + "thr"], g[k + "gdiff"]
    assert len(iters) == s["steps"] + 1 and np.array_equal(thr, 2.0 * gdiff) and float(gdiff.min()) > 0
    pgd_kw = dict(y=y, model=model, eps=s["eps"], gamma=s["gamma"], idx=idx, randinit=s["randinit"], clip=s["clip"])
    torch.set_rng_state(torch.from_numpy(g[k + "rng0"]))
    x0 = aa.PGD(fm, x, steps=0, **pgd_kw)
    assert bool((x0.detach().cpu() - torch.from_numpy(iters[0])).abs().max() <= 2.0 ** -24)
    assert s["randinit"] == (not np.array_equal(iters[0], g[k + "fm"]))
    seen = []
    real = pkg.pgd.step
    monkeypatch.setattr(pkg.pgd, "step", lambda x_adv, grad, *a, **kw: (seen.append(grad.detach().clone()), real(x_adv, grad, *a, **kw))[1])
    under = 0
    for t in range(s["steps"]):
        torch.set_rng_state(torch.from_numpy(g[k + "rng"][t]))
        out = aa.PGD(fm, x, steps=1, start=torch.from_numpy(iters[t]).to(gpu), **pgd_kw)
        dev_g = seen[-1].float().cpu().numpy()
        big = np.abs(grads[t]) > thr[t]
        under += int((~big).sum())
        worst = float(np.abs(dev_g - grads[t]).max())
        print(f"DETSAT {case} idx {idx} step {t}: max |device g - golden g| = {worst:.3e}, thr = {thr[t]:.3e}, under thr: {int((~big).sum())}")
        assert np.array_equal(np.sign(dev_g)[big], np.sign(grads[t])[big])
        assert np.array_equal(out.detach().cpu().numpy()[big], iters[t + 1][big])
    assert len(seen) == s["steps"] and under <= 0.01 * grads.size
    assert np.array_equal(iters[-1], g[k + "adv"])
    # the points, from the golden's own adversarial map: the composed path (NCHW fp32), then the one launch on channels-last copies
    adv = torch.from_numpy(g[k + "adv"]).to(gpu)
    before = pkg.ops.CALLS["sat_points"]
    composed = aa.sat_layer_points(fm, adv, pkg.det_eval.SAT_TABLE, torch.float32, fused=True)
    assert pkg.ops.CALLS["sat_points"] == before
    fused = aa.sat_layer_points(fm.contiguous(memory_format=torch.channels_last), adv.contiguous(memory_format=torch.channels_last),
                                pkg.det_eval.SAT_TABLE, torch.float32, fused=True)
    assert pkg.ops.CALLS["sat_points"] == before + 1
    ratio = 0.0
    for (j, mix), pc, pf in zip(pkg.det_eval.SAT_TABLE, composed, fused):
        assert torch.equal(aa.sat_layer_point(fm, adv, j, mix), pc)
        for dev in (pc.cpu().numpy(), pf.cpu().numpy()):
            if not mix:
                assert np.array_equal(dev, g[k + f"pt/{j}"])
                continue
            m64, mdiff = g[k + f"mixed64/{j}"], float(g[k + f"mdiff/{j}"])
            bound = max(4.0 * mdiff, 8.0 * 2.0 ** -24 * float(np.abs(m64).max()))
            err = float(np.abs(dev.astype(np.float64) - m64).max())
            ratio = max(ratio, err / bound)
            if j >= 1:
                assert float(np.abs(g[k + f"mixed/{j}"] - g[k + f"pt/{j}"]).max()) >= 1e-3        # the mix is no identity here
    print(f"DETSAT {case} idx {idx}: worst |device - mixed64| / bound = {ratio:.4f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------- the program
@pytest.mark.parametrize("table", [False, True])
def test_program_on_a_synthetic_split(pkg, gpu, tmp_path, capsys, table):
    entry = importlib.import_module("cv_a-fan_amd.eval_sat_layers")
    de = pkg.det_entry
    small = ["--image_min_side", "96", "--image_max_side", "128", "--anchor_sizes", "[64]", "--rpn_pre_nms_top_n", "200", "--rpn_post_nms_top_n", "64"]
    args = entry.get_argparser().parse_args(["-s", "voc2007", "-b", "resnet101"] + small + ["x.pth"])
    cfg = dict(de.DEFAULTS)
    cfg.update(pkg.det_eval.config(args))
    torch.manual_seed(2)
    model = de.build_model(args, cfg, 21)
    model.detection._proposal_class.weight.data.mul_(40.0)
    os.makedirs(tmp_path / "ckpt")
    path = de.save_checkpoint(str(tmp_path / "ckpt"), 7, model, torch.optim.SGD(model.parameters(), lr=0.001), cfg)
    del model
    flags = ["--synthetic", "4", "--steps", "1", "--clip", "--pertub_idx", "3", "--sat_layer", "2", "--mix"] + (["--table"] if table else [])
    mean_ap, detail = entry.main(["-s", "voc2007", "-b", "resnet101"] + flags + small + [path])
    assert pkg.ops.CALLS["vendor_conv"] == 0
    assert 0.0 <= mean_ap <= 1.0 and len(detail.splitlines()) == 20
    text = capsys.readouterr().out
    assert text.startswith("steps" + "." * (80 - len("steps") - 1) + "1\n")             # print_args comes first
    assert "SAT LAYER:[2] MIX:[True]\n" in text
    results = [d for d in os.listdir(tmp_path / "ckpt") if d.startswith("results-")]
    assert len(results) == 1 and "-model-7-" in results[0]
    files = os.listdir(tmp_path / "ckpt" / results[0])
    assert len(files) == 21
    assert sorted(files) == sorted(["eval.log"] + [f"comp3_det_test_{pkg.det_eval.LABEL_TO_CATEGORY_DICT[c]}.txt" for c in range(1, 21)])
    log = open(tmp_path / "ckpt" / results[0] / "eval.log").read()
    lines = ["Found 4 samples", "Start evaluating Robustness with 1 GPU (1 batch per GPU)", "INFO     mean AP = {:.4f}".format(mean_ap),
             "Scored 0 images without a non-difficult object from their clean feature", "1: aeroplane AP = ", "20: tvmonitor AP = ", "\tsteps = 1",
             "\tpertub_idx = 3", "\tsat_layer = 2", "\tmix = True", "\ttable = {}".format(table)]
    if table:
        lines += ["SAT LAYER:[{}] MIX:[{}] mean AP = ".format(j, m) for j, m in pkg.det_eval.SAT_TABLE]
        assert "SAT LAYER:[2] MIX:[True] mean AP = {:.4f}".format(mean_ap) in log
    else:
        assert "SAT LAYER:[0] MIX:[False] mean AP" not in log
    for line in lines:
        assert line in text and line in log, line
    assert "Load Weight:[" in text
