"""Segmentation validation without a GPU: seg_eval.StreamSegMetrics against what the reference's own class computed
(tests/golden/seg_metrics.npz, written by tools/record_seg_metrics.py), main_seg_val's parser against the reference's names and
defaults (tests/golden/seg_args.json), its loud failure on a host, the C-ABI argument errors of afan_seg_confusion_upsampled, and
the float64 restatement of that kernel's definition (tests/seg_eval_refs.py) against torch on the CPU."""
import ctypes
import importlib
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_eval_refs as E
from conftest import GOLDEN, golden

SCALARS = ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU")
CASES = ("absent3", "ignore255", "pred_only", "single_class", "two_updates")


@pytest.fixture(scope="module")
def fx():
    return golden("seg_metrics")


def _same(got, ref):
    """rel 1e-12 (numpy's summation order is the only freedom: same formulas, same float64), NaN where the reference has NaN."""
    if math.isnan(ref):
        return math.isnan(got)
    return got == pytest.approx(ref, rel=1e-12, abs=0.0)


def _run(pkg, fx, name, as_tensor=False):
    m = pkg.seg_eval.StreamSegMetrics(int(fx[f"{name}/n_classes"]))
    for i in range(int(fx[f"{name}/n_updates"])):
        t, p = fx[f"{name}/targets_{i}"], fx[f"{name}/preds_{i}"]
        m.update(torch.from_numpy(t), torch.from_numpy(p)) if as_tensor else m.update(t, p)
    return m


def test_fixture_holds_the_cases(fx):
    assert tuple(fx["names"]) == CASES
    assert int(np.isnan(fx["absent3/class_iou"]).sum()) == 3 and int(fx["absent3/n_classes"]) == 21
    assert (fx["ignore255/targets_0"] == 255).any() and int(fx["two_updates/n_updates"]) == 2
    assert fx["pred_only/confusion"][:, 3].sum() > 0 and fx["pred_only/confusion"][3].sum() == 0
    assert np.count_nonzero(fx["single_class/confusion"]) == 1


@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("name", CASES)
def test_metrics_equal_the_references(pkg, fx, name, as_tensor):
    m = _run(pkg, fx, name, as_tensor)
    cm = m.confusion_matrix
    assert cm.dtype == np.float64 and np.array_equal(cm, fx[f"{name}/confusion"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # absent classes divide by zero: suppressed, not raised
        r = m.get_results()
    assert list(r) == list(SCALARS) + ["Class IoU"]
    for k, ref in zip(SCALARS, fx[f"{name}/scalars"]):
        assert _same(float(r[k]), float(ref)), k
    assert list(r["Class IoU"]) == list(range(m.n_classes))
    for c, ref in enumerate(fx[f"{name}/class_iou"]):
        assert _same(float(r["Class IoU"][c]), float(ref)), c
    assert m.to_str(r) == str(fx[f"{name}/to_str"])
    m.reset()
    assert not m.confusion_matrix.any()


def test_restated_scores_equal_the_references(fx):
    """tests/seg_eval_refs.scores is what the GPU tests compare validate() with: hold it to the fixture as well."""
    for name in CASES:
        got = E.scores(fx[f"{name}/confusion"])
        for g, ref in zip(got[:4], fx[f"{name}/scalars"]):
            assert _same(float(g), float(ref))
        assert all(_same(float(g), float(ref)) for g, ref in zip(got[4], fx[f"{name}/class_iou"]))
        calls = [(fx[f"{name}/targets_{i}"], fx[f"{name}/preds_{i}"]) for i in range(int(fx[f"{name}/n_updates"]))]
        assert np.array_equal(sum(E.fast_hist(int(fx[f"{name}/n_classes"]), t, p) for t, p in calls), fx[f"{name}/confusion"])


def test_update_logits_without_a_gpu_takes_torch(pkg):
    """CPU logits: no kernel applies, so torch's max(dim=1) on the resized logits and the host count."""
    g = torch.Generator().manual_seed(3)
    lo = torch.randint(-1, 2, (2, 5, 3, 4), generator=g).float()
    t = torch.randint(0, 5, (2, 12, 8), generator=g)
    t[0, :2] = 255
    m = pkg.seg_eval.StreamSegMetrics(5)
    m.update_logits(pkg.deeplab.LowResLogits(lo, (12, 8)), t)
    assert np.array_equal(m.confusion_matrix, E.confusion_upsampled(lo.numpy(), t.numpy()))
    with pytest.raises(ValueError, match="do not match"):
        m.update_logits(pkg.deeplab.LowResLogits(lo, (12, 9)), t)


# ---------------------------------------------------------------------------------------------------------------- main_seg_val
@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.main_seg_val")


def test_parser_defaults_equal_the_references(entry):
    ref = {a["dest"]: a for a in json.load(open(os.path.join(GOLDEN, "seg_args.json")))}
    table = [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in entry.get_argparser()._actions
             if a.dest != "help"]
    shared = ("ckpt", "model", "output_stride", "data_root", "year", "crop_val", "crop_size", "val_batch_size", "gpu_id", "random_seed")
    assert tuple(a["dest"] for a in table) == shared + entry.ADDITIONS == shared + ("dtype", "layout", "synthetic", "max_side")
    for a in table[:len(shared)]:
        assert a == ref[a["dest"]], a["dest"]
    o = entry.get_argparser().parse_args([])
    assert (o.dtype, o.layout, o.synthetic, o.max_side) == ("bf16", "nhwc", 0, 0)
    train = importlib.import_module("cv_a-fan_amd.main_aug_final").get_full_argparser().parse_args(["E"])
    assert all(getattr(o, k) == getattr(train, k) for k in entry.ADDITIONS)      # the additions default as the training entry's


def test_entry_fails_loudly_without_a_gpu(entry, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        entry.main(["--synthetic", "4", "--crop_val", "--crop_size", "33", "--max_side", "48"])
    assert not os.listdir(tmp_path)


def test_training_entry_names_the_new_program(pkg):
    train = importlib.import_module("cv_a-fan_amd.main_aug_final")
    with pytest.raises(NotImplementedError, match="main_seg_val.py"):
        train.main(["E", "--mix_layer", "11", "--pertub_idx_sd", "aspp", "--test_only", "ck.pth"])
    with pytest.raises(NotImplementedError, match="save_val_results"):
        pkg.seg_eval.validate(type("O", (), {"save_val_results": True})(), None, [], "cpu", pkg.seg_eval.StreamSegMetrics(3))


# --------------------------------------------------------------------------------------------- the kernel's C-ABI, on host pointers
def test_confusion_argument_errors_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    f = lib.afan_seg_confusion_upsampled
    assert f(p, p, 0, 21, 9, 9, 33, 33, p, None) == 0                     # empty batch: no launch
    assert f(None, None, 0, 21, 9, 9, 33, 33, None, None) == 0
    assert f(p, p, 1, 33, 9, 9, 33, 33, p, None) == -3                    # more than 32 classes
    assert f(p, p, 1, 0, 9, 9, 33, 33, p, None) == -3
    assert f(p, p, 1, 21, 34, 9, 33, 33, p, None) == -3                   # h > H
    assert f(p, p, 1, 21, 9, 34, 33, 33, p, None) == -3                   # w > W
    assert f(p, p, -1, 21, 9, 9, 33, 33, p, None) == -3
    assert f(None, p, 1, 21, 9, 9, 33, 33, p, None) == -4                 # AFAN_ENULL
    assert f(p, None, 1, 21, 9, 9, 33, 33, p, None) == -4
    assert f(p, p, 1, 21, 9, 9, 33, 33, None, None) == -4
    assert f(p, odd, 1, 21, 9, 9, 33, 33, p, None) == -2                  # AFAN_EALIGN: int64 labels and matrix
    assert f(p, p, 1, 21, 9, 9, 33, 33, odd, None) == -2
    # a ratio below 2 on a map of several tiles is a shape afan_ce2d_upsampled declines and this entry takes
    assert lib.afan_ce2d_upsampled_supported(21, 33, 33, 65, 65) == 0
    with pytest.raises(TypeError):
        pkg.ops.seg_confusion_upsampled(torch.zeros(1, 3, 2, 2), torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(9, dtype=torch.int64))


# ------------------------------------------------------------------------------- the float64 restatement against torch, exactly
# integer-valued logits in {-1, 0, 1} and dyadic ratios (weights in eighths): every interpolated value is a multiple of 1/64, exact in
# float32 and float64 alike, so ties are real ties and F.interpolate + max(dim=1) + bincount must agree with the restatement exactly
EXACT = [((1, 1), (4, 4)), ((3, 3), (12, 6)), ((5, 4), (20, 16)), ((9, 9), (18, 36)), ((7, 7), (7, 7))]


@pytest.mark.parametrize("src,dst", EXACT, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("c", [2, 21])
def test_restated_definition_equals_torch(src, dst, c):
    assert all(E.R.dyadic(a, b) for a, b in zip(src, dst))
    g = torch.Generator().manual_seed(11)
    lo = torch.randint(-1, 2, (2, c) + src, generator=g).float()
    t = torch.randint(0, c, (2,) + dst, generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = 255
    t[0, 0, 0], t[1, -1, -1] = c, -1                                   # out of range on both sides: skipped
    up = F.interpolate(lo, size=dst, mode="bilinear", align_corners=False)
    assert np.array_equal(up.double().numpy(), E.resize(lo.numpy(), *dst))
    pred = up.max(dim=1)[1]
    assert int((up == up.max(dim=1, keepdim=True)[0]).sum(1).max()) > 1   # ties exist
    assert np.array_equal(pred.numpy(), E.argmax_first(up.double().numpy()))
    m = (t >= 0) & (t < c)
    ref = torch.bincount(c * t[m] + pred[m], minlength=c * c).reshape(c, c).numpy()
    got = E.confusion_upsampled(lo.numpy(), t.numpy())
    assert got.dtype == np.int64 and np.array_equal(got, ref) and got.sum() == int(m.sum())


def test_restated_argmax_nan_rule_equals_torch():
    nan, inf = float("nan"), float("inf")
    px = torch.tensor([[1.0, nan, 3.0, nan], [2.0, 2.0, 1.0, 2.0], [-inf] * 4, [0.0, 5.0, nan, 9.0]])          # [pixel, class]
    x = px.t().reshape(1, 4, 2, 2)
    assert E.argmax_first(x.double().numpy()).reshape(-1).tolist() == x.max(dim=1)[1].reshape(-1).tolist() == [1, 0, 0, 2]
