"""seg_eval.pgd_validate (Segmentation/args.py:223-255) on the GPU: every validation batch attacked by image-space sign-PGD
(seg_attack_algo.adv_input), the predictions on the adversarial images scored in one launch per batch.  The expected matrix is built
by hand from the package's own pieces — adv_input, the forward, deeplab.interpolate, max(dim=1), seg_eval._fast_hist — and must be
equal exactly; without steps the matrix is validate()'s.  On the protocol-faithful stand-in network (fp32, both sides) the adversarial
images agree with the oracle's seg_adv_input under tests/test_seg_gpu.py's cap."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import assert_close_frac, golden

pytestmark = pytest.mark.gpu

SPLIT = dict(seed=1, min_side=36, max_side=48, classes=21)            # what --synthetic 4 --max_side 48 draws


def _opts(**kw):
    o = dict(steps_pgd=2, eps_pgd=8.0, gamma_pgd=2.0, randinit_pgd=False, clip_pgd=True, save_val_results=False)
    o.update(kw)
    return types.SimpleNamespace(**o)


@pytest.fixture(scope="module")
def model(pkg, gpu):
    torch.manual_seed(0)
    m = pkg.deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=21, output_stride=16)
    return m.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(gpu).eval()


@pytest.fixture(scope="module")
def loader(pkg, gpu):
    split = pkg.seg_data.SyntheticSegSplit(4, **SPLIT)
    return pkg.seg_data.SegDeviceLoader(split.images, split.labels, 2, gpu, False, 33, crop_val=True)


def _crit():
    return nn.CrossEntropyLoss(ignore_index=255, reduction="mean")


def _full(pkg, model, x):
    with torch.no_grad():
        out = model({"x": x, "adv": None, "out_idx": 0, "flag": "clean", "low_res": True})
        return pkg.deeplab.interpolate(out.logits, out.size)


def test_no_steps_is_validate(pkg, gpu, model, loader):
    m = pkg.seg_eval.StreamSegMetrics(21, gpu)
    pkg.seg_eval.validate(_opts(), model, loader, gpu, m)
    clean = m.confusion_matrix
    assert clean.sum() > 0
    score, samples = pkg.seg_eval.pgd_validate(_opts(steps_pgd=0), model, loader, gpu, m, _crit(), ret_samples_ids=[0])
    assert samples == [] and np.array_equal(m.confusion_matrix, clean)
    assert score["Mean IoU"] == m.get_results()["Mean IoU"]


def test_attacked_matrix_equals_the_hand_built_one(pkg, gpu, model, loader, monkeypatch):
    opts = _opts()
    eps = opts.eps_pgd / 255
    state = {k: v.clone() for k, v in model.state_dict().items()}
    crit = _crit()
    fused = pkg.deeplab.seg_criterion(crit)
    hist = np.zeros((21, 21), np.int64)
    for images, labels in loader:
        adv = pkg.seg_attack_algo.adv_input(x=images, criterion=fused, y=labels, model=model, steps=opts.steps_pgd, eps=eps,
                                            gamma=opts.gamma_pgd / 255, randinit=False, clip=True).detach()
        assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
        assert float((adv - images.float()).abs().max()) <= eps + 1e-7
        full_adv, full_clean = _full(pkg, model, adv), _full(pkg, model, images)
        l_adv, l_clean = float(crit(full_adv.float(), labels)), float(crit(full_clean.float(), labels))
        print(f"criterion clean {l_clean:.6f} adversarial {l_adv:.6f}")
        assert l_adv >= l_clean
        hist += pkg.seg_eval._fast_hist(21, labels.cpu().numpy().flatten(), full_adv.max(dim=1)[1].cpu().numpy().flatten())
    seen = []
    adv_input = pkg.seg_attack_algo.adv_input
    monkeypatch.setattr(pkg.seg_attack_algo, "adv_input", lambda **kw: (seen.append(kw), adv_input(**kw))[1])
    m = pkg.seg_eval.StreamSegMetrics(21, gpu)
    before = pkg.ops.CALLS["seg_confusion"]
    score, samples = pkg.seg_eval.pgd_validate(opts, model, loader, gpu, m, crit)
    assert samples == [] and pkg.ops.CALLS["seg_confusion"] - before == len(loader) == len(seen)
    assert all(kw["steps"] == 2 and kw["eps"] == eps and kw["gamma"] == 2.0 / 255 and kw["clip"] is True and kw["randinit"] is False
               and getattr(kw["criterion"], "fused", False) for kw in seen)
    assert np.array_equal(m.confusion_matrix, hist.astype(np.float64))
    assert set(score) == {"Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU", "Class IoU"}
    # the model is what it was: no buffer moved, no parameter got a gradient, still in eval mode
    now = model.state_dict()
    assert all(torch.equal(v, now[k]) for k, v in state.items())
    assert all(p.grad is None for p in model.parameters()) and model.training is False


def test_random_start_follows_the_host_generator(pkg, gpu, model, loader):
    mats = []
    for _ in range(2):
        torch.manual_seed(11)
        m = pkg.seg_eval.StreamSegMetrics(21, gpu)
        pkg.seg_eval.pgd_validate(_opts(randinit_pgd=True), model, loader, gpu, m, _crit())
        mats.append(m.confusion_matrix)
    assert mats[0].sum() > 0 and np.array_equal(mats[0], mats[1])


def test_adversarial_images_agree_with_the_oracle(pkg, orc, gpu, monkeypatch):
    """tests/test_seg_gpu.py::test_seg_adv_input_and_decoder_clip_error's inputs, settings, cap and tolerances, through pgd_validate."""
    g = golden("seg_step_aspp_k1")

    def net(dev):
        torch.manual_seed(5)
        return orc.TinySegNet().to(dev).eval()

    images, labels = torch.from_numpy(g["images"]), torch.from_numpy(g["labels"])
    crit = _crit()
    ref = orc.seg_adv_input(x=images, criterion=crit, y=labels, model=net(torch.device("cpu")), steps=2, eps=2.0 / 255, gamma=1.0 / 255,
                            clip=True)
    got = []
    adv_input = pkg.seg_attack_algo.adv_input
    monkeypatch.setattr(pkg.seg_attack_algo, "adv_input", lambda **kw: (got.append(adv_input(**kw)), got[-1])[1])
    m = pkg.seg_eval.StreamSegMetrics(5, gpu)
    pkg.seg_eval.pgd_validate(_opts(eps_pgd=2.0, gamma_pgd=1.0), net(gpu), [(images, labels)], gpu, m, crit)
    assert len(got) == 1 and m.confusion_matrix.sum() > 0
    adv = got[0].detach()
    assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
    assert float((adv.cpu() - images).abs().max()) <= 2.0 / 255 + 1e-7
    assert_close_frac(adv.cpu().numpy(), ref.detach().numpy(), 0, 1e-6, 2e-2, "adv_input")
