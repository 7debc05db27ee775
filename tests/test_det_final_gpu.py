"""det_attack_algo.det_final_phases / det_base_phases — one iteration of Detection/train_aug_final.py:78-163 and
Detection/train_baseline.py:76-89 — on the GPU.

(1) On oracle.TinyDetNet with the library's ROIAlign inside, against the reference's OWN loop bodies executed on the same model
(tools/gen_det_final_golden.py: det_final_tiny_readme.npz — the README's setting —, det_final_tiny_mixnoise.npz — the deepest layer,
mix + noise on the ROI feature, all four losses in its attack, random starts —, det_base_tiny.npz).  Bounds and sign-flip accounting
are those of tests/test_det_gpu.py::test_detection_step_matches_reference_functions for the same model, for the same reasons: losses
rtol 1e-4; a one-step perturbation identical except where sign() flips on a gradient within rounding of zero (at most 2 % of the
elements off by more than half a step); adv_sd rtol / atol 1e-3; updated weights rtol 2e-3 / atol 2e-5.  The host generator ends
where the reference's did.

(2) On Faster-RCNN / ResNet-101 at 2 x 3 x 128 x 160 (det_frcnn_r101_align.npz's model and batch), bf16 channels-last: one step of each
iteration under DetTrainer — finite losses, parameters that moved — and the switches: det_model.BATCH_PROPOSALS on / off is the same
rows and the same draws (losses, adversarial tensors, arena gradients, final host-generator state torch.equal); BATCH_LAYER3 /
BATCH_ROI_HEAD on / off leave the losses bit-equal and the arena gradients within the bounds tests/test_det_model_gpu.py holds them
to (1e-5 / 2e-3 relative norm: fp32 summation order of the parameter gradients)."""
import json

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu


def _tiny(pkg, orc, gpu, g):
    torch.manual_seed(11)
    model = orc.TinyDetNet(roi_align=pkg.det_ops.roi_align)
    ck0 = np.array([[float(v.double().sum()), float(v.double().abs().sum())] for v in model.state_dict().values()])
    np.testing.assert_allclose(ck0, g["ck0"], rtol=1e-12)
    model.to(gpu).train()
    opt = torch.optim.SGD(model.parameters(), 0.01, momentum=0.9, weight_decay=5e-4)
    images = torch.rand(2, 3, 32, 32)                   # leaves the CPU generator where the reference's draws found it
    np.testing.assert_array_equal(images.numpy(), g["images"])
    return model, opt, images.to(gpu), torch.from_numpy(g["bboxes"]).to(gpu), torch.from_numpy(g["labels"]).to(gpu)


def _check_weights(model, g):
    sd = model.state_dict()
    keys = [k for k in g.files if k.startswith("sd1/")]
    assert len(keys) == 6
    for k in keys:
        np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), g[k], rtol=2e-3, atol=2e-5, err_msg=k)


@pytest.mark.parametrize("case", ["det_final_tiny_readme", "det_final_tiny_mixnoise"])
def test_final_iteration_matches_the_references_loop(pkg, orc, gpu, case):
    g = golden(case)
    s = json.loads(str(g["settings"]))
    model, opt, images, bboxes, labels = _tiny(pkg, orc, gpu, g)
    r = pkg.det_attack_algo.det_final_step(model, opt, images, bboxes, labels, **s)
    print(case, "losses", r["losses"].cpu().numpy(), "ref", g["losses"], "loss", float(r["loss"]), float(g["loss"]))
    assert r["losses"].shape == (6,)
    np.testing.assert_allclose(r["losses"].cpu().numpy(), g["losses"], rtol=1e-4)
    assert abs(float(r["loss"]) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    np.testing.assert_allclose(r["fm_se"].float().cpu().numpy(), g["fm_se"], rtol=1e-4, atol=1e-5)
    gamma = s["gamma_se"] / 255
    frac = float((np.abs(r["adv_se"].cpu().numpy() - g["adv_se"]) > 0.5 * gamma).mean())
    print(case, "adv_se elements off by more than half a step:", frac)
    assert frac <= 2e-2, frac
    assert float(np.abs(g["adv_se"] - g["fm_se"]).max()) > 0.5 * gamma         # (the fixture's perturbation is a step, not nothing)
    np.testing.assert_allclose(r["adv_sd"].cpu().numpy(), g["adv_sd"], rtol=1e-3, atol=1e-3)
    _check_weights(model, g)
    assert np.array_equal(torch.get_rng_state().numpy(), g["rng_state"])      # the same draws from the host generator


def test_baseline_iteration_matches_the_references_loop(pkg, orc, gpu):
    g = golden("det_base_tiny")
    model, opt, images, bboxes, labels = _tiny(pkg, orc, gpu, g)
    r = pkg.det_attack_algo.det_base_step(model, opt, images, bboxes, labels)
    np.testing.assert_allclose(r["losses"].cpu().numpy(), g["losses"], rtol=1e-4)
    assert abs(float(r["loss"]) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    _check_weights(model, g)
    assert np.array_equal(torch.get_rng_state().numpy(), g["rng_state"])


def test_clip_is_the_references_name_error(pkg, orc, gpu):
    g = golden("det_final_tiny_readme")
    model, opt, images, bboxes, labels = _tiny(pkg, orc, gpu, g)
    with pytest.raises(NameError, match="rpn_feature1"):
        pkg.det_attack_algo.det_final_step(model, opt, images, bboxes, labels, pertub_idx_se=2, mix_layer="0011", clip=True)
    with pytest.raises(ValueError, match="mix_layer"):
        pkg.det_attack_algo.det_final_step(model, opt, images, bboxes, labels, pertub_idx_se=2, mix_layer="01")
    with pytest.raises(ValueError, match="pertub_idx_se"):
        pkg.det_attack_algo.det_final_step(model, opt, images, bboxes, labels, pertub_idx_se=None, mix_layer="0011")


# ------------------------------------------------------------------------------------------------ Faster-RCNN / ResNet-101, B = 2
FINAL = dict(pertub_idx_se=2, mix_layer="0011", gamma_se=1.0, gamma_sd=0.1, sd_adv_loss_weight=0.3, only_roi_sd=True, mix_sd=True,
             noise_sd=0.01, randinit=True)
_runs = {}


def _run(pkg, gpu, phases, **off):
    """One DetTrainer step of `phases` from the fixture's state and host seed 5 with the named switches off; computed once per key."""
    key = (phases,) + tuple(sorted(off))
    if key in _runs:
        return _runs[key]
    from test_det_model_gpu import _build, _golden_for
    g = _golden_for("align")
    images, bboxes, labels = (torch.from_numpy(g[k]).to(gpu) for k in ("images", "bboxes", "labels"))
    assert images.shape == (2, 3, 128, 160)
    da, dm = pkg.det_attack_algo, pkg.det_model
    where = {"BATCH_PROPOSALS": dm, "BATCH_LAYER3": da, "BATCH_ROI_HEAD": da}
    old = {k: getattr(where[k], k) for k in where}
    calls = []
    real = pkg.det_ops.rpn_proposals
    try:
        for k in where:
            setattr(where[k], k, k not in off)
        dm.rpn_proposals = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
        m = _build(pkg, g, gpu, torch.bfloat16, True, "align")
        tr = pkg.det_trainer.DetTrainer(m, phases=phases, final=FINAL if phases == "final" else None)
        p0 = tr.arena.param.clone()
        torch.manual_seed(5)
        r = tr.step(images, bboxes, labels)
        torch.cuda.synchronize()
    finally:
        dm.rpn_proposals = real
        for k in where:
            setattr(where[k], k, old[k])
    res = {"losses": r["losses"].clone(), "loss": r["loss"].clone(), "grad": tr.arena.grad.clone(), "rng": torch.get_rng_state().clone(),
           "moved": float((tr.arena.param - p0).abs().max()), "finite": bool(torch.isfinite(tr.arena.param).all()), "batched_calls": len(calls)}
    for k in ("adv_se", "adv_sd", "fm_se"):
        if k in r:
            res[k] = r[k].clone()
    _runs[key] = res
    return res


@pytest.mark.parametrize("phases, n_losses", [("final", 6), ("base", 4)])
def test_one_step_on_faster_rcnn(pkg, gpu, phases, n_losses):
    r = _run(pkg, gpu, phases)
    assert r["losses"].shape == (n_losses,) and torch.isfinite(r["losses"]).all() and np.isfinite(float(r["loss"]))
    assert r["finite"] and r["moved"] > 0 and float(r["grad"].abs().sum()) > 0
    assert r["batched_calls"] > 0                                           # B = 2: the proposal layer took the whole batch
    assert pkg.ops.CALLS["vendor_conv"] == 0
    if phases == "final":
        d = (r["adv_se"].float() - r["fm_se"].float()).abs()
        assert float(d.max()) <= 2.0 / 255 + 1.0 / 255 + 1e-6 and float(d.max()) > 0      # a random start inside eps, one step of gamma_se


@pytest.mark.parametrize("phases", ["final", "base"])
def test_batched_proposals_are_the_same_rows_and_the_same_draws(pkg, gpu, phases):
    on, off = _run(pkg, gpu, phases), _run(pkg, gpu, phases, BATCH_PROPOSALS=0)
    assert on["batched_calls"] > 0 and off["batched_calls"] == 0
    for k in ("losses", "loss", "adv_se", "adv_sd", "grad", "rng"):
        if k in on:
            assert torch.equal(on[k], off[k]), k


@pytest.mark.parametrize("switch, bound", [("BATCH_LAYER3", 1e-5), ("BATCH_ROI_HEAD", 2e-3)])
def test_sharing_forms_of_the_final_iteration(pkg, gpu, switch, bound):
    on, off = _run(pkg, gpu, "final"), _run(pkg, gpu, "final", **{switch: 0})
    assert torch.equal(on["losses"], off["losses"]) and torch.equal(on["adv_se"], off["adv_se"]) and torch.equal(on["adv_sd"], off["adv_sd"])
    assert torch.equal(on["rng"], off["rng"])
    rel = float((on["grad"] - off["grad"]).norm() / off["grad"].norm())
    print(switch, "arena gradient, relative norm of the difference:", rel)
    assert rel < bound
