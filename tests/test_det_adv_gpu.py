"""det_attack_algo.det_adv_phases — one iteration of Detection/train_baseline_advtrain.py:75-93, PGD training — on the GPU.

(1) On oracle.TinyDetNet with the library's ROIAlign inside, against the reference's OWN loop body executed on the same model
(tools/gen_det_adv_golden.py: det_adv_tiny_plain.npz — one step, no start, no clip —, det_adv_tiny_rand_clip.npz — one step from a
random start, projected —, det_adv_tiny_rand_clip3.npz — three steps).  Bounds are those tests/test_det_final_gpu.py holds the same
model to, for the same reasons: losses rtol 1e-4; an adversarial image identical except where sign() flips on a gradient within
rounding of zero (at most 2 % of the pixels off by more than half a step; the fixture's own fp32-against-float64 share,
`ref_flip_share`, is asserted below half of that when it is written, and the fixture is asserted to have moved); updated weights
rtol 2e-3 / atol 2e-5, for the two one-step cases; the host generator ends where the reference's did.  The three-step case is also
redone STEP BY STEP through adv_input(start=..., steps=1, clamp=False), every step from the fixture's own iterate and generator state,
so that a flipped sign cannot compound, the last step once more with the clamp and under both settings of ADV_FUSED_CLAMP.

(2) On Faster-RCNN / ResNet-101 at 2 x 3 x 128 x 160 (det_frcnn_r101_align.npz's model and batch), bf16 channels-last: one
DetTrainer(phases="adv") step — finite losses, parameters that moved, an adversarial batch inside [0, 1] and inside the eps-ball;
ADV_FUSED_CLAMP on / off torch.equal in the adversarial batch, the losses, the arena gradients and the host generator's state, with
the call counters showing which export ended the attack; steps = 0 from a device-drawn start equal to clamp(x + (2u - 1) eps) with u
re-derived from out["noise_seed"] by the numpy Philox of tests/test_rand_start_ref.py; noise="device" leaving the host generator
where noise="host" without a random start leaves it."""
import json

import numpy as np
import pytest
import torch

from conftest import golden
from test_det_final_gpu import _check_weights, _tiny

pytestmark = pytest.mark.gpu

CASES = ["det_adv_tiny_plain", "det_adv_tiny_rand_clip", "det_adv_tiny_rand_clip3"]


def _off_share(got, want, gamma):
    return float((np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) > 0.5 * gamma / 255).mean())


class _switch:
    def __init__(self, pkg, on):
        self.da, self.on = pkg.det_attack_algo, bool(on)

    def __enter__(self):
        self.old, self.da.ADV_FUSED_CLAMP = self.da.ADV_FUSED_CLAMP, self.on

    def __exit__(self, *exc):
        self.da.ADV_FUSED_CLAMP = self.old
        return False


@pytest.mark.parametrize("fused", [False, True], ids=["composed", "fused"])
@pytest.mark.parametrize("case", CASES)
def test_iteration_matches_the_references_loop(pkg, orc, gpu, case, fused):
    g = golden(case)
    s = json.loads(str(g["settings"]))
    assert float(g["ref_flip_share"]) <= 1e-2
    model, opt, images, bboxes, labels = _tiny(pkg, orc, gpu, g)
    with _switch(pkg, fused):
        r = pkg.det_attack_algo.det_adv_step(model, opt, images, bboxes, labels, noise="host", **s)
    print(case, "losses", r["losses"].cpu().numpy(), "ref", g["losses"], "loss", float(r["loss"]), float(g["loss"]))
    assert r["losses"].shape == (4,) and "noise_seed" not in r
    np.testing.assert_allclose(r["losses"].cpu().numpy(), g["losses"], rtol=1e-4)
    assert abs(float(r["loss"]) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    adv = r["adv"].cpu().numpy()
    frac = _off_share(adv, g["adv_image_batch"], s["gamma"])
    print(case, "adversarial pixels off by more than half a step:", frac, "the reference's own fp32 / float64 share:", float(g["ref_flip_share"]))
    assert frac <= 2e-2, frac
    assert float(np.abs(g["adv_image_batch"] - g["images"]).max()) > 0.5 * s["gamma"] / 255       # (the fixture moved)
    assert adv.min() >= 0.0 and adv.max() <= 1.0 and not r["adv"].requires_grad
    if s["steps"] == 1:
        _check_weights(model, g)
    assert np.array_equal(torch.get_rng_state().numpy(), g["rng_state"])      # the same draws from the host generator


def test_three_steps_one_at_a_time(pkg, orc, gpu):
    g = golden("det_adv_tiny_rand_clip3")
    s = json.loads(str(g["settings"]))
    assert s["steps"] == 3 and s["randinit"] and s["clip"]
    model, _, images, bboxes, labels = _tiny(pkg, orc, gpu, g)
    da = pkg.det_attack_algo
    y = {"bb": bboxes, "lb": labels}
    kw = dict(x=images, y=y, model=model, eps=s["eps"] / 255, gamma=s["gamma"] / 255, randinit=True, clip=True, noise="host")
    # the start itself: the reference's draw, bit for bit (one launch of exact-by-operation arithmetic on the same u)
    x0 = da.adv_input(steps=0, clamp=False, **kw)
    np.testing.assert_array_equal(x0.detach().cpu().numpy(), g["iter0"])
    assert np.array_equal(torch.get_rng_state().numpy(), g["rng_pass0"])
    for k in range(3):
        torch.set_rng_state(torch.from_numpy(g[f"rng_pass{k}"]))
        start = torch.from_numpy(g[f"iter{k}"]).to(gpu)
        with _switch(pkg, k % 2 == 1):          # (without the clamp the switch changes nothing)
            x1 = da.adv_input(start=start, steps=1, clamp=False, **kw)
        assert x1.requires_grad and torch.equal(start, torch.from_numpy(g[f"iter{k}"]).to(gpu))     # the start is copied, not stepped
        frac = _off_share(x1.detach().cpu().numpy(), g[f"iter{k + 1}"], s["gamma"])
        print("step", k, "pixels off by more than half a step:", frac)
        assert frac <= 2e-2, (k, frac)
        assert float(np.abs(g[f"iter{k + 1}"] - g[f"iter{k}"]).max()) > 0.5 * s["gamma"] / 255
        assert np.array_equal(torch.get_rng_state().numpy(), g[f"rng_pass{k + 1}"] if k < 2 else g["rng_train"])
    assert (g["iter3"] < 0).any() and (g["iter3"] > 1).any()                  # the un-clamped iterate does leave [0, 1]
    last = {}
    for fused in (False, True):
        torch.set_rng_state(torch.from_numpy(g["rng_pass2"]))
        before = dict(pkg.ops.CALLS.other)
        with _switch(pkg, fused):
            last[fused] = da.adv_input(start=torch.from_numpy(g["iter2"]).to(gpu), steps=1, **kw).detach()
        ran = {k: pkg.ops.CALLS[k] - before[k] for k in ("pgd_step_clamp", "tensor_clamp")}
        assert ran == ({"pgd_step_clamp": 1, "tensor_clamp": 0} if fused else {"pgd_step_clamp": 0, "tensor_clamp": 1}), ran
        assert _off_share(last[fused].cpu().numpy(), g["adv_image_batch"], s["gamma"]) <= 2e-2
        assert float(last[fused].min()) >= 0.0 and float(last[fused].max()) <= 1.0
    assert torch.equal(last[False], last[True])


# ------------------------------------------------------------------------------------------------ Faster-RCNN / ResNet-101, B = 2
ADV = dict(steps=1, eps=2.0, gamma=0.5, randinit=True, clip=True, noise="host")
_runs = {}


def _run(pkg, gpu, fused, **settings):
    """One DetTrainer(phases="adv") step from the fixture's state and host seed 5; computed once per key."""
    key = (bool(fused),) + tuple(sorted(settings.items()))
    if key in _runs:
        return _runs[key]
    from test_det_model_gpu import _build, _golden_for
    g = _golden_for("align")
    images, bboxes, labels = (torch.from_numpy(g[k]).to(gpu) for k in ("images", "bboxes", "labels"))
    assert images.shape == (2, 3, 128, 160) and float(images.min()) >= 0.0 and float(images.max()) <= 1.0
    pkg.ops.noise_state(gpu)                     # (its first use seeds it from the host generator: not inside the measured draws)
    m = _build(pkg, g, gpu, torch.bfloat16, True, "align")
    tr = pkg.det_trainer.DetTrainer(m, phases="adv", adv=dict(ADV, **settings))
    p0 = tr.arena.param.clone()
    torch.manual_seed(5)
    before = dict(pkg.ops.CALLS.other)
    with _switch(pkg, fused):
        r = tr.step(images, bboxes, labels)
    torch.cuda.synchronize()
    res = {"losses": r["losses"].clone(), "loss": r["loss"].clone(), "adv": r["adv"].clone(), "grad": tr.arena.grad.clone(),
           "rng": torch.get_rng_state().clone(), "moved": float((tr.arena.param - p0).abs().max()),
           "finite": bool(torch.isfinite(tr.arena.param).all()), "images": images, "seed": r.get("noise_seed"),
           "ran": {k: pkg.ops.CALLS[k] - before[k] for k in ("pgd_step_clamp", "tensor_clamp")}}
    _runs[key] = res
    return res


@pytest.mark.parametrize("fused", [False, True], ids=["composed", "fused"])
def test_one_step_on_faster_rcnn(pkg, gpu, fused):
    r = _run(pkg, gpu, fused)
    assert r["losses"].shape == (4,) and torch.isfinite(r["losses"]).all() and np.isfinite(float(r["loss"]))
    assert r["finite"] and r["moved"] > 0 and float(r["grad"].abs().sum()) > 0
    assert pkg.ops.CALLS["vendor_conv"] == 0
    adv, x = r["adv"], r["images"]
    assert adv.dtype == torch.float32 and adv.shape == x.shape
    assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
    d = (adv.double() - x.double()).abs()
    # the ball's edges are fl32(x -+ fl32(eps)): within an ulp of a number below 1.01 of the real eps
    assert float(d.max()) <= 2.0 / 255 + 2.0 ** -23 and float(d.max()) > 0.5 / 255
    assert r["ran"] == ({"pgd_step_clamp": 1, "tensor_clamp": 0} if fused else {"pgd_step_clamp": 0, "tensor_clamp": 1}), r["ran"]


def test_fused_clamp_is_the_same_bits(pkg, gpu):
    on, off = _run(pkg, gpu, True), _run(pkg, gpu, False)
    for k in ("adv", "losses", "loss", "grad", "rng"):
        assert torch.equal(on[k], off[k]), k


@pytest.mark.parametrize("fused", [False, True], ids=["composed", "fused"])
def test_no_steps_from_a_device_drawn_start(pkg, gpu, fused):
    from test_rand_start_ref import uniform
    r = _run(pkg, gpu, fused, steps=0, noise="device")
    assert r["seed"] is not None and r["seed"].shape == (1,) and r["seed"].dtype == torch.int64
    x = r["images"].cpu().numpy()
    u = uniform(int(r["seed"].item()), x.shape).reshape(x.shape)
    t = (np.float32(2.0) * u).astype(np.float32)               # afan_pgd_rand_start's roundings, each operation on its own
    t = (t - np.float32(1.0)).astype(np.float32)
    t = (t * np.float32(2.0 / 255)).astype(np.float32)
    want = np.clip((x + t).astype(np.float32), np.float32(0.0), np.float32(1.0))
    np.testing.assert_array_equal(r["adv"].cpu().numpy(), want)
    assert (x + t < 0).any() and (x + t > 1).any()                # (the clamp had something to do)
    assert r["ran"] == ({"pgd_step_clamp": 1, "tensor_clamp": 0} if fused else {"pgd_step_clamp": 0, "tensor_clamp": 1}), r["ran"]
    assert r["finite"] and r["moved"] > 0 and torch.isfinite(r["losses"]).all()


def test_device_noise_leaves_the_host_generator_alone(pkg, gpu):
    dev, host_plain, host_rand = _run(pkg, gpu, False, noise="device"), _run(pkg, gpu, False, randinit=False), _run(pkg, gpu, False)
    assert dev["seed"] is not None and host_plain["seed"] is None and host_rand["seed"] is None
    assert torch.equal(dev["rng"], host_plain["rng"])            # the sampling draws only
    assert not torch.equal(dev["rng"], host_rand["rng"])         # (the host start reads 2 x 3 x 128 x 160 numbers more)
    assert not torch.equal(dev["adv"], host_rand["adv"])


def test_bad_settings_raise_in_the_constructor(pkg):
    dt = pkg.det_trainer
    with pytest.raises(ValueError, match="phases"):
        dt.DetTrainer(None, phases="pgd")
    with pytest.raises(ValueError, match="noise"):
        dt.DetTrainer(None, phases="adv", adv={"noise": "cpu"})
    with pytest.raises(ValueError, match="steps"):
        dt.DetTrainer(None, phases="adv", adv={"steps": -1})
