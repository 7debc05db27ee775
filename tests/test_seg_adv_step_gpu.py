"""seg_trainer.SegAdvTrainer (the iteration of the reference's Segmentation/main_advtrain.py:185-202) on the GPU, in the setting of
tests/test_seg_base_step_gpu.py: DeepLabv3+ ResNet-50, output stride 16, 2 x 3 x 65 x 65, 19 classes, labels with some 255, fp32 NCHW,
ASPP's dropout at p = 0 (two forwards that are compared value for value must not draw two masks)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import test_rand_start_ref as R
from conftest import assert_close_frac, golden
from test_seg_base_step_gpu import LR, WD, _batch, _model

pytestmark = pytest.mark.gpu

ATTACK = dict(steps_pgd=2, eps_pgd=2.0, gamma_pgd=0.5, clip=True)
SEED = 0x0BAD_5EED_1234_5678


def _hand_written(pkg, gpu, state, x, y, crit, **kw):
    """main_advtrain.py:185-201 on a copy of the pre-step state: adv_input in training mode, then forward, loss and backward on the
    result -> (copy, adversarial images, loss)."""
    copy = _model(pkg, gpu, state)
    pkg.deeplab.set_bn_momentum(copy.backbone, 0.01)
    pkg.ops.acc_reset(gpu)
    ce = pkg.deeplab.seg_criterion(crit)
    adv = pkg.seg_attack_algo.adv_input(x=x, criterion=ce, y=y, model=copy, steps=ATTACK["steps_pgd"], eps=ATTACK["eps_pgd"] / 255,
                                        gamma=ATTACK["gamma_pgd"] / 255, clip=ATTACK["clip"], **kw).detach()
    assert all(p.grad is None for p in copy.parameters())               # the attack passes compute no parameter gradient
    loss = ce(copy({"x": adv, "adv": None, "out_idx": 0, "flag": "clean", "low_res": True}), y)
    loss.backward()
    torch.cuda.synchronize()
    return copy, adv, loss


def _assert_step_equals(pkg, tr, model, r, copy, adv, loss):
    print(f"loss: step {float(r['loss']):.9g}, hand-written {float(loss):.9g}, |d| = {abs(float(r['loss']) - float(loss)):.3e}; "
          f"adversarial images: {int((r['adv_images'] != adv).sum())} elements differ")
    got, bad = dict(model.named_parameters()), []
    mom = {n: tr.arena.view(tr.arena.momentum_buf, i) for i, n in enumerate(tr.arena.names)}
    for n, p in copy.named_parameters():
        lr = 0.1 * LR if n.startswith("backbone.") else LR
        with torch.no_grad():
            d = p.grad + p * WD                                     # grad.add(param, alpha=weight_decay), rounded operation by operation
            want = p - d * lr                                       # first step: the momentum buffer is the gradient itself
        dv, dm = float((got[n].detach() - want).abs().max()), float((mom[n].reshape(want.shape) - d).abs().max())
        if dv != 0.0 or dm != 0.0:
            bad.append((n, dv, dm))
    print(f"parameters: {len(bad)} of {len(got)} tensors differ")
    assert torch.equal(r["adv_images"], adv)
    assert float(r["loss"]) == float(loss)
    assert not bad, bad[:5]
    tracked = 0
    for (k, v), (_, w) in zip(model.named_buffers(), copy.named_buffers()):
        assert torch.equal(v, w), f"BatchNorm buffer {k} differs"
        if k.endswith("num_batches_tracked"):
            tracked += 1
            assert int(v) == 3, k                                       # two attack passes and the training pass
    assert tracked > 50
    assert pkg.ops.CALLS["vendor_conv"] == 0


def test_one_eager_step_equals_the_hand_written_iteration(pkg, gpu):
    x, y = _batch(gpu)
    model = _model(pkg, gpu)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    crit = nn.CrossEntropyLoss(ignore_index=255, reduction="mean")
    tr = pkg.seg_trainer.SegAdvTrainer(model, crit, lr=LR, weight_decay=WD, total_itrs=100, use_graph=False, **ATTACK)
    assert [g["lr"] for g in tr.optimizer.param_groups] == [0.1 * LR, LR] and tr._small == ("loss",)
    r = tr.step(x, y)
    assert set(r) == {"loss", "adv_images", "noise_seed"} and r["noise_seed"] is None and tr._graph is None
    d = (r["adv_images"] - x).abs()
    assert float(d.max()) <= 2.0 / 255 + 1e-7 and float(d.max()) > 0 and float(r["adv_images"].min()) >= 0 and float(r["adv_images"].max()) <= 1
    _assert_step_equals(pkg, tr, model, r, *_hand_written(pkg, gpu, state, x, y, crit))


def test_one_eager_step_with_a_device_drawn_start(pkg, gpu):
    """The hand-written side re-derives the start from the seed word the step hands out: the generator is put back to it."""
    x, y = _batch(gpu)
    model = _model(pkg, gpu)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    crit = nn.CrossEntropyLoss(ignore_index=255, reduction="mean")
    tr = pkg.seg_trainer.SegAdvTrainer(model, crit, lr=LR, weight_decay=WD, total_itrs=100, use_graph=False, randinit=True,
                                       noise="device", **ATTACK)
    ns = pkg.ops.noise_state(gpu)
    ns.fill_(SEED)
    r = tr.step(x, y)
    seed = int(r["noise_seed"])
    assert seed == SEED and int(ns) == R.lcg(SEED)
    # the start itself, from the numpy generator: x + (2u - 1) eps through afan_axpy_noise, before any step
    u = torch.from_numpy(R.uniform(seed, tuple(x.shape))).to(gpu)
    start = pkg.ops.axpy_noise_(x.clone(), u, 2.0 / 255)
    # two sign steps of gamma, each projected back onto the ball the start lies in, then the clamp to [0, 1] (1-Lipschitz)
    assert float((r["adv_images"] - start.clamp(0, 1)).abs().max()) <= 2 * 0.5 / 255 + 1e-7
    assert float((start - x).abs().max()) > 1.9 / 255
    ns.fill_(seed)
    copy, adv, loss = _hand_written(pkg, gpu, state, x, y, crit, randinit=True, noise="device")
    _assert_step_equals(pkg, tr, model, r, copy, adv, loss)


def test_four_graph_steps_equal_four_eager_steps_with_a_random_start(pkg, gpu):
    """A random start no longer forbids the graph: drawn on the device, the whole iteration is captured, every replay draws a fresh
    start, and four replayed iterations are the four eager ones from the same generator word."""
    x, y = _batch(gpu)
    state, res = None, {}
    ns = pkg.ops.noise_state(gpu)
    for mode in ("eager", "graph"):
        model = _model(pkg, gpu, state)
        if state is None:
            state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        tr = pkg.seg_trainer.SegAdvTrainer(model, lr=LR, weight_decay=WD, total_itrs=100, use_graph=(mode == "graph"), graph_warmup=1,
                                           randinit=True, noise="device", **ATTACK)
        ns.fill_(SEED)
        losses, advs, seeds = [], [], []
        for _ in range(4):
            r = tr.step(x, y)
            losses.append(r["loss"].clone())
            advs.append(r["adv_images"].clone())
            seeds.append(int(r["noise_seed"]))
            tr.scheduler.step()
        tr.flush_guard()
        if mode == "graph":
            assert tr._graph is not None, tr._graph_failed
        else:
            assert tr._graph is None
        res[mode] = ([float(l) for l in losses], {k: v.detach().clone() for k, v in model.state_dict().items()}, advs, seeds)
    print("losses eager", res["eager"][0], "graph", res["graph"][0])
    worst = max((float((res["eager"][1][k].float() - res["graph"][1][k].float()).abs().max()), k) for k in state)
    print(f"state after 4 steps: largest |d| = {worst[0]:.3e} in {worst[1]}")
    want, s = [], SEED
    for _ in range(4):
        want.append(s)
        s = R.lcg(s)
    assert res["eager"][3] == res["graph"][3] == want and int(ns) == s
    assert res["eager"][0] == res["graph"][0] and all(np.isfinite(v) for v in res["eager"][0])
    assert worst[0] == 0.0
    for mode in ("eager", "graph"):
        advs = res[mode][2]
        assert not any(torch.equal(advs[a], advs[b]) for a in range(4) for b in range(a + 1, 4)), mode
    assert all(torch.equal(a, b) for a, b in zip(res["eager"][2], res["graph"][2]))
    assert pkg.ops.CALLS["vendor_conv"] == 0


def test_host_noise_stays_eager_and_draws_the_references_stream(pkg, gpu):
    x, y = _batch(gpu)
    model = _model(pkg, gpu)
    tr = pkg.seg_trainer.SegAdvTrainer(model, lr=LR, weight_decay=WD, total_itrs=100, use_graph=True, graph_warmup=0, randinit=True,
                                       noise="host", steps_pgd=0, eps_pgd=2.0, clip=True)
    ns0 = int(pkg.ops.noise_state(gpu))
    for k in range(2):
        torch.manual_seed(100 + k)
        r = tr.step(x, y)
        torch.manual_seed(100 + k)
        u = torch.rand(x.shape)                                         # attack_algo.py:90: the CPU generator's draw
        want = pkg.ops.axpy_noise_(x.clone(), u.to(gpu), 2.0 / 255).clamp_(0, 1)
        assert tr._graph is None and not tr.use_graph and r["noise_seed"] is None
        assert torch.equal(r["adv_images"], want), k
    assert int(pkg.ops.noise_state(gpu)) == ns0                         # the device generator was not asked
    with pytest.raises(ValueError):
        pkg.seg_trainer.SegAdvTrainer(model, noise="gpu")


def test_training_mode_adv_input_against_the_oracle(pkg, orc, gpu):
    """tests/test_seg_gpu.py::test_seg_adv_input_and_decoder_clip_error's network, inputs, settings and cap (2 % of the elements may
    differ — a gradient within rounding distance of zero flips a sign step — the rest within 1e-6), with both networks in TRAINING
    mode, as the PGD-training loop runs the attack.  The cap was set for eval mode; in training mode the oracle run against itself on
    the CPU in float32 and in float64 on these inputs differs in 0 of 6534 elements by more than 1e-6 (largest difference 6.0e-8),
    so the cap holds for the reference alone and is kept.  The network's running statistics after the two attack passes are compared
    too: every pass updates them."""
    g = golden("seg_step_aspp_k1")
    crit = nn.CrossEntropyLoss(ignore_index=255, reduction="mean")
    images, labels = torch.from_numpy(g["images"]).to(gpu), torch.from_numpy(g["labels"]).to(gpu)

    def net(device):
        torch.manual_seed(5)
        return orc.TinySegNet().train().to(device)

    mine, theirs = net(gpu), net(torch.device("cpu"))
    ref = orc.seg_adv_input(x=images.cpu(), criterion=crit, y=labels.cpu(), model=theirs, steps=2, eps=2.0 / 255, gamma=1.0 / 255, clip=True)
    got = pkg.seg_attack_algo.adv_input(x=images, criterion=crit, y=labels, model=mine, steps=2, eps=2.0 / 255, gamma=1.0 / 255, clip=True)
    assert mine.training and got.requires_grad and got.is_leaf
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert float((got.detach() - images).abs().max()) <= 2.0 / 255 + 1e-7
    d = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref.detach().numpy().astype(np.float64))
    print(f"training-mode adv_input: {(d > 1e-6).sum()} of {d.size} elements off by more than 1e-6 (share {(d > 1e-6).mean():.3e}), max {d.max():.3e}")
    assert_close_frac(got.detach().cpu().numpy(), ref.detach().numpy(), 0, 1e-6, 2e-2, "adv_input, training mode")
    for (k, v), (_, w) in zip(mine.named_buffers(), theirs.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(w) == 2, k
