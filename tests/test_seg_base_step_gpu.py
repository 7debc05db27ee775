"""seg_trainer.SegBaseTrainer (the iteration of the reference's Segmentation/main_ori.py:158-163) on the GPU: DeepLabv3+ ResNet-50,
output stride 16, 2 x 3 x 65 x 65, 19 classes, labels with some 255, fp32 NCHW.  ASPP's dropout is set to p = 0 in every model
here: its mask comes from a device generator, and two forwards that are compared value for value must not draw two masks."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

LR, WD, MOM = 0.01, 1e-4, 0.9


def _model(pkg, gpu, state=None):
    torch.manual_seed(11)
    m = pkg.deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=19, output_stride=16)
    if state is not None:
        m.load_state_dict(state)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    m.set_compute_dtype(torch.float32)
    m.set_channels_last(False).to(gpu).train()
    return m


def _batch(gpu):
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.random((2, 3, 65, 65), dtype=np.float32)).to(gpu)
    y = rng.integers(0, 19, (2, 65, 65))
    y[rng.random(y.shape) < 0.05] = 255
    return x, torch.from_numpy(y.astype(np.int64)).to(gpu)


def test_one_eager_step_equals_the_hand_written_iteration(pkg, gpu):
    """The step's loss is seg_criterion of an independent forward on a copy made before the step, and its parameters and momentum
    buffers afterwards are the hand-written two-group SGD update (backbone at 0.1 x lr, weight decay, momentum) from that copy's
    gradients.  The same kernels run on both sides and tests/test_seg_gpu.py holds no tolerance for this comparison: exact equality."""
    ops = pkg.ops
    x, y = _batch(gpu)
    model = _model(pkg, gpu)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    crit = nn.CrossEntropyLoss(ignore_index=255, reduction="mean")
    tr = pkg.seg_trainer.SegBaseTrainer(model, crit, lr=LR, weight_decay=WD, total_itrs=100, use_graph=False)
    assert [g["lr"] for g in tr.optimizer.param_groups] == [0.1 * LR, LR]
    copy = _model(pkg, gpu, state)
    pkg.deeplab.set_bn_momentum(copy.backbone, 0.01)
    before = ops.CALLS["vendor_conv"]
    r = tr.step(x, y)
    assert set(r) == {"loss"} and tr._graph is None

    ops.acc_reset(gpu)
    ce = pkg.deeplab.seg_criterion(crit)
    out = copy({"x": x, "adv": None, "out_idx": 0, "flag": "clean", "low_res": True})
    loss = ce(out, y)
    loss.backward()
    torch.cuda.synchronize()
    print(f"loss: step {float(r['loss']):.9g}, hand-written {float(loss):.9g}, |d| = {abs(float(r['loss']) - float(loss)):.3e}")
    got, worst = dict(model.named_parameters()), (0.0, "")
    mom = {n: tr.arena.view(tr.arena.momentum_buf, i) for i, n in enumerate(tr.arena.names)}
    bad = []
    for n, p in copy.named_parameters():
        lr = 0.1 * LR if n.startswith("backbone.") else LR
        with torch.no_grad():
            d = p.grad + p * WD                                     # grad.add(param, alpha=weight_decay), rounded operation by operation
            want = p - d * lr                                       # first step: the momentum buffer is the gradient itself
        dv = float((got[n].detach() - want).abs().max())
        dm = float((mom[n].reshape(want.shape) - d).abs().max())
        worst = max(worst, (max(dv, dm), n))
        if dv != 0.0 or dm != 0.0:
            bad.append((n, dv, dm))
    print(f"parameters: {len(bad)} of {len(got)} tensors differ; largest |d| = {worst[0]:.3e} in {worst[1]}")
    for (k, v), (_, w) in zip(model.named_buffers(), copy.named_buffers()):
        assert torch.equal(v, w), f"BatchNorm buffer {k} differs"
    assert float(r["loss"]) == float(loss)
    assert not bad, bad[:5]
    assert ops.CALLS["vendor_conv"] == before == 0


def test_four_graph_steps_equal_four_eager_steps(pkg, gpu):
    """The captured iteration replays the eager one: two trainers from the same weights, four iterations with the schedule stepped,
    losses and final parameters equal (exact: the replay runs the launches the eager step runs)."""
    x, y = _batch(gpu)
    state, res = None, {}
    for mode in ("eager", "graph"):
        model = _model(pkg, gpu, state)
        if state is None:
            state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        tr = pkg.seg_trainer.SegBaseTrainer(model, lr=LR, weight_decay=WD, total_itrs=100, use_graph=(mode == "graph"), graph_warmup=1)
        losses = []
        for _ in range(4):
            losses.append(tr.step(x, y)["loss"].clone())
            tr.scheduler.step()
        tr.flush_guard()
        if mode == "graph":
            assert tr._graph is not None, tr._graph_failed
        else:
            assert tr._graph is None
        res[mode] = ([float(l) for l in losses], {k: v.detach().clone() for k, v in model.state_dict().items()})
    print("losses eager", res["eager"][0], "graph", res["graph"][0])
    worst = max((float((res["eager"][1][k].float() - res["graph"][1][k].float()).abs().max()), k) for k in state)
    print(f"state after 4 steps: largest |d| = {worst[0]:.3e} in {worst[1]}")
    assert res["eager"][0] == res["graph"][0]
    assert all(np.isfinite(v) for v in res["eager"][0]) and res["eager"][0][0] != res["eager"][0][3]
    assert worst[0] == 0.0
    assert pkg.ops.CALLS["vendor_conv"] == 0
