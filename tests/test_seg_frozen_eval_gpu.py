"""The eval-mode DeepLab on the frozen-BatchNorm forms (deeplab.FROZEN_EVAL): a Bottleneck as one node over the frozen bottleneck
sequencers (the block's dilation included), a conv -> BatchNorm (-> ReLU) pair as one node with a one-launch forward.  The switch
changes how the layers are issued, not what they compute: the low-resolution logits and the image gradient are bit-equal with the
switch on and off, the convolution count stays, the autograd graph shrinks, no parameter gets a gradient, no buffer moves, edits
of a BatchNorm's buffers or of a weight are seen at the next forward, and training mode, fp32 and NCHW never reach the frozen forms."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
                m.weight.copy_(torch.rand(c, generator=g) + 0.5)
                m.bias.copy_(torch.randn(c, generator=g) * 0.1)


@pytest.fixture(scope="module")
def models(pkg, gpu):
    out = {}
    for os_ in (16, 8):
        torch.manual_seed(os_)
        m = pkg.deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=21, output_stride=os_)
        _randomise_bn(m, os_)
        out[os_] = m.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(gpu).eval()
    return out


@pytest.fixture(scope="module")
def batch(gpu):
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 65, 65, generator=g)
    y = torch.randint(0, 21, (2, 65, 65), generator=g)
    y[torch.rand(2, 65, 65, generator=g) < 0.05] = 255
    return x.to(gpu), y.to(gpu)


def _nodes(fn):
    seen, stack = set(), [fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        stack.extend(n for n, _ in f.next_functions)
    return len(seen)


def _logits(model, x):
    with torch.no_grad():
        out = model({"x": x, "adv": None, "out_idx": 0, "flag": "clean", "low_res": True})
    return out.logits


def _passes(pkg, model, x, y):
    """-> (low-resolution logits, image gradient, convolution forwards of the gradient pass, autograd nodes of the gradient pass)"""
    crit = pkg.deeplab.seg_criterion(nn.CrossEntropyLoss(ignore_index=255, reduction="mean"))
    logits = _logits(model, x)
    xin = x.clone().requires_grad_(True)
    before = pkg.ops.CALLS["conv_fwd"]
    with pkg.resnet_s.dgrad_only():
        loss = crit(model({"x": xin, "adv": None, "out_idx": 0, "flag": "clean", "low_res": True}), y)
        fwd = pkg.ops.CALLS["conv_fwd"] - before
        nodes = _nodes(loss.grad_fn)
        grad = torch.autograd.grad(loss, xin, grad_outputs=pkg.ops.one(loss.device) if loss.dim() == 0 else None, only_inputs=True)[0]
    return logits, grad, fwd, nodes


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("os_", [16, 8])
def test_frozen_eval_equals_the_layer_by_layer_path(pkg, gpu, models, batch, monkeypatch, os_):
    model, (x, y) = models[os_], batch
    state = {k: v.clone() for k, v in model.state_dict().items()}
    monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", False)
    l_off, g_off, fwd_off, nodes_off = _passes(pkg, model, x, y)
    monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", True)
    blocks = []
    plan_fwd = pkg.ops.frozen_bottleneck_fwd_plan
    monkeypatch.setattr(pkg.ops, "frozen_bottleneck_fwd_plan", lambda x_, p: (blocks.append(p.dilation), plan_fwd(x_, p))[1])
    l_on, g_on, fwd_on, nodes_on = _passes(pkg, model, x, y)
    assert l_on.dtype == torch.float32 and tuple(l_on.shape[:2]) == (2, 21) and bool(torch.isfinite(l_on).all())
    assert float(g_on.abs().max()) > 0 and bool(torch.isfinite(g_on).all())
    assert torch.equal(_bits(l_on), _bits(l_off)), float((l_on - l_off).abs().max())
    assert torch.equal(_bits(g_on), _bits(g_off)), float((g_on - g_off).abs().max())
    assert fwd_on == fwd_off                                          # the same convolutions ...
    assert nodes_on < nodes_off, (nodes_on, nodes_off)                # ... behind fewer autograd nodes
    # every bottleneck of both passes took the one-node form, the atrous ones with their dilation — but layer2's first, whose input the
    # decoder reads too (deeplab.Bottleneck.shared_input: a bf16 sum of three gradients keeps its order)
    want = [1] * (3 + 3) + ([1] * 6 if os_ == 16 else [1] + [2] * 5) + ([1, 2, 2] if os_ == 16 else [2, 4, 4])
    assert blocks == want + want, blocks
    # no parameter gradient, no buffer moved
    assert all(p.grad is None for p in model.parameters())
    now = model.state_dict()
    assert all(torch.equal(v, now[k]) for k, v in state.items())


def test_frozen_eval_sees_edited_buffers_and_weights(pkg, gpu, models, batch, monkeypatch):
    """The stale-cache check: coefficient blocks and launch plans are kept between calls; an in-place edit of a running mean (inside a
    bottleneck, and of a stand-alone conv -> BatchNorm pair) and of a convolution weight must show at the next forward."""
    model, (x, _) = models[16], batch
    bb, head = model.backbone, model.classifier
    monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", True)
    first = _logits(model, x)
    saved = [t.clone() for t in (bb.layer3[0].bn2.running_mean, head.aspp.convs[1][1].running_mean, bb.layer4[1].conv2.weight)]
    try:
        with torch.no_grad():
            bb.layer3[0].bn2.running_mean.add_(0.25)
            head.aspp.convs[1][1].running_mean.sub_(0.25)
            bb.layer4[1].conv2.weight.mul_(1.5)
        on = _logits(model, x)
        monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", False)
        off = _logits(model, x)
        assert not torch.equal(on, first)                             # the edits matter ...
        assert torch.equal(_bits(on), _bits(off))                     # ... and the frozen forms saw them
    finally:
        with torch.no_grad():
            for t, s in zip((bb.layer3[0].bn2.running_mean, head.aspp.convs[1][1].running_mean, bb.layer4[1].conv2.weight), saved):
                t.copy_(s)
    monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", True)
    assert torch.equal(_bits(_logits(model, x)), _bits(first))
    # ... and so do running statistics moved by a training-mode forward in between (the kernels write them through their own pointers)
    model.train()
    try:
        with torch.no_grad():
            model({"x": x, "adv": None, "out_idx": 0, "flag": "clean"})
    finally:
        model.eval()
    on = _logits(model, x)
    monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", False)
    assert not torch.equal(on, first) and torch.equal(_bits(on), _bits(_logits(model, x)))


@pytest.mark.parametrize("config", ["train", "fp32", "nchw"])
def test_other_paths_never_reach_the_frozen_forms(pkg, gpu, models, batch, monkeypatch, config):
    """Training mode, fp32 and NCHW: the same result with the switch on and off, and the frozen forms' coefficient builder is never
    called with it on."""
    model, (x, _) = models[16], batch
    state = {k: v.clone() for k, v in model.state_dict().items()}
    drop = model.classifier.aspp.project[3]
    p_drop = drop.p

    def boom(bn, cache=True):
        raise AssertionError("a frozen form ran on the %s path" % config)

    try:
        if config == "train":
            model.train()
            drop.p = 0.0                                              # (no random draw: the two runs are comparable)
        elif config == "fp32":
            model.set_compute_dtype(torch.float32)
        else:
            model.set_channels_last(False)
        outs = []
        for on in (True, False):
            model.load_state_dict(state)
            monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", on)
            if on:
                monkeypatch.setattr(pkg.frozen, "bn_coefs", boom)
            with torch.no_grad():
                outs.append(model({"x": x, "adv": None, "out_idx": 0, "flag": "clean"}))
        assert bool(torch.isfinite(outs[0].float()).all())
        assert outs[0].dtype == outs[1].dtype and torch.equal(outs[0], outs[1])
    finally:
        drop.p = p_drop
        model.set_compute_dtype(torch.bfloat16).set_channels_last(True).eval()
        model.load_state_dict(state)
