"""frozen.block_plan keeps launch plans (ctypes pointers to weights, transposed weights and coefficient blocks) on the block, valid
as long as the stamp read from the live module attributes stands.  For both families — Detection's bottlenecks (stride-2 first
block, one stage node) and DeepLab's in eval mode (dilation 2, one node per block) — every way a tensor behind a plan can change
must show at the next forward: the output and the input gradient of the module with the warm cache equal, bit for bit, those of a
copy.deepcopy of it, whose cache is cold (__getstate__ drops it).  Before the one cache, Detection's validity key read the tensor
objects captured when the first plan was built: its case failed at the replaced buffer entry (the output did not move)."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _stage(pkg, family, gpu):
    """Two blocks, planes 64 behind 256 channels: projection, then identity."""
    torch.manual_seed(5)
    rs = pkg.resnet_s
    if family == "det":
        B, bn = pkg.det_model.Bottleneck, pkg.det_model.FrozenBatchNorm2d
        proj = nn.Sequential(rs.Conv2d(256, 256, kernel_size=1, stride=2, bias=False), bn(256))
        stage = nn.Sequential(B(256, 64, 2, proj), B(256, 64))
    else:
        B, bn = pkg.deeplab.Bottleneck, rs.BatchNorm2d
        proj = nn.Sequential(rs.Conv2d(256, 256, kernel_size=1, stride=1, bias=False), bn(256))
        stage = nn.Sequential(B(256, 64, 1, proj, 2), B(256, 64, dilation=2))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for m in stage.modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
                m.weight.copy_(torch.rand(c, generator=g) + 0.5)
                m.bias.copy_(torch.randn(c, generator=g) * 0.1)
            elif isinstance(m, rs.Conv2d):
                m.compute_dtype = torch.bfloat16
    stage = stage.to(gpu).eval()
    # one convolution reads an arena-style low-precision copy: kept at its address, rewritten when the weights move (edit c)
    c = stage[1].conv1
    c._arena_shadow = c.weight.detach().to(torch.bfloat16).contiguous(memory_format=CL)
    return stage


def _edits(pkg, stage):
    flags = pkg.resnet_s._Flags

    def running_var():
        stage[0].bn2.running_var.mul_(1.75)

    def weight_in_place():
        stage[0].conv2.weight.mul_(1.5)

    def weight_through_data():
        c = stage[1].conv1
        v = c.weight._version
        c.weight.data.mul_(1.5)
        c._arena_shadow.copy_(c.weight.detach())
        assert c.weight._version == v                     # no version saw it: only the epoch says so
        flags.weight_epoch += 1

    def buffer_replaced():
        bn = stage[1].bn1
        bn._buffers["running_mean"] = bn._buffers["running_mean"].clone()
        bn.running_mean.add_(0.25)

    return [running_var, weight_in_place, weight_through_data, buffer_replaced]


@pytest.mark.parametrize("family", ["det", "seg"])
def test_cached_plans_see_every_edit(pkg, gpu, monkeypatch, family):
    monkeypatch.setattr(pkg.deeplab, "FROZEN_EVAL", True)
    monkeypatch.setattr(pkg.deeplab, "COEF_CACHE", True)
    monkeypatch.setattr(pkg.det_model._FrozenBlockFn, "ON", True)
    monkeypatch.setattr(pkg.det_model._FrozenStageFn, "ON", True)
    monkeypatch.setattr(pkg.det_model._StageGraphs, "ON", False)
    monkeypatch.setattr(pkg.resnet_s._Flags, "weight_epoch", pkg.resnet_s._Flags.weight_epoch)       # (restored afterwards)
    calls = []
    fwd_plan = pkg.ops.frozen_bottleneck_fwd_plan
    monkeypatch.setattr(pkg.ops, "frozen_bottleneck_fwd_plan", lambda x_, p: (calls.append(p), fwd_plan(x_, p))[1])
    stage = _stage(pkg, family, gpu)
    g = torch.Generator().manual_seed(7)
    x = torch.relu(torch.randn(1, 256, 9, 9, generator=g)).to(gpu).bfloat16().contiguous(memory_format=CL)
    go = torch.randn(1, 256, 9 if family == "seg" else 5, 9 if family == "seg" else 5, generator=g).to(gpu).bfloat16().contiguous(memory_format=CL)

    def run(st):
        """-> (output, dx) as int16 bit patterns; every block must have taken the one-call form."""
        n = len(calls)
        xin = x.clone().requires_grad_(True)
        with pkg.resnet_s.dgrad_only():
            out = pkg.det_model._run_stage(st, xin) if family == "det" else st(xin)
            (dx,) = torch.autograd.grad(out, xin, go)
        assert len(calls) - n == len(st), "a block left the one-node form"
        return out.detach().view(torch.int16).clone(), dx.view(torch.int16).clone()

    last = run(stage)
    assert all(torch.equal(a, b) for a, b in zip(run(stage), last))                   # warm: the same bits again
    for edit in _edits(pkg, stage):
        with torch.no_grad():
            edit()
        got = run(stage)
        cold = copy.deepcopy(stage)
        assert all("_frozen_plans" not in b.__dict__ for b in cold)
        want = run(cold)
        assert not torch.equal(got[0], last[0]), edit.__name__                        # the edit matters ...
        assert torch.equal(got[0], want[0]), edit.__name__                            # ... and the cached plans saw it: output
        assert torch.equal(got[1], want[1]), edit.__name__                            # ... and input gradient
        last = got
