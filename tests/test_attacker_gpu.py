"""infer.Attacker: image-space PGD on the eval-mode model with a fused forward and backward (one launch per convolution, one
hipGraph per batch shape) equals the same schedule through the model's eval-mode autograd bit for bit, stays inside the eps-ball
and the pixel range, and leaves the model alone."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

EPS, GAMMA, STEPS = 8 / 255, 2 / 255, 3


def _model(pkg, gpu, arch, dtype=torch.bfloat16, nhwc=True, seed=0):
    torch.manual_seed(seed)
    m = pkg.resnet_s.ARCHS[arch][0]()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                  # non-trivial running statistics
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.empty_like(mod.running_mean).uniform_(-0.2, 0.2, generator=g))
                mod.running_var.copy_(torch.empty_like(mod.running_var).uniform_(0.5, 2.0, generator=g))
                mod.weight.copy_(torch.empty_like(mod.weight).uniform_(0.5, 1.5, generator=g))
                mod.bias.copy_(torch.empty_like(mod.bias).uniform_(-0.1, 0.1, generator=g))
    m.set_compute_dtype(dtype)
    m.set_channels_last(nhwc).to(gpu)
    return m.eval()


def _batch(gpu, n, seed, side=32):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, side, side, generator=g).to(gpu), torch.randint(0, 10, (n,), generator=g).to(gpu)


def _bits(t):
    return t.float().contiguous().view(torch.int32)


def _same(got, want):
    return all(g.shape == w.shape and torch.equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _properties(x_adv, x):
    # exactly, in the images' own fp32: the projection clamps to [fl(x - eps), fl(x + eps)] (no tolerance added)
    assert bool((x_adv <= x + EPS).all()) and bool((x_adv >= x - EPS).all()), (x_adv - x).abs().max().item()
    assert x_adv.min().item() >= 0.0 and x_adv.max().item() <= 1.0
    assert (x_adv - x).abs().max().item() > 0


@pytest.mark.parametrize("randinit", [False, True])
@pytest.mark.parametrize("arch", ["resnet20s", "resnet18"])
def test_attacker_equals_the_eager_attack(pkg, gpu, arch, randinit):
    m = _model(pkg, gpu, arch)
    at = pkg.infer.Attacker(m, nn.CrossEntropyLoss(), EPS, GAMMA, STEPS, randinit)
    assert at.fused
    state = {k: v.clone() for k, v in m.state_dict().items()}
    at.refresh()
    x, y = _batch(gpu, 4, 11)
    torch.manual_seed(5)                                  # the host's generator draws the random start
    want = at.attack_eager(x, y)
    _properties(want[0], x)
    n_convs = sum(isinstance(mod, pkg.resnet_s.Conv2d) for mod in m.modules())
    for sight in range(3):                                # fused, captured, replayed
        torch.manual_seed(5)
        with pkg.ops.conv_trace() as tr:
            got = at.attack(x, y)
        if sight == 0:                                    # forward: one launch per convolution, STEPS + 1 times
            assert sum(r["op"] == "fwd" for r in tr.records) == (STEPS + 1) * n_convs
            names = {r["kernel"] for r in tr.records if r["op"] == "dgrad"}
            assert any(k.startswith("small_dgrad_aff") or k == "c64_dgrad_aff" for k in names), names
        if sight == 2:
            assert tr.records == []                       # the replay enqueues nothing but the graph
        assert _same(got, want), (arch, sight)
    # a second batch shape, and new weights behind refresh()
    x2, y2 = _batch(gpu, 3, 12)
    torch.manual_seed(6)
    want2 = at.attack_eager(x2, y2)
    torch.manual_seed(6)
    assert _same(at.attack(x2, y2), want2)
    after = m.state_dict()
    assert all(torch.equal(state[k], after[k]) for k in state)           # buffers and parameters bit-unchanged
    assert all(p.grad is None for p in m.parameters())
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.mul_(1.05)
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.add_(0.05)
    at.refresh()
    torch.manual_seed(7)
    want3 = at.attack_eager(x, y)
    assert not torch.equal(want3[0], want[0]) or not torch.equal(want3[1], want[1])
    torch.manual_seed(7)
    with pkg.ops.conv_trace() as tr:
        got3 = at.attack(x, y)                            # the first shape's graph, replayed on the refreshed buffers
    assert tr.records == []
    assert _same(got3, want3)
    _properties(got3[0], x)


def test_fp32_model_takes_the_eager_attack(pkg, gpu):
    m = _model(pkg, gpu, "resnet20s", dtype=torch.float32, nhwc=False)
    at = pkg.infer.Attacker(m, nn.CrossEntropyLoss(), EPS, GAMMA, STEPS)
    assert not at.fused
    at.refresh()
    x, y = _batch(gpu, 2, 13)
    want = at.attack_eager(x, y)
    for _ in range(2):
        got = at.attack(x, y)
        assert len(got) == 3 and _same(got, want)
    _properties(got[0], x)
    assert got[1].dim() == 0 and got[2].dim() == 0


def test_attack_needs_eval_mode(pkg, gpu):
    m = _model(pkg, gpu, "resnet20s")
    at = pkg.infer.Attacker(m, nn.CrossEntropyLoss(), EPS, GAMMA, 1)
    m.train()
    with pytest.raises(ValueError):
        at.attack(*_batch(gpu, 2, 1))
