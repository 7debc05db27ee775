"""pgd.py, the sign-PGD core of every attack path: start / input_gradient / step / ascend on the smallest inputs that take each layout
branch, bit for bit against a plain-torch transcription of the reference loop (attack_algo.py:44-57: `x_adv + gamma * sign(g)`, then
`min(max(x_adv, x - eps), x + eps)`; gamma * +-1 is exact and the kernel clamps to [fl(x - eps), fl(x + eps)], so nothing rounds
differently), and the `grad0` contract of the callers through the public functions."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

GAMMA, EPS = 0.7 / 255, 1.0 / 255          # (two steps leave the eps-ball: the projection acts)


def _inputs(gpu):
    """name -> feature map on the GPU: every layout branch of start() and step()."""
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"f32_nchw": r(2, 4, 5, 3).to(gpu),
            "bf16_nhwc": r(2, 8, 3, 5).bfloat16().to(gpu).contiguous(memory_format=torch.channels_last),
            "n_c_1_1": r(2, 8, 1, 1).to(gpu).as_strided((2, 8, 1, 1), (8, 1, 8, 8)),          # (both layouts at once, channels-last strides)
            "view": r(2, 4, 5, 6).to(gpu)[..., ::2]}


CASES = ["f32_nchw", "bf16_nhwc", "n_c_1_1", "view"]


def _weights(x):
    """Fixed random w of x's shape with zeros, positives and negatives, in x_adv's layout (CPU copy beside it)."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(x.shape, generator=g)
    w[torch.rand(x.shape, generator=g) < 0.25] = 0.0
    assert (w == 0).any() and (w > 0).any() and (w < 0).any()
    return w


def _other_layout(t):
    """`t` in the dense layout it does not have."""
    nhwc = t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
    return t.contiguous() if nhwc else t.contiguous(memory_format=torch.channels_last)


def _reference(x, w, steps, clip):
    x = x.detach().float().cpu()
    x_adv = x.clone()
    for _ in range(steps):
        x_adv = x_adv + GAMMA * torch.sign(w)
        if clip:
            x_adv = torch.min(torch.max(x_adv, x - EPS), x + EPS)
    return x_adv


@pytest.mark.parametrize("case", CASES)
def test_start_layout_and_aliasing(pkg, gpu, case):
    x = _inputs(gpu)[case]
    before, layout = x.clone(), (x.dtype, x.stride(), x.data_ptr())
    x32, x_adv = pkg.pgd.start(x, EPS, False)
    for t in (x32, x_adv):
        assert t.dtype == torch.float32 and not t.requires_grad and t.shape == x.shape
        if case == "bf16_nhwc":
            assert t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
        elif case == "n_c_1_1":
            assert t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)
        else:
            assert t.is_contiguous()
    assert torch.equal(x32, before.float()) and torch.equal(x_adv, x32)
    assert x_adv.data_ptr() != x32.data_ptr() and x_adv.data_ptr() != x.data_ptr()
    assert torch.equal(x, before) and (x.dtype, x.stride(), x.data_ptr()) == layout
    with pytest.raises(pkg.AfanLibraryError):
        pkg.pgd.start(x.cpu(), EPS, False)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_loop_bit_for_bit(pkg, gpu, case, clip):
    pgd = pkg.pgd
    x = _inputs(gpu)[case]
    w_cpu = _weights(x)
    ref = _reference(x, w_cpu, 3, clip)
    # ascend: the gradient autograd hands back
    x32, x_adv = pgd.start(x, EPS, False)
    w = w_cpu.to(gpu)
    for _ in range(3):
        pgd.ascend(x_adv, lambda t: (t.float() * w).sum(), GAMMA, x32, EPS, clip)
    assert torch.equal(x_adv.cpu(), ref)
    # step: the gradient in the layout x_adv does not have, as fp32 and as bf16 (sign() survives the rounding)
    for cast in (lambda t: t, lambda t: t.bfloat16()):
        x32, x_adv = pgd.start(x, EPS, False)
        grad = cast(_other_layout(w))
        for _ in range(3):
            assert pgd.step(x_adv, grad, GAMMA, x32, EPS, clip) is None
        assert torch.equal(x_adv.cpu(), ref)
        assert torch.equal(x32, x.float())


@pytest.mark.parametrize("case", CASES)
def test_random_start_one_draw(pkg, gpu, case):
    x = _inputs(gpu)[case]
    torch.manual_seed(7)
    x32, x_adv = pkg.pgd.start(x, EPS, True)
    nxt = torch.rand(1)
    torch.manual_seed(7)
    u = torch.rand(x.shape)
    assert torch.equal(nxt, torch.rand(1))           # exactly one draw of exactly numel numbers
    ref = x.detach().float().cpu() + (2.0 * u - 1.0) * EPS
    assert torch.equal(x_adv.cpu(), ref) and torch.equal(x32, x.float())
    # a caller's own draw (host or device): the generator is not touched
    for own in (u, u.to(gpu)):
        state = torch.get_rng_state()
        _, x_adv2 = pkg.pgd.start(x, EPS, True, own)
        assert torch.equal(torch.get_rng_state(), state)
        assert torch.equal(x_adv2.cpu(), ref)
    state = torch.get_rng_state()
    pkg.pgd.start(x, EPS, False)
    assert torch.equal(torch.get_rng_state(), state)


def test_input_gradient_context_and_leaves(pkg, gpu):
    pgd, flags = pkg.pgd, pkg.resnet_s._Flags
    seen = []

    def loss_of(t):
        seen.append((flags.param_grads, torch.is_grad_enabled()))
        return (t * t).sum()
    leaf = torch.randn(2, 3, device=gpu).requires_grad_(True)
    assert flags.param_grads is True
    with torch.no_grad():
        g = pgd.input_gradient(loss_of, leaf)
        assert not torch.is_grad_enabled()
    assert seen == [(False, True)] and flags.param_grads is True and torch.is_grad_enabled()
    assert torch.equal(g, 2 * leaf.detach()) and leaf.grad is None

    def boom(t):
        raise RuntimeError("inside")
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="inside"):
            pgd.input_gradient(boom, leaf)
        assert not torch.is_grad_enabled()
    assert flags.param_grads is True
    # three leaves, one backward: each gradient depends on its own leaf only
    leaves = [torch.randn(2, 3, device=gpu).requires_grad_(True) for _ in range(3)]
    grads = pgd.input_gradient(lambda ts: sum(((k + 1) * t * t).sum() for k, t in enumerate(ts)), leaves)
    assert isinstance(grads, tuple) and len(grads) == 3
    for k, (t, g) in enumerate(zip(leaves, grads)):
        assert torch.equal(g, 2 * (k + 1) * t.detach())
    # a loss that is not a 0-dim fp32 scalar takes autograd's own root
    g = pgd.input_gradient(lambda t: (t.double() * 3).sum(), leaf)
    assert torch.equal(g, torch.full_like(g, 3.0))


def test_step_eps_none_and_norms(pkg, gpu):
    pgd = pkg.pgd
    x = _inputs(gpu)["bf16_nhwc"]
    w = _weights(x).to(gpu)
    outs = []
    for eps in (None, 0.0):
        x32, x_adv = pgd.start(x, EPS, False)
        pgd.step(x_adv, w, GAMMA, None, eps, False)
        outs.append(x_adv)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0].cpu(), _reference(x, w.cpu(), 1, False))
    with pytest.raises(ValueError):
        pgd.step(x_adv, w, GAMMA, x32, None, True)
    x32, x_adv = pgd.start(x, EPS, False)
    l2, linf = pgd.step(x_adv, w, GAMMA, x32, EPS, True, norms=True)
    r2, rinf = pkg.ops.perturb_norms(x_adv, x32)
    assert torch.equal(l2, r2) and torch.equal(linf, rinf)
    assert torch.equal(x_adv.cpu(), _reference(x, w.cpu(), 1, True))


class _SliceToy(nn.Module):
    """The Classification slice protocol `model(t, end_point=, start_point=)` on elementwise arithmetic (deterministic, and not linear
    in t: the gradient moves from step to step)."""

    def __init__(self, w, compute_dtype):
        super().__init__()
        self.w, self.compute_dtype, self.calls = w, compute_dtype, 0

    def forward(self, t, end_point=None, start_point=None):
        self.calls += 1
        assert t.dtype == self.compute_dtype
        return (t.float() * self.w).sum(dim=(2, 3))


class _DictToy(nn.Module):
    """The Segmentation dict protocol, flag 'tail': per-pixel logits from the perturbed feature."""

    def __init__(self, w):
        super().__init__()
        self.w, self.calls = w, 0

    def forward(self, d):
        self.calls += 1
        assert d["flag"] == "tail" and d["out_idx"] == 2
        return d["adv"].float() * self.w + d["low_level_feat"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grad0_classification(pkg, gpu, dtype):
    """attack_algo.PGD(grad0 = the true gradient at x) == the call without it, one model call less; fp32 and the bf16-shadow path."""
    x = _inputs(gpu)["bf16_nhwc"].float()        # (bf16-representable: the shadow of x is x)
    y = torch.tensor([1, 5], device=gpu)
    steps, kw = 3, dict(y=y, steps=3, gamma=GAMMA, start_idx=1, layer_number=2, eps=EPS, clip=True)
    crit = nn.CrossEntropyLoss()
    model = _SliceToy(_weights(x).to(gpu) * 3.0, dtype)
    plain = pkg.attack_algo.PGD(x, crit, model=model, **kw)
    assert model.calls == steps
    xin = x.to(dtype).requires_grad_(True)
    grad0 = torch.autograd.grad(crit(model(xin), y), xin)[0]
    model.calls = 0
    got = pkg.attack_algo.PGD(x, crit, model=model, grad0=grad0, **kw)
    assert model.calls == steps - 1
    assert torch.equal(got, plain) and got.requires_grad and got.is_leaf
    assert not torch.equal(plain.detach(), pkg.attack_algo.PGD(x, crit, model=model, **dict(kw, steps=1)).detach())
    if dtype == torch.bfloat16:
        assert torch.equal(got._afan_shadow, plain._afan_shadow) and torch.equal(got._afan_shadow, got.detach().bfloat16())
    with pytest.raises(ValueError):
        pkg.attack_algo.PGD(x, crit, model=model, grad0=grad0, **dict(kw, randinit=True))


def test_grad0_segmentation(pkg, gpu):
    x = _inputs(gpu)["bf16_nhwc"]
    labels = torch.randint(0, 8, (2, 3, 5), generator=torch.Generator().manual_seed(1)).to(gpu)
    low = torch.full((2, 8, 3, 5), 0.25, device=gpu)
    crit = nn.CrossEntropyLoss(ignore_index=255)
    model = _DictToy(_weights(x).to(gpu) * 3.0)
    steps, kw = 3, dict(y=labels, model=model, steps=3, eps=EPS, gamma=GAMMA, idx=2, clip=True)
    plain = pkg.seg_attack_algo.PGD(x, None, low, crit, **kw)
    assert model.calls == steps
    xin = x.float().requires_grad_(True)
    grad0 = torch.autograd.grad(crit(model({"adv": xin, "flag": "tail", "out_idx": 2, "low_level_feat": low}), labels), xin)[0]
    model.calls = 0
    got = pkg.seg_attack_algo.PGD(x, None, low, crit, grad0=_other_layout(grad0), **kw)
    assert model.calls == steps - 1
    assert torch.equal(got, plain) and got.requires_grad and got.is_leaf
    with pytest.raises(ValueError):
        pkg.seg_attack_algo.PGD(x, None, low, crit, grad0=grad0, **dict(kw, randinit=True))
