"""Eval-mode input gradients (resnet_s._BNEvalFn): a model in eval mode whose input requires a gradient runs its frozen
BatchNorms as autograd nodes (afan_bn_apply forward, afan_affine_relu_bwd backward), so attack_algo.PGD works on a trained
classifier from any start_idx — fp32 / NCHW against the CPU oracle, and without touching the model's state."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

# Tolerance of the eval-mode image gradient: twice the error of the fp32 / NCHW TRAIN-mode image gradient (a path that exists
# without the eval-mode node) against the CPU oracle on the same models and batch, max |g - g_ref| / max |g_ref|, taken by the
# test itself beside the eval-mode figure (both are printed; profiles/attack_README.md).


def _pair(pkg, orc, gpu, seed=0):
    """(oracle model on the CPU, product model in fp32 / NCHW on the GPU) with one state_dict and non-trivial running statistics."""
    torch.manual_seed(seed)
    ref = orc.resnet20s()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in ref.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.empty_like(mod.running_mean).uniform_(-0.2, 0.2, generator=g))
                mod.running_var.copy_(torch.empty_like(mod.running_var).uniform_(0.5, 2.0, generator=g))
                mod.weight.copy_(torch.empty_like(mod.weight).uniform_(0.5, 1.5, generator=g))
                mod.bias.copy_(torch.empty_like(mod.bias).uniform_(-0.1, 0.1, generator=g))
                mod.num_batches_tracked.fill_(5)
    m = pkg.resnet_s.resnet20()
    m.load_state_dict(ref.state_dict())
    m.set_compute_dtype(torch.float32).set_channels_last(False).to(gpu)
    return ref, m


def _batch(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, 3, 32, 32, generator=g), torch.randint(0, 10, (2,), generator=g)


def _input_grad(model, x, y):
    xin = x.detach().clone().requires_grad_(True)
    out = model(xin, end_point=len(model.sequential_model), start_point=0)
    loss = nn.CrossEntropyLoss()(out, y)
    return torch.autograd.grad(loss, xin)[0], out.detach()


def _rel_err(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


def test_eval_mode_input_gradient_matches_the_oracle(pkg, orc, gpu):
    ref, m = _pair(pkg, orc, gpu)
    x, y = _batch()
    ref.eval(), m.eval()
    g_ref, out_ref = _input_grad(ref, x, y)
    g, out = _input_grad(m, x.to(gpu), y.to(gpu))         # (raised NotImplementedError before the eval-mode node existed)
    assert g.shape == x.shape and g.dtype == torch.float32
    assert torch.allclose(out.cpu(), out_ref, rtol=1e-4, atol=1e-5)
    err = _rel_err(g, g_ref)
    # the yardstick: the train-mode gradient of the same models on the same batch (batch statistics; the running buffers it moves
    # are not read again)
    ref.train(), m.train()
    g_ref_t, _ = _input_grad(ref, x, y)
    g_t, _ = _input_grad(m, x.to(gpu), y.to(gpu))
    err_train = _rel_err(g_t, g_ref_t)
    print(f"eval-mode input gradient: rel err {err:.3e}; train-mode (existing path): {err_train:.3e}; bound {2 * err_train:.3e}")
    assert err_train > 0
    assert err <= 2.0 * err_train, (err, err_train)
    assert all(p.grad is None for p in m.parameters())     # no parameter gradients in eval mode


@pytest.mark.parametrize("dtype,nhwc", [(torch.float32, False), (torch.bfloat16, True)])
def test_forward_values_do_not_depend_on_requires_grad(pkg, orc, gpu, dtype, nhwc):
    _, m = _pair(pkg, orc, gpu)
    m.set_compute_dtype(dtype).set_channels_last(nhwc)
    m.eval()
    x = _batch()[0].to(gpu)
    with torch.no_grad():
        want = m(x, end_point=m.layer_number, start_point=0)
    got = m(x.clone().requires_grad_(True), end_point=m.layer_number, start_point=0)
    assert got.requires_grad
    assert torch.equal(got.detach().float().view(torch.int32), want.float().view(torch.int32))


@pytest.mark.parametrize("dtype,nhwc", [(torch.float32, False), (torch.bfloat16, True)])
@pytest.mark.parametrize("start", [0, None])
def test_pgd_on_an_eval_model_leaves_its_state_alone(pkg, orc, gpu, dtype, nhwc, start):
    _, m = _pair(pkg, orc, gpu)
    m.set_compute_dtype(dtype).set_channels_last(nhwc)
    m.eval()
    idx = pkg.resnet_s.ARCHS["resnet20s"][1] if start is None else start
    x, y = _batch()
    x, y = x.to(gpu), y.to(gpu)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        feat = x if idx == 0 else m(x, end_point=idx, start_point=0)
    eps = 8 / 255 if idx == 0 else 2.0
    adv = pkg.attack_algo.PGD(feat, nn.CrossEntropyLoss(), y=y, model=m, steps=2, gamma=eps / 4, start_idx=idx,
                              layer_number=m.layer_number, eps=eps, clip=True)
    torch.cuda.synchronize()
    assert adv.shape == feat.shape and bool(torch.isfinite(adv).all())
    a, f = adv.detach().float(), feat.float()
    assert (a - f).abs().max().item() > 0
    assert bool((a <= f + eps).all()) and bool((a >= f - eps).all())      # the projection's own fp32 bounds
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)          # running statistics, num_batches_tracked, parameters
    assert all(p.grad is None for p in m.parameters())
