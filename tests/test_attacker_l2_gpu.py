"""infer.Attacker(norm="l2"): the L2 attack (normalised-gradient steps projected onto the L2 ball, ops.pgd_step_l2_) inside the fused,
graph-replayed schedule equals the eager schedule bit for bit, equals the fp32 restatement of tests/pgd_l2_refs.py on the eager input
gradient, and stays inside the ball; norm="linf" is the attack without the argument.

The norm bound: the projected iterate is fl(x + fl(d s)) with s = fl(eps / nd) and nd within pgd_l2_refs.norm_rel(C_D) of the true
norm of d, so ||x_adv - x||_2 <= eps (1 + norm_rel(C_D)) (1 + u)^2 + u ||x_adv||_2 (the last sum's rounding, element by element);
a sample that was not projected had nd <= eps in the kernel's own sum, the same window.  The clamp to [0, 1] moves every element
towards x (x is inside [0, 1]), so it only shrinks the norm."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import pgd_l2_refs as L
from test_attacker_gpu import _batch, _model, _same

pytestmark = pytest.mark.gpu

EPS, GAMMA, STEPS = 0.5, 0.25, 3
PER = 3 * 32 * 32


def _norm_bound_holds(x_adv, x):
    xa, xc = x_adv.double().flatten(1), x.double().flatten(1)
    d = (xa - xc).norm(dim=1)
    lim = EPS * (1 + L.norm_rel(L.c_d(PER))) * (1 + L.U) ** 2 + L.U * xa.norm(dim=1)
    print("L2ATTACK norms", d.tolist(), "limit", lim.tolist())
    assert bool((d <= lim).all()), (d - lim).max().item()
    assert x_adv.min().item() >= 0.0 and x_adv.max().item() <= 1.0
    assert d.max().item() > 0.5 * EPS            # (three steps of eps / 2 reach the sphere: the projection ran)


@pytest.mark.parametrize("randinit", [False, True])
def test_l2_attacker_equals_the_eager_attack(pkg, gpu, randinit):
    m = _model(pkg, gpu, "resnet20s")
    at = pkg.infer.Attacker(m, nn.CrossEntropyLoss(), EPS, GAMMA, STEPS, randinit, norm="l2")
    assert at.fused and at.norm == "l2"
    at.refresh()
    x, y = _batch(gpu, 4, 11)
    torch.manual_seed(5)                                  # the host's generator draws the start's direction
    want = at.attack_eager(x, y, torch.randn(x.shape).to(gpu) if randinit else None)
    _norm_bound_holds(want[0], x)
    for sight in range(3):                                # fused, captured, replayed
        torch.manual_seed(5)
        with pkg.ops.conv_trace() as tr:
            got = at.attack(x, y)
        if sight == 2:
            assert tr.records == []                       # the replay enqueues nothing but the graph
        assert _same(got, want), sight
    if randinit:                                          # the start lies on the eps-sphere
        torch.manual_seed(5)
        _, x0 = pkg.pgd.start(x, EPS, True, norm="l2")
        d0 = (x0.double() - x.double()).flatten(1).norm(dim=1)
        assert bool(((d0 - EPS).abs() <= EPS * (L.norm_rel(L.c_g(PER)) + 4 * L.U) + L.U * x0.double().flatten(1).norm(dim=1)).all()), d0
        with pytest.raises(ValueError):
            pkg.pgd.start(x, EPS, True, noise="device", norm="l2")


def test_one_l2_step_is_the_restatement_on_the_eager_gradient(pkg, gpu):
    m = _model(pkg, gpu, "resnet20s")
    crit = nn.CrossEntropyLoss()
    at = pkg.infer.Attacker(m, crit, EPS, 2 * EPS, 1, False, norm="l2")           # one step of 2 eps: every sample is projected
    at.refresh()
    x, y = _batch(gpu, 4, 11)
    for _ in range(2):
        got = at.attack(x, y)[0]
    fc = pkg.resnet_s.fused_criterion(crit, m)
    grad = pkg.pgd.input_gradient(lambda t: fc(m(t, end_point=m.layer_number, start_point=0), y), x.clone().requires_grad_(True))
    grad = grad.detach().float().contiguous()
    _, gn, nd = pkg.ops.pgd_step_l2_(x.clone(), grad, 2 * EPS, x, EPS, False, None, want_norms=True)     # the kernel's own norms
    g64 = grad.double().flatten(1).norm(dim=1).cpu().numpy()
    assert (np.abs(gn.cpu().numpy() - g64) <= L.norm_window(g64, L.c_g(PER), PER)).all()
    flat = lambda t: t.flatten(1).cpu().numpy()
    want, _ = L.step_l2(flat(x), flat(grad), flat(x), 2 * EPS, EPS, True, gn.cpu().numpy(), nd.cpu().numpy())
    assert (nd.cpu().numpy() > 1.1 * EPS).all()
    want = np.clip(want, np.float32(0), np.float32(1))
    assert L.same_f32(flat(got), want) is None
    _norm_bound_holds(got, x)


def test_linf_is_the_attack_without_the_argument(pkg, gpu):
    m = _model(pkg, gpu, "resnet20s")
    x, y = _batch(gpu, 4, 11)
    outs = []
    for kw in ({}, {"norm": "linf"}):
        at = pkg.infer.Attacker(m, nn.CrossEntropyLoss(), 8 / 255, 2 / 255, STEPS, True, **kw)
        at.refresh()
        for _ in range(2):
            torch.manual_seed(5)
            got = at.attack(x, y)
        outs.append(got)
    assert _same(outs[1], outs[0])
    with pytest.raises(ValueError):
        pkg.infer.Attacker(m, nn.CrossEntropyLoss(), EPS, GAMMA, STEPS, norm="l1")
    with pytest.raises(ValueError):
        pkg.pgd.step(x.clone(), x, GAMMA, x, EPS, True, norm="l1")


def test_fp32_model_takes_the_eager_l2_attack(pkg, gpu):
    m = _model(pkg, gpu, "resnet20s", dtype=torch.float32, nhwc=False)
    at = pkg.infer.Attacker(m, nn.CrossEntropyLoss(), EPS, GAMMA, STEPS, norm="l2")
    assert not at.fused
    at.refresh()
    x, y = _batch(gpu, 2, 13)
    want = at.attack_eager(x, y)
    for _ in range(2):
        got = at.attack(x, y)
        assert len(got) == 3 and _same(got, want)
    _norm_bound_holds(got[0], x)
