"""The one-launch end of a tail pass: afan_head_ce / afan_loss_mean (classifier head, cross-entropy terms, the head's input gradient as
one row per image, the last BatchNorm's backward sums) and afan_bn_backward_acc_rows (the accumulator-form BatchNorm backward reading
that row), against the launches they replace: afan_head_forward -> afan_cross_entropy (x root) -> afan_head_backward -> afan_bn_backward.

  * logits, pooled, dlogits, the mean loss and v (expanded over the pixels) are the replaced launches' values BIT FOR BIT, for the
    root gradients 1 and 1/2; loss_row (which the replaced launches never store) is held to float64 within the roundings of
    m + logf(s) - l[t]: three fp32 operations at magnitude <= max|logit| + log K, i.e. 3 spacings of fp32 there.  Both instantiations
    of the kernel: with the accumulator block (the sums mode) and without it (the default launch, which takes no sums).
  * the two accumulator sums against a float64 sum of the same bf16 inputs, with the bounds tests/test_bn_pinned_gpu.py applies to the
    self-reducing accumulator form (C_DB / C_DW ["f32sum"], units of 2^-24 * sum |term|).
  * the row-reading apply against afan_bn_backward_acc on the materialised map, both given the SAME accumulator contents: bit for bit;
    the row-reading slab backward (afan_bn_backward_rows, what the trainer's route runs) against afan_bn_backward on the map: bit for bit.
  * one AfanTrainer step with the route on and off (AFAN_TAIL_END), eager and graph-replayed.
  * (no GPU) a plain m(x) never enters the new node; a head that cannot take it falls back.
"""
import itertools
import math

import pytest
import torch
import torch.nn as nn

from test_bn_pinned_gpu import C_DB, C_DW, U, acc_slots, ulp32

gpu_mark = pytest.mark.gpu
BF16 = torch.bfloat16
CL = torch.channels_last

# (N, HW, C, K, flavour): the issue's grid, whole; "big": logits of magnitude ~80; "dead": a channel whose out is zero everywhere
CASES = [(n, hw, c, k, "plain") for n, hw, c, k in itertools.product((3, 16), (1, 4, 16), (64, 512), (10, 16))]
CASES += [(16, 16, 512, 10, "big"), (3, 4, 64, 16, "big"), (16, 16, 512, 10, "dead"), (3, 16, 64, 16, "dead")]
# "loops": the two loops of head_ce_kernel behind its register-held operands — pixels p >= pg + 4 G (ragged, and at the HW cap of 64)
# and channels c >= 512 (G = 2 and G = 1) — and the HW cap at 64 channels
CASES += [(3, 25, 512, 10, "loops"), (3, 64, 512, 10, "loops"), (16, 64, 512, 16, "loops"), (3, 16, 1024, 10, "loops"),
          (3, 4, 1024, 16, "loops"), (3, 1, 2048, 10, "loops"), (3, 64, 64, 10, "loops")]
ROW_CASES = [c for c in CASES if c[1] > 1 and c[3] == 10 and c[4] != "loops"]


def case_id(c):
    return "n%d-hw%d-c%d-k%d-%s" % c


def _inputs(case, dev):
    n, hw, c, k, flavour = case
    h = {1: 1, 4: 2, 16: 4, 25: 5, 64: 8}[hw]
    gen = torch.Generator().manual_seed(1000 * n + 100 * hw + c + k + len(flavour))
    raw = (torch.randn(n, c, h, h, generator=gen) * 1.5 + 0.25)
    out = torch.relu(raw * 0.7 + torch.randn(n, c, h, h, generator=gen))
    if flavour == "dead":
        out[:, 5] = 0.0
        out[:, c - 1] = 0.0
    mean = raw.mean((0, 2, 3)) + 0.01 * torch.randn(c, generator=gen)
    invstd = 1.0 / raw.var((0, 2, 3), unbiased=False).add(1e-5).sqrt() if n * hw > 1 else torch.ones(c)
    gamma = torch.rand(c, generator=gen) + 0.5
    beta = 0.1 * torch.randn(c, generator=gen)
    stats = torch.stack([mean, invstd, invstd * gamma, beta - mean * invstd * gamma]).float().contiguous()
    weight = torch.randn(k, c, generator=gen) * (2.0 / math.sqrt(c))
    bias = 0.1 * torch.randn(k, generator=gen)
    if flavour == "big":
        bias = bias + 80.0 * torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(k)])
    target = torch.randint(0, k, (n,), generator=gen)
    target[0], target[-1] = 0, k - 1
    to_cl = lambda t: t.to(dev).to(BF16).contiguous(memory_format=CL)
    return dict(out=to_cl(out), raw=to_cl(raw), stats=stats.to(dev), weight=weight.to(dev).contiguous(), bias=bias.to(dev),
                target=target.to(dev), bn_w=gamma.to(dev), bn_b=beta.to(dev))


def _chain(ops, d, root):
    """The launches the new one replaces."""
    logits, pooled = ops.head_forward(d["out"], d["weight"], d["bias"])
    loss, dlogits = ops.cross_entropy(logits, d["target"])
    if root != 1.0:
        dlogits = dlogits * torch.full((), root, dtype=torch.float32, device=dlogits.device)
    dx = ops.head_backward(dlogits, d["weight"], pooled, d["out"], True)
    return logits, pooled, loss, dlogits, dx


def _head_ce(pkg, d, root, with_acc=True):
    ops = pkg.ops
    c = d["out"].shape[1]
    acc = torch.zeros(ops.acc_block_doubles(c), dtype=torch.float64, device=d["out"].device) if with_acc else None
    logits, pooled, loss_row, dlogits, v = ops.head_ce(d["out"], d["raw"], d["stats"], d["weight"], d["bias"], d["target"], root, acc)
    return logits, pooled, loss_row, dlogits, v, acc


@gpu_mark
@pytest.mark.parametrize("root", [1.0, 0.5])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_head_ce_equals_the_launches_it_replaces(pkg, gpu, case, root):
    """With the accumulator block: the sums mode's instantiation of the kernel."""
    _check_head_ce(pkg, gpu, case, root, True)


@gpu_mark
@pytest.mark.parametrize("root", [1.0, 0.5])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_head_ce_without_the_sums_equals_the_launches_it_replaces(pkg, gpu, case, root):
    """acc = None, the default launch: the same five bit-equalities and loss_row bound (the parameter over acc given / None is two
    test functions, so that the cases with acc keep the ids they had)."""
    _check_head_ce(pkg, gpu, case, root, False)


def _check_head_ce(pkg, gpu, case, root, with_acc):
    ops = pkg.ops
    n, hw, c, k, flavour = case
    d = _inputs(case, gpu)
    r_logits, r_pooled, r_loss, r_dlogits, r_dx = _chain(ops, d, root)
    logits, pooled, loss_row, dlogits, v, acc = _head_ce(pkg, d, root, with_acc)
    loss = ops.loss_mean(loss_row)
    torch.cuda.synchronize()
    if flavour == "big":
        assert float(r_logits.abs().max()) > 70.0
    assert torch.equal(logits, r_logits), "logits"
    assert torch.equal(pooled, r_pooled), "pooled"
    assert torch.equal(dlogits, r_dlogits), "dlogits (x root)"
    assert torch.equal(loss.reshape(1), r_loss.reshape(1)), f"mean loss {float(loss)} vs {float(r_loss)}"
    assert torch.equal(v.view(n, c, 1, 1).expand_as(r_dx), r_dx), "v expanded over the pixels vs head_backward's dx"
    # loss_row against float64 of the same logits
    l64 = r_logits.double()
    row64 = torch.logsumexp(l64, 1) - l64.gather(1, d["target"][:, None])[:, 0]
    tol = 3.0 * ulp32(l64.abs().max(1).values + math.log(k))
    worst = float(((loss_row.double() - row64).abs() / tol).max())
    print(f"TAILEND loss_row {worst:.3f} of the bound {case_id(case)} root {root}")
    assert worst <= 1.0, "loss_row off float64"
    if acc is None:         # the default launch: no sums taken
        return
    # the two sums against float64 of the same bf16 inputs
    g = torch.where(d["out"].double() > 0, v.double().view(n, c, 1, 1).expand(n, c, *d["out"].shape[2:]), torch.zeros((), dtype=torch.float64, device=gpu))
    xm = d["raw"].double() - d["stats"][0].double().view(1, c, 1, 1)
    sg, sgx = g.sum((0, 2, 3)), (g * xm).sum((0, 2, 3))
    s_g, s_gx = g.abs().sum((0, 2, 3)), (g * xm).abs().sum((0, 2, 3))
    ns, _ = acc_slots(pkg._lib.load(), c)
    got = acc[:2 * ns * c].view(ns, 2, c).sum(0)
    rg = float(((got[0] - sg).abs() / (U * s_g).clamp_min(1e-300)).max())
    rgx = float(((got[1] - sgx).abs() / (U * s_gx).clamp_min(1e-300)).max())
    print(f"TAILEND sum_g {rg:.3f} (bound {C_DB['f32sum']:.2f}) sum_gx {rgx:.3f} (bound {C_DW['f32sum']:.2f}) {case_id(case)}")
    assert rg <= C_DB["f32sum"] and rgx <= C_DW["f32sum"]
    dead = s_g == 0
    if flavour == "dead":
        assert int(dead.sum()) >= 2
    assert bool((got[:, dead] == 0).all()), "an empty mask must leave the sums zero"


@gpu_mark
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", ROW_CASES, ids=case_id)
def test_row_reading_apply_equals_the_map_reading_one(pkg, gpu, case, accumulate):
    ops = pkg.ops
    n, hw, c, k, _ = case
    d = _inputs(case, gpu)
    *_, v, acc = _head_ce(pkg, d, 0.5)
    rows = v.view(n, c, 1, 1).expand_as(d["out"])
    assert ops.is_row_broadcast(rows, d["raw"])
    res = []
    for dy in (rows.contiguous(memory_format=CL), rows):
        dwb = torch.full((2, c), 3.0 if accumulate else float("nan"), dtype=torch.float32, device=gpu)
        part = ops.ConvStats(None, 0, None, acc.clone())
        dx, dres = ops.bn_backward(dy, d["raw"], d["out"], d["stats"], d["bn_w"], d["bn_b"], True, True, dwb[0], dwb[1], accumulate,
                                   partials=part)
        res.append((dx, dres, dwb))
    torch.cuda.synchronize()
    for name, a, b in zip(("d_raw", "dres", "dweight | dbias"), res[0], res[1]):
        assert torch.equal(a, b), name
    assert not bool(torch.isnan(res[1][2]).any())


@gpu_mark
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", ROW_CASES, ids=case_id)
def test_row_reading_slab_backward_equals_the_map_reading_one(pkg, gpu, case, accumulate):
    """afan_bn_backward_rows against afan_bn_backward on the written-out map: same launches, same order, every output bit for bit."""
    ops = pkg.ops
    n, hw, c, k, _ = case
    d = _inputs(case, gpu)
    v = _head_ce(pkg, d, 0.5)[4]
    rows = v.view(n, c, 1, 1).expand_as(d["out"])
    res = []
    for dy in (rows.contiguous(memory_format=CL), rows):
        dwb = torch.full((2, c), 3.0 if accumulate else float("nan"), dtype=torch.float32, device=gpu)
        dx, dres = ops.bn_backward(dy, d["raw"], d["out"], d["stats"], d["bn_w"], d["bn_b"], True, True, dwb[0], dwb[1], accumulate)
        res.append((dx, dres, dwb))
    torch.cuda.synchronize()
    for name, a, b in zip(("d_raw", "dres", "dweight | dbias"), res[0], res[1]):
        assert torch.equal(a, b), name
    assert not bool(torch.isnan(res[1][2]).any())


# ---- one trainer step, route on / off -----------------------------------------------------------------------------------------------
_STEP = {}


def _one_step(pkg, gpu, graph, route, monkeypatch, sums=False):
    torch.manual_seed(7)
    model = pkg.resnet_s.resnet18()
    model.set_compute_dtype(BF16).set_channels_last(True).to(gpu).train()
    gen = torch.Generator().manual_seed(8)
    x, y = torch.rand(16, 3, 32, 32, generator=gen).to(gpu), torch.randint(0, 10, (16,), generator=gen).to(gpu)
    monkeypatch.setattr(pkg.resnet_s, "_TAIL_END", route)
    monkeypatch.setattr(pkg.resnet_s, "_TAIL_END_SUMS", sums)
    tr = pkg.train_step.AfanTrainer(model, nn.CrossEntropyLoss(), steps=2, gamma=0.5, eps=2.0, perturb_idx=6, lr=0.1, use_graph=graph,
                                    graph_warmup=0)
    n0 = pkg.ops.CALLS["head_ce"]
    r = tr.step(x, y)
    torch.cuda.synchronize()
    assert (tr._graph is not None) == graph, getattr(tr, "_graph_failed", None)
    assert pkg.ops.CALLS["head_ce"] - n0 == (3 if route else 0)       # the clean pass, PGD's second pass, the adversarial pass
    assert not pkg.ops.grid_barrier_error(gpu)
    return {"loss_clean": r["loss_clean"].clone(), "loss_adv": r["loss_adv"].clone(), "x_adv": r["x_adv"].clone(),
            "params": tr.arena.param.detach().clone()}


def _maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


@gpu_mark
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_trainer_step_same_with_and_without_the_route(pkg, gpu, graph, monkeypatch):
    """ResNet-18, batch 16, 32 x 32, K = 2, bf16 channels-last.  loss_clean depends on the forward only: bit-equal.  The separate-launch
    route is run twice first: where that repeats bit for bit, loss_adv, x_adv and the parameters must be bit-equal between the routes;
    where it does not, they are held to twice its own run-to-run difference.
    Measured on an MI355X (max |difference|, eager and graph-replayed alike; printed as "TAILEND step ..."): the separate launches
    against themselves 0 everywhere (they repeat bit for bit), against the route 0 everywhere: the route's BatchNorm backward reads the
    head's gradient by rows in the slab kernels' own order."""
    a0 = _one_step(pkg, gpu, graph, False, monkeypatch)
    a1 = _one_step(pkg, gpu, graph, False, monkeypatch)
    b = _one_step(pkg, gpu, graph, True, monkeypatch)
    own = {k: _maxdiff(a0[k], a1[k]) for k in a0}
    got = {k: _maxdiff(a0[k], b[k]) for k in a0}
    print(f"TAILEND step {'graph' if graph else 'eager'}: off-vs-off {own}  off-vs-on {got}")
    assert torch.equal(a0["loss_clean"], b["loss_clean"]), "loss_clean"
    for k in ("loss_adv", "x_adv", "params"):
        if own[k] == 0.0:
            assert torch.equal(a0[k], b[k]), f"{k}: the separate launches repeat bit for bit, the routes differ by {got[k]:.3e}"
        else:
            assert got[k] <= 2.0 * own[k], f"{k}: {got[k]:.3e} between the routes > twice the route's own {own[k]:.3e}"


@gpu_mark
def test_trainer_step_with_the_sums_in_the_head_launch(pkg, gpu, monkeypatch):
    """AFAN_TAIL_END=2: the head launch takes the last BatchNorm's sums per image (another summation order than the slab reduce, so the
    backward is not bit-comparable: see resnet_s._TAIL_END_SUMS).  What IS exact: the route runs, and everything the forward alone
    decides — loss_clean — is bit-equal; the rest is finite."""
    a = _one_step(pkg, gpu, False, False, monkeypatch)
    b = _one_step(pkg, gpu, False, True, monkeypatch, sums=True)
    print(f"TAILEND sums-mode step: {({k: _maxdiff(a[k], b[k]) for k in a})}")
    assert torch.equal(a["loss_clean"], b["loss_clean"])
    assert all(bool(torch.isfinite(v).all()) for v in b.values())


# ---- no GPU ---------------------------------------------------------------------------------------------------------------------------
def test_plain_forward_never_enters_the_node_and_an_ineligible_head_falls_back(pkg, monkeypatch):
    ops, rs = pkg.ops, pkg.resnet_s

    def boom(*a, **kw):
        raise AssertionError("ops.head_ce was called")

    monkeypatch.setattr(ops, "head_ce", boom)
    n0 = ops.CALLS["head_ce"]
    torch.manual_seed(0)
    # (the head slice alone: pool / flatten / linear run as torch modules on host tensors, everything before it is GPU-only)
    y = torch.tensor([0, 999])
    m = rs.resnet20().train()
    ln = m.layer_number
    plain = m(torch.rand(2, 64, 8, 8, requires_grad=True), end_point=ln, start_point=ln - 3)
    assert getattr(plain, "_afan_ce", None) is None and plain.shape == (2, 10)
    # K = 1000, fp32: not a head the one-launch form takes, with the target given
    m = rs.resnet18(num_classes=1000).train()
    ln = m.layer_number
    x = torch.rand(2, 512, 4, 4, requires_grad=True)
    a = m(x, end_point=ln, start_point=ln - 3)
    with_target = m(x, end_point=ln, start_point=ln - 3, ce_target=y, ce_root=torch.ones(()))
    assert getattr(with_target, "_afan_ce", None) is None and with_target.shape == (2, 1000)
    assert with_target.grad_fn is not None and "HeadCE" not in type(with_target.grad_fn).__name__
    crit = rs.fused_criterion(nn.CrossEntropyLoss(), m)
    loss = crit(with_target, y)
    loss.backward()
    assert a.shape == with_target.shape and ops.CALLS["head_ce"] == n0
    # the predicate itself: no block tail on the tensor, a wide head, a foreign root gradient
    lin = m.sequential_model[-1]
    assert not rs._head_ce_ok(torch.zeros(2, 512, 4, 4), lin, y, torch.ones(()))
    assert rs._ce_root_value(None, torch.device("cpu")) is None
