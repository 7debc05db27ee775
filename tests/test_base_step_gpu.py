"""train_step.BaseTrainer — the baseline iteration (Classification/main_base.py:157-162) — against three iterations of the
reference's own ResNet-20s (tests/golden/base_r20s.npz, tools/gen_base_golden.py), and against itself: captured vs eager, the
trainer vs the same steps written out by hand, the data-parallel program on one GPU vs the plain one.

Measured on an MI355X (fp32 NCHW against the golden): see the PARITY lines this test prints."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import golden

pytestmark = pytest.mark.gpu


def _sd0():
    g = golden("step_r20s_k1")
    return {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd0/")}


def _model(pkg, gpu, arch, dtype, nhwc, sd=None, seed=3):
    torch.manual_seed(seed)
    torch.backends.cudnn.deterministic = True
    m = pkg.resnet_s.ARCHS[arch][0]()
    if sd is not None:
        m.load_state_dict(sd)
    m.set_compute_dtype(dtype)
    m.set_channels_last(nhwc).to(gpu).train()
    return m


def _state(tr):
    torch.cuda.synchronize()
    out = {"param": tr.arena.param.clone(), "momentum": tr.arena.momentum_buf.clone()}
    for k, v in tr.model.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out[k] = v.clone()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _batches(n, bs, gpu, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(bs, 3, 32, 32, generator=g).to(gpu), torch.randint(0, 10, (bs,), generator=g).to(gpu)) for _ in range(n)]


def test_three_steps_fp32_match_the_reference(pkg, gpu):
    g = golden("base_r20s")
    model = _model(pkg, gpu, "resnet20s", torch.float32, False, _sd0())
    ck = np.array([[float(v.double().sum()), float(v.double().abs().sum())] for v in model.state_dict().values()])
    np.testing.assert_allclose(ck, g["ck0"], rtol=1e-12)                 # the initial weights are the reference's
    assert list(model.state_dict().keys()) == [str(k) for k in g["keys"]]
    lr, mom, wd = [float(v) for v in g["hyper"]]
    tr = pkg.train_step.BaseTrainer(model, nn.CrossEntropyLoss(), lr=lr, momentum=mom, weight_decay=wd)
    xs, ys = torch.from_numpy(g["xs"]).to(gpu), torch.from_numpy(g["ys"]).to(gpu)
    got, out0 = [], None
    for i in range(3):
        r = tr.step(xs[i], ys[i])
        assert set(r) == {"loss", "prec1", "out_clean"}
        got.append(float(r["loss"]))
        if i == 0:
            out0 = r["out_clean"].float().cpu().numpy()
    ref, spread = [float(v) for v in g["losses"]], [float(v) for v in g["loss_spread"]]
    bounds = [1e-5] + [max(1e-4, 2.0 * spread[i]) * max(1.0, abs(ref[i])) for i in (1, 2)]
    for i in range(3):
        print(f"PARITY base_r20s [fp32 NCHW]: |loss - reference| {abs(got[i] - ref[i]):.2e}   reference-vs-reference spread "
              f"{spread[i]:.2e}   bound {bounds[i]:.2e}   (iteration {i})")
    for i in range(3):
        assert abs(got[i] - ref[i]) <= bounds[i], (i, got[i], ref[i])
    np.testing.assert_allclose(out0, g["out_clean"], rtol=1e-3, atol=2e-4)
    sd1 = model.state_dict()
    for k, v in sd1.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3, k
    for k in g.files:
        if k.startswith("sd1/") and "num_batches" not in k:
            np.testing.assert_allclose(sd1[k[4:]].cpu().numpy(), g[k], rtol=2e-3, atol=2e-4, err_msg=k)
    ck1 = np.array([[float(v.double().sum()), float(v.double().abs().sum())] for v in sd1.values()])
    np.testing.assert_allclose(ck1[:, 1], g["ck1"][:, 1], rtol=5e-2, atol=5e-3)


@pytest.mark.parametrize("arch", ["resnet20s", "resnet18"])
def test_captured_equals_eager_bf16(pkg, gpu, arch):
    data = _batches(6, 8, gpu)
    runs = []
    for use_graph in (True, False):
        model = _model(pkg, gpu, arch, torch.bfloat16, True)
        tr = pkg.train_step.BaseTrainer(model, nn.CrossEntropyLoss(), use_graph=use_graph, graph_warmup=2)
        losses = [tr.step(x, y)["loss"].clone() for x, y in data]
        assert (tr._graph is not None) == use_graph and tr._graph_failed is None
        assert not pkg.ops.grid_barrier_error(gpu)
        runs.append((torch.stack(losses), _state(tr)))
    assert torch.equal(runs[0][0], runs[1][0])
    _same(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][0]).all())


def test_trainer_equals_the_steps_written_out(pkg, gpu):
    data = _batches(2, 8, gpu, seed=1)
    crit = nn.CrossEntropyLoss()
    model = _model(pkg, gpu, "resnet20s", torch.bfloat16, True)
    tr = pkg.train_step.BaseTrainer(model, crit, use_graph=False)
    for x, y in data:
        tr.step(x, y)
    a = _state(tr)
    model = _model(pkg, gpu, "resnet20s", torch.bfloat16, True)
    arena = pkg.arena.ParamArena(model)
    opt = pkg.arena.ArenaSGD(arena, 0.1, 0.9, 5e-4)
    fc = pkg.resnet_s.fused_criterion(crit, model)
    for x, y in data:
        pkg.ops.acc_reset(gpu)
        loss = fc(model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    b = _state(type("T", (), {"arena": arena, "model": model}))
    _same(a, b)


def test_data_parallel_program_on_one_gpu_equals_the_plain_trainer(pkg, gpu):
    data = _batches(3, 8, gpu, seed=2)
    states = []
    for emulate in (False, True):
        model = _model(pkg, gpu, "resnet20s", torch.bfloat16, True)
        tr = pkg.train_step.BaseTrainer(model, nn.CrossEntropyLoss(), graph_warmup=1, emulate_dp=emulate)
        for x, y in data:
            tr.step(x, y)
        if emulate:
            assert isinstance(tr.reducer, pkg.train_step.NullReducer) and tr.reducer.announced == [(0, len(tr.arena.params))]
            assert tr.reducer.fused_while_in_flight == 0
        states.append(_state(tr))
    _same(states[0], states[1])


def test_afan_trainer_is_unchanged_beside_a_base_trainer(pkg, gpu):
    x, y = _batches(1, 8, gpu, seed=4)[0]

    def afan_step():
        model = _model(pkg, gpu, "resnet20s", torch.bfloat16, True)
        tr = pkg.train_step.AfanTrainer(model, nn.CrossEntropyLoss(), steps=2, gamma=0.5, eps=2.0, perturb_idx=7, layer_number=16)
        r = tr.step(x, y)
        return {k: r[k].clone() for k in ("loss", "loss_adv", "loss_clean", "prec1", "l2", "linf", "out_clean")}, _state(tr)
    first = afan_step()
    bt = pkg.train_step.BaseTrainer(_model(pkg, gpu, "resnet20s", torch.bfloat16, True), nn.CrossEntropyLoss(), use_graph=False)
    bt.step(x, y)
    second = afan_step()
    _same(first[0], second[0])
    _same(first[1], second[1])
    assert isinstance(bt, pkg.train_step.StepTrainer) and issubclass(pkg.train_step.AfanTrainer, pkg.train_step.StepTrainer)
