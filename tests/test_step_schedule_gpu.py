"""The one eager-then-captured schedule (train_step.StepTrainer) under each of the five trainers that run it: `graph_warmup` eager
iterations, one capture, replay; `_drop_graphs()` (what the grid guard calls when a barrier gave up) forgets the graphs and the next
step captures again.  Four iterations from one seed, three ways — eager throughout, captured, captured with the graphs dropped
between iterations two and three — must leave the same bits in the parameter arena and return the same last loss."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

KINDS = ("afan", "base", "learnable", "seg", "seg_base")


def _classification(pkg, gpu, kind, use_graph):
    torch.manual_seed(3)
    m = pkg.resnet_s.ARCHS["resnet20s"][0](init_weight_eta=1 / 9)
    m.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(gpu).train()
    crit, kw = nn.CrossEntropyLoss(), dict(lr=0.05, use_graph=use_graph, graph_warmup=1)
    if kind == "afan":
        tr = pkg.train_step.AfanTrainer(m, crit, steps=3, gamma=0.5, eps=2.0, perturb_idx=7, **kw)
    elif kind == "base":
        tr = pkg.train_step.BaseTrainer(m, crit, **kw)
    else:       # one mixing weight per residual block of ResNet-20s
        tr = pkg.learnable.LearnableTrainer(m, crit, steps=1, gamma=0.5, eps=2.0, idx_list=tuple(range(4, 13)), **kw)
    gen = torch.Generator().manual_seed(17)
    data = [(torch.rand(64, 3, 32, 32, generator=gen).to(gpu), torch.randint(0, 10, (64,), generator=gen).to(gpu)) for _ in range(4)]
    return m, tr, data


def _segmentation(pkg, gpu, kind, use_graph):
    torch.manual_seed(3)
    m = pkg.deeplab.deeplabv3plus_resnet50(num_classes=21, output_stride=16)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    m.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(gpu).train()
    kw = dict(lr=0.01, use_graph=use_graph, graph_warmup=1)
    tr = pkg.seg_trainer.SegTrainer(m, steps=1, **kw) if kind == "seg" else pkg.seg_trainer.SegBaseTrainer(m, **kw)
    gen = torch.Generator().manual_seed(5)
    data = [(torch.rand(2, 3, 129, 129, generator=gen).to(gpu), torch.randint(0, 21, (2, 129, 129), generator=gen).to(gpu))
            for _ in range(4)]
    return m, tr, data


def _run(pkg, gpu, kind, use_graph, drop=False):
    m, tr, data = (_segmentation if kind.startswith("seg") else _classification)(pkg, gpu, kind, use_graph)
    keys, graphed = [], []
    for i, (x, y) in enumerate(data):
        if drop and i == 2:
            tr._drop_graphs()
            assert tr._graph is None and tr._pieces is None and tr._graph_failed is None
        r = tr.step(x, y)
        keys.append(set(r))
        graphed.append(tr._graph is not None)
    torch.cuda.synchronize()
    assert tr.flush_guard() == 0
    return {"tr": tr, "param": tr.arena.param.clone(), "loss": r["loss"].clone(), "w": m.w.detach().clone() if kind == "learnable" else None,
            "keys": keys, "graphed": graphed}


@pytest.mark.parametrize("kind", KINDS)
def test_eager_captured_and_recaptured_steps_are_the_same_steps(pkg, gpu, kind):
    eager, graph, again = _run(pkg, gpu, kind, False), _run(pkg, gpu, kind, True), _run(pkg, gpu, kind, True, drop=True)
    for name, r in (("captured", graph), ("recaptured", again)):      # the figures first, then the assertions
        print(f"{kind} {name} vs eager: max |d param| = {float((r['param'] - eager['param']).abs().max()):.3e}, "
              f"loss {float(r['loss']):.9g} vs {float(eager['loss']):.9g}")
    assert eager["graphed"] == [False] * 4 and eager["tr"]._graph_failed is None
    assert graph["graphed"] == [False, True, True, True]               # the first step ran eagerly, the capture came with the second
    assert again["graphed"] == [False, True, True, True]               # ... and again with the third, after the drop
    for r in (graph, again):
        assert r["tr"]._graph is not None and r["tr"]._graph_failed is None
        assert torch.equal(r["param"], eager["param"])
        assert torch.equal(r["loss"], eager["loss"])
        if kind == "learnable":
            assert torch.equal(r["w"], eager["w"])
        assert all(k == eager["keys"][0] for k in r["keys"] + eager["keys"])       # eager and replayed steps return the same observables
