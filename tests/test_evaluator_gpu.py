"""infer.Evaluator: the fused eval forward (one launch per convolution, BatchNorm in the epilogue, hipGraph per batch shape) gives the
eager eval forward's logits bit for bit, follows the weights through training, and leaves the model's state alone."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _model(pkg, gpu, arch, dtype=torch.bfloat16, nhwc=True, seed=0):
    torch.manual_seed(seed)
    ctor, idx = pkg.resnet_s.ARCHS[arch]
    m = ctor()
    m.set_compute_dtype(dtype)
    m.set_channels_last(nhwc).to(gpu)
    return m, idx


def _trainer(pkg, m, idx):
    return pkg.train_step.AfanTrainer(m, nn.CrossEntropyLoss(), steps=1, gamma=0.5, eps=2.0, perturb_idx=idx,
                                      layer_number=m.layer_number, lr=0.05)


def _batch(gpu, n, side, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, side, side, generator=g).to(gpu), torch.randint(0, classes, (n,), generator=g).to(gpu)


def _train(pkg, tr, m, gpu, steps, side, classes, n, seed=1):
    m.train()
    for i in range(steps):
        x, y = _batch(gpu, n, side, classes, seed + i)
        tr.step(x, y)
    torch.cuda.synchronize()


def _eager(m, x):
    m.eval()
    with torch.no_grad():
        return m(x, end_point=m.layer_number, start_point=0)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.float().view(torch.int32), b.float().view(torch.int32))


CONFIGS = [("resnet20s", 128, 32, 10), ("resnet20s", 16, 32, 10), ("resnet56s", 128, 32, 10), ("resnet56s", 16, 32, 10),
           ("resnet18", 256, 32, 10), ("resnet50", 8, 224, 1000)]


@pytest.mark.parametrize("arch,n,side,classes", CONFIGS)
def test_evaluator_matches_eager_and_follows_training(pkg, gpu, arch, n, side, classes):
    m, idx = _model(pkg, gpu, arch)
    tr = _trainer(pkg, m, idx)
    _train(pkg, tr, m, gpu, 2, side, classes, min(n, 64))
    crit = nn.CrossEntropyLoss()
    ev = pkg.infer.Evaluator(m, crit)
    assert ev.fused
    n_convs = sum(isinstance(mod, pkg.resnet_s.Conv2d) for mod in m.modules())
    for rnd in range(2):
        m.eval()
        bufs = {k: v.clone() for k, v in m.state_dict().items()}
        ev.refresh()
        x, y = _batch(gpu, n, side, classes, 100 + rnd)
        want = _eager(m, x)
        if rnd == 0:
            calls = {"bn_apply": 0, "affine_apply": 0}
            orig = {k: getattr(pkg.ops, k) for k in calls}

            def counted(name):
                def f(*a, **k):
                    calls[name] += 1
                    return orig[name](*a, **k)
                return f
            try:
                for k in calls:
                    setattr(pkg.ops, k, counted(k))
                with pkg.ops.conv_trace() as t1:
                    loss1, prec1 = ev.evaluate(x, y)                   # first sight of the shape: fused, no graph
            finally:
                for k, f in orig.items():
                    setattr(pkg.ops, k, f)
            assert _same(ev.last_logits, want), arch
            fwd = [r for r in t1.records if r["op"] == "fwd"]
            assert len(fwd) == n_convs == len(t1.records), (len(fwd), n_convs)
            assert calls == {"bn_apply": 0, "affine_apply": 0}
            with pkg.ops.conv_trace() as t2:
                loss2, prec2 = ev.evaluate(x, y)                       # second sight: captured
            results = [(loss1, prec1), (loss2, prec2)]
        else:
            results = []                                               # the graph of round 0 replays on refreshed buffers
        with pkg.ops.conv_trace() as t3:
            loss3, prec3 = ev.evaluate(x, y)                           # replay
        assert len(t3.records) == 0
        assert _same(ev.last_logits, want), (arch, rnd)
        ref_loss = crit(want, y).float()
        ref_prec = pkg.infer.accuracy(want.float(), y)
        for l_, p_ in results + [(loss3, prec3)]:
            assert l_.item() == ref_loss.item() and p_.item() == ref_prec.item()
        # running statistics, num_batches_tracked and parameters untouched by the evaluation
        after = m.state_dict()
        assert all(torch.equal(bufs[k], after[k]) for k in bufs)
        if rnd == 0:
            _train(pkg, tr, m, gpu, 2, side, classes, min(n, 64), seed=50)   # stale buffers would show in round 2


def test_training_interleaved_with_evaluations_is_unchanged(pkg, gpu):
    """Training with Evaluator evaluations between the steps ends on the same parameters as with eager evaluations."""
    finals = []
    for use_ev in (False, True):
        m, idx = _model(pkg, gpu, "resnet20s", seed=4)
        tr = _trainer(pkg, m, idx)
        ev = pkg.infer.Evaluator(m, nn.CrossEntropyLoss())
        for i in range(3):
            _train(pkg, tr, m, gpu, 2, 32, 10, 64, seed=10 * i)
            m.eval()
            x, y = _batch(gpu, 64, 32, 10, 7)
            if use_ev:
                ev.refresh()
                for _ in range(3):
                    ev.evaluate(x, y)
            else:
                _eager(m, x)
        torch.cuda.synchronize()
        finals.append({k: v.clone() for k, v in m.state_dict().items()})
    assert all(torch.equal(finals[0][k], finals[1][k]) for k in finals[0])


@pytest.mark.parametrize("dtype,nhwc", [(torch.float32, True), (torch.float32, False), (torch.bfloat16, False)])
def test_fp32_and_nchw_models_take_the_eager_forward(pkg, gpu, dtype, nhwc):
    m, idx = _model(pkg, gpu, "resnet20s", dtype=dtype, nhwc=nhwc)
    ev = pkg.infer.Evaluator(m, nn.CrossEntropyLoss())
    assert not ev.fused
    x, y = _batch(gpu, 32, 32, 10, 3)
    want = _eager(m, x)
    ev.refresh()
    for _ in range(3):
        loss, prec = ev.evaluate(x, y)
        assert _same(ev.last_logits, want)
    assert loss.item() == nn.CrossEntropyLoss()(want, y).float().item()


def test_other_criterion_takes_the_eager_forward(pkg, gpu):
    m, _ = _model(pkg, gpu, "resnet20s")
    ev = pkg.infer.Evaluator(m, nn.CrossEntropyLoss(label_smoothing=0.1))
    assert not ev.fused
