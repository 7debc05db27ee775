"""cls_entry.py without a GPU: the shared train(), the evaluation loop, the epoch-end files, resume and the epoch loop, on stubs.  The
log lines are literal: what main_perturb.py, main_base.py and main_learnable.py print, by the reference's format strings."""
import argparse
import importlib
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

BARRIER = ("in-launch BatchNorm: a grid barrier gave up; the affected steps were run again on the two-launch forms "
           "(their logged loss / accuracy values are invalid)")
SIZES = [4, 2, 2, 4, 2]                                 # batch sizes: the meters weigh by them
LOSS = [1.0, 0.25, 0.5, 2.0, 0.75]
PREC = [50.0, 100.0, 25.0, 0.0, 75.0]
L2 = [1.0, 2.0, 3.0, 4.0, 5.0]                          # per-sample norm of batch i; linf is an eighth of it (exact in binary)
LINES = ["Epoch: [0][0/5]\tLoss 1.0000 (1.0000)\tAccuracy 50.000 (50.000)\t",         # 4 samples
         "Epoch: [0][2/5]\tLoss 0.5000 (0.6875)\tAccuracy 25.000 (56.250)\t",         # 8 samples: 5.5 / 8, 450 / 8
         "Epoch: [0][4/5]\tLoss 0.7500 (1.0714)\tAccuracy 75.000 (42.857)\t"]         # 14 samples: 15 / 14, 600 / 14
NORM_LINES = {None: [],
              "cat": ["l2 mean = 2.857142925262451", "linf mean = 0.3571428656578064"],                   # float32(40 / 14), float32(5 / 14)
              "layers": ["l2 mean = tensor([2.8571, 5.7143])", "linf mean = tensor([0.3571, 0.7143])"]}   # second layer: twice the first


@pytest.fixture(scope="module")
def ce(pkg):
    return importlib.import_module("cv_a-fan_amd.cls_entry")


class _Arena:
    refreshed = 0

    def refresh_shadow(self):
        self.refreshed += 1


class StubTrainer:
    """step() hands out the fixed scalars of batch i and records the learning rate it ran at; flush_guard() returns a scripted value
    and records how many steps had been issued."""

    def __init__(self, norms=None, guard=()):
        self.model = nn.Linear(2, 2)
        self.optimizer = torch.optim.SGD(self.model.parameters(), lr=7.0)
        self.arena = _Arena()
        self.norms, self.guard = norms, list(guard)
        self.lrs, self.flushes = [], []

    def step(self, inp, target):
        i = len(self.lrs) % len(SIZES)
        self.lrs.append(self.optimizer.param_groups[0]["lr"])
        r = {"loss": torch.tensor(LOSS[i]), "prec1": torch.tensor(PREC[i])}
        if self.norms == "cat":
            r["l2"], r["linf"] = torch.full((inp.size(0),), L2[i]), torch.full((inp.size(0),), L2[i] / 8)
        elif self.norms == "layers":
            l2 = torch.stack([torch.full((inp.size(0),), L2[i]), torch.full((inp.size(0),), 2 * L2[i])])
            r["l2"], r["linf"] = l2, l2 / 8
        return r

    def flush_guard(self):
        self.flushes.append(len(self.lrs))
        return self.guard.pop(0) if self.guard else False


def _batches(n=5):
    return [(torch.zeros(m, 3), torch.zeros(m, dtype=torch.int64)) for m in SIZES[:n]]


def _args(**kw):
    return argparse.Namespace(**dict(dict(print_freq=2, max_iters=0, lr=0.1), **kw))


def _train(ce, norms, epoch=0, n=5, guard=(), **kw):
    trainer, lines = StubTrainer(norms, guard), []
    out = ce.train(_batches(n), trainer, trainer.optimizer, epoch, _args(**kw), lambda *a: lines.append(" ".join(str(v) for v in a)),
                   norms=norms)
    return out, trainer, lines


@pytest.mark.parametrize("norms", [None, "cat", "layers"])
def test_train_lines_meters_and_cadence(ce, norms):
    out, trainer, lines = _train(ce, norms)
    assert lines == LINES + NORM_LINES[norms] + ["train_accuracy 42.857"]
    assert out[:2] == (600.0 / 14, 15.0 / 14)                          # averages weighted by batch size
    assert trainer.flushes == [1, 3, 5, 5]                              # read back after iterations 0, 2, 4 and at the end
    assert trainer.model.training
    if norms is None:
        assert len(out) == 2
    else:
        l2, linf = out[2:]
        want = np.array(40.0 / 14) if norms == "cat" else np.array([40.0 / 14, 80.0 / 14])
        assert isinstance(l2, np.ndarray) and l2.dtype == np.float32 and l2.shape == want.shape
        assert np.allclose(l2, want, rtol=1e-6, atol=0) and np.allclose(linf, want / 8, rtol=1e-6, atol=0)


@pytest.mark.parametrize("norms", [None, "cat", "layers"])
def test_warm_up_is_epoch_0_only(ce, norms):
    _, trainer, _ = _train(ce, norms)
    assert trainer.lrs == [min(i * 0.1 / 4, 0.1) for i in range(5)] and trainer.lrs[0] == 0.0 and trainer.lrs[-1] == 0.1
    _, trainer, lines = _train(ce, norms, epoch=3)
    assert trainer.lrs == [7.0] * 5 and lines[0].startswith("Epoch: [3][0/5]\t")


@pytest.mark.parametrize("norms", [None, "cat", "layers"])
def test_one_batch_epoch_warms_up_to_the_full_rate(ce, norms):
    """A one-batch epoch 0 has no ramp to divide: it runs at --lr (train_step.warmup_lr alone raises ZeroDivisionError here)."""
    out, trainer, lines = _train(ce, norms, n=1)
    assert trainer.lrs == [0.1] and out[:2] == (50.0, 1.0)
    assert lines[0] == "Epoch: [0][0/1]\tLoss 1.0000 (1.0000)\tAccuracy 50.000 (50.000)\t" and lines[-1] == "train_accuracy 50.000"


def test_max_iters_stops_the_epoch(ce):
    out, trainer, lines = _train(ce, "cat", max_iters=3)
    assert len(trainer.lrs) == 3 and trainer.flushes == [1, 3, 3]
    assert lines == LINES[:2] + ["l2 mean = 1.75", "linf mean = 0.21875", "train_accuracy 56.250"]     # 14 / 8
    assert out[:2] == (56.25, 0.6875)


@pytest.mark.parametrize("norms", [None, "cat", "layers"])
def test_barrier_message_at_a_print_and_at_the_end(ce, norms):
    _, _, lines = _train(ce, norms, guard=[False, True, False, True])
    assert [i for i, ln in enumerate(lines) if ln == BARRIER] == [1, 4]        # before the [2/5] line; after the [4/5] line
    assert [ln for ln in lines if ln != BARRIER] == LINES + NORM_LINES[norms] + ["train_accuracy 42.857"]


# ------------------------------------------------------------------------------------ evaluation loop
EVAL_BODY = ["{}: [0/3]\tLoss 1.0000 (1.0000)\tAccuracy 50.000 (50.000)",
             "{}: [2/3]\tLoss 0.5000 (0.6875)\tAccuracy 25.000 (56.250)"]


def _per_batch():
    seen = []

    def per_batch(inp, target):
        seen.append(inp.size(0))
        i = len(seen) - 1
        return torch.tensor(LOSS[i]), torch.tensor(PREC[i])

    return per_batch


@pytest.mark.parametrize("tag, closing", [("Test", "valid_accuracy"), ("Robust", "robust_accuracy")])
def test_evaluation_loop(ce, tag, closing):
    lines = []
    got = ce.evaluate(_batches(3), _per_batch(), tag, closing, _args(), lambda *a: lines.append(" ".join(str(v) for v in a)))
    assert lines == [ln.format(tag) for ln in EVAL_BODY] + [closing + " 56.250"] and got == (56.25, 0.6875)
    lines = []
    ce.evaluate(_batches(3), _per_batch(), tag, closing, _args(print_freq=1), lines.append)
    assert lines[1] == tag + ": [1/3]\tLoss 0.2500 (0.7500)\tAccuracy 100.000 (66.667)" and len(lines) == 4      # 4.5 / 6, 400 / 6


def test_validate_and_robust_validate_are_that_loop(ce, pkg, monkeypatch):
    mp, mi = (importlib.import_module("cv_a-fan_amd." + n) for n in ("main_perturb", "main_inference"))
    assert mp.validate is ce.validate
    made = []

    class Ev:
        def __init__(self, *a):
            made.append(a)
            self.evaluate = _per_batch()
            self.attack = lambda inp, target, f=_per_batch(): ("x_adv",) + f(inp, target)

        def refresh(self):
            made.append("refresh")

    monkeypatch.setattr(pkg.infer, "evaluator_for", Ev)
    monkeypatch.setattr(pkg.infer, "Attacker", Ev)
    model, crit = nn.Linear(2, 2), nn.CrossEntropyLoss()
    lines = []
    assert mp.validate(_batches(3), model, crit, _args(), lines.append) == (56.25, 0.6875)
    assert lines == [ln.format("Test") for ln in EVAL_BODY] + ["valid_accuracy 56.250"]
    assert made == [(model, crit), "refresh"] and not model.training
    del lines[:], made[:]
    args = _args(attack_eps=8.0, attack_gamma=2.0, attack_steps=3, attack_randinit=True)
    assert mi.robust_validate(_batches(3), model.train(), crit, args, lines.append) == (56.25, 0.6875)
    assert lines == [ln.format("Robust") for ln in EVAL_BODY] + ["robust_accuracy 56.250"]
    assert made == [(model, crit, 8.0 / 255.0, 2.0 / 255.0, 3, True), "refresh"] and not model.training


# ------------------------------------------------------------------------ epoch end, resume, epoch loop
def _state(lr=0.1, w=False):
    model = nn.Linear(2, 2)
    opts = {"optimizer": torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9)}
    if w:
        opts["optimizer_w"] = torch.optim.SGD([nn.Parameter(torch.zeros(9))], lr=0.01)
    return model, opts, torch.optim.lr_scheduler.MultiStepLR(opts["optimizer"], milestones=[1, 2], gamma=0.1)


PROGRAMS = {"main_perturb": dict(w=False, norms=True, plot=True), "main_base": dict(w=False, norms=False, plot=True),
            "main_learnable": dict(w=True, norms=True, plot=False)}


@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_epoch_end_files_and_resume(ce, tmp_path, program):
    cfg = PROGRAMS[program]
    model, opts, sched = _state(w=cfg["w"])
    sched.step()
    result = {"train": [10.0], "test_ta": [30.0], "ta": [20.0]}
    norm_result = {"l2": {1: np.float32(1.5)}, "linf": {1: np.float32(0.5)}} if cfg["norms"] else None
    d = tmp_path / "first"
    d.mkdir()
    ce.write_epoch(str(d), 0, model, 20.0, False, opts, sched, result, norm_result, cfg["plot"])
    files = {"checkpoint.pt", "result.pkl"} | ({"result_norm.pkl"} if cfg["norms"] else set())
    try:
        import matplotlib  # noqa: F401
        files |= {"net_train.png"} if cfg["plot"] else set()
    except ImportError:
        pass
    assert set(os.listdir(d)) == files                                   # no improvement: no best_model.pt
    ce.write_epoch(str(d), 1, model, 25.0, True, opts, sched, result, norm_result, cfg["plot"])
    assert set(os.listdir(d)) == files | {"best_model.pt"}
    keys = ["epoch", "state_dict", "best_prec1", "optimizer"] + (["optimizer_w"] if cfg["w"] else []) + ["scheduler"]
    for name in ("checkpoint.pt", "best_model.pt"):
        ck = torch.load(str(d / name), map_location="cpu", weights_only=False)
        assert list(ck) == keys and ck["epoch"] == 2 and ck["best_prec1"] == 25.0
    assert pickle.load(open(d / "result.pkl", "rb")) == result
    if cfg["norms"]:
        assert pickle.load(open(d / "result_norm.pkl", "rb")) == norm_result

    model2, opts2, sched2 = _state(lr=0.5, w=cfg["w"])
    trainer = StubTrainer()
    assert ce.resume(str(d), "cpu", model2, trainer, opts2, sched2) == (25.0, 2)
    assert trainer.arena.refreshed == 1 and sched2.last_epoch == 1
    assert all(torch.equal(a, b) for a, b in zip(model2.state_dict().values(), model.state_dict().values()))
    assert opts2["optimizer"].param_groups[0]["lr"] == opts["optimizer"].param_groups[0]["lr"] == pytest.approx(0.01)


@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_epoch_loop_and_resume(ce, tmp_path, program):
    """Two epochs, then --resume into a third: the learning-rate line (after main_learnable's weight lines), the curves, the
    checkpoint's epoch and best_prec1, and a resumed run that starts where the checkpoint says."""
    cfg = PROGRAMS[program]
    norms = None if not cfg["norms"] else "layers" if cfg["w"] else "cat"
    scores = iter([60.0, 1.0, 50.0, 2.0, 70.0, 3.0])                     # validation, test, per epoch

    def run(epochs, resume):
        trainer, lines = StubTrainer(norms), []
        model = trainer.model
        opts = {"optimizer": trainer.optimizer}
        if cfg["w"]:
            opts["optimizer_w"] = torch.optim.SGD([nn.Parameter(torch.zeros(9))], lr=0.01)
        sched = torch.optim.lr_scheduler.MultiStepLR(trainer.optimizer, milestones=[50], gamma=0.1)
        args = _args(epochs=epochs, resume=resume, save_dir=str(tmp_path / "run"))
        log = lambda *a: lines.append(" ".join(str(v) for v in a))
        kw = dict(header=lambda log, lr: (log("weight1 = ", 0.5), log(lr), log(0.01))) if cfg["w"] else {}
        best = ce.run_epochs(args, "cpu", 0, log, model, None, trainer, opts, sched, [_batches()] * 3,
                             lambda *a: (next(scores), 0.0), norms=norms, plot=cfg["plot"], **kw)
        return best, lines, trainer

    best, lines, trainer = run(2, False)
    assert best == 60.0 and "resume from checkpoint" not in lines
    head = ["weight1 =  0.5", "7.0", "0.01"] if cfg["w"] else ["7.0"]
    assert lines[:len(head) + 1] == head + [LINES[0]]
    assert [ln for ln in lines if ln.startswith("Epoch: [") and "][0/5]" in ln] == [LINES[0], LINES[0].replace("[0][", "[1][")]
    d = tmp_path / "run"
    ck = torch.load(str(d / "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert ck["epoch"] == 2 and ck["best_prec1"] == 60.0 and ("optimizer_w" in ck) == cfg["w"]
    assert torch.load(str(d / "best_model.pt"), map_location="cpu", weights_only=False)["epoch"] == 1       # epoch 2 was no better
    assert pickle.load(open(d / "result.pkl", "rb")) == {"train": [600.0 / 14] * 2, "test_ta": [1.0, 2.0], "ta": [60.0, 50.0]}
    assert os.path.exists(d / "result_norm.pkl") == cfg["norms"] and os.path.exists(d / "net_train.png") <= cfg["plot"]
    if cfg["norms"]:
        assert set(pickle.load(open(d / "result_norm.pkl", "rb"))["l2"]) == {1, 2}

    best, lines, trainer = run(3, True)
    assert lines[0] == "resume from checkpoint" and best == 70.0 and trainer.arena.refreshed == 1
    assert [ln for ln in lines if ln.startswith("Epoch: [")][0].startswith("Epoch: [2][0/5]\t") and len(trainer.lrs) == 5
    assert torch.load(str(d / "checkpoint.pt"), map_location="cpu", weights_only=False)["epoch"] == 3
    assert torch.load(str(d / "best_model.pt"), map_location="cpu", weights_only=False)["best_prec1"] == 70.0
