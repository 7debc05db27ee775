"""main_inference.py (cmd/run_test.sh's entry point) end to end on the GPU, and main_perturb.validate's output against the eager loop
it replaced."""
import importlib
import io
import os
import pickle
import re
import subprocess
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT

pytestmark = pytest.mark.gpu
CWD = os.path.join(ROOT, "cv_a-fan_amd")


def _mp():
    return importlib.import_module("cv_a-fan_amd.main_perturb")


def _run(script, args):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-u", script] + args, cwd=CWD, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _eager_validate(mp, loader, model, criterion, print_freq):
    """main_perturb.validate as it was before the Evaluator (per-batch reads, eager forward)."""
    losses, top1 = mp.AverageMeter(), mp.AverageMeter()
    model.eval()
    for i, (inp, target) in enumerate(loader):
        with torch.no_grad():
            output = model(inp, end_point=model.layer_number, start_point=0)
            loss = criterion(output, target)
        losses.update(loss.float().item(), inp.size(0))
        top1.update(mp.accuracy(output.float(), target).item(), inp.size(0))
        if i % print_freq == 0:
            print("Test: [{0}/{1}]\t"
                  "Loss {loss.val:.4f} ({loss.avg:.4f})\t"
                  "Accuracy {top1.val:.3f} ({top1.avg:.3f})".format(i, len(loader), loss=losses, top1=top1))
    print("valid_accuracy {top1.avg:.3f}".format(top1=top1))
    return top1.avg, losses.avg


def _model(pkg, gpu, arch, state=None):
    m = pkg.resnet_s.ARCHS[arch][0]()
    m.set_compute_dtype(torch.bfloat16)
    m.set_channels_last(True).to(gpu)
    if state is not None:
        m.load_state_dict(state)
    return m


def test_checkpoint_of_main_perturb_evaluates(pkg, gpu, tmp_path):
    save = str(tmp_path / "run")
    _run("main_perturb.py", ["--seed", "3", "--save_dir", save, "--arch", "resnet20s", "--perturb_idx", "7", "--synthetic", "256",
                             "--batch_size", "64", "--print_freq", "2", "--steps", "1", "--epochs", "1"])
    ck = os.path.join(save, "checkpoint.pt")
    out = _run("main_inference.py", ["--pretrained", ck, "--arch", "resnet20s", "--synthetic", "200", "--batch_size", "64",
                                     "--print_freq", "1"])
    assert out.splitlines()[0].startswith("Namespace(")
    assert "Test: [0/3]\tLoss" in out
    got = re.findall(r"valid_accuracy (\S+)", out)
    state = torch.load(ck, map_location=gpu, weights_only=False)["state_dict"]
    m = _model(pkg, gpu, "resnet20s", state)
    loader = _mp().SyntheticLoader(200, 64, gpu)
    buf = io.StringIO()
    with redirect_stdout(buf):
        _eager_validate(_mp(), loader, m, nn.CrossEntropyLoss(), 1)
    assert got == re.findall(r"valid_accuracy (\S+)", buf.getvalue())
    assert out.split("\n", 1)[1] == buf.getvalue()


def test_reference_layout_checkpoint_and_test_batch(pkg, gpu, orc, tmp_path):
    """A state_dict of the reference's own model (335 keys) and a tiny cifar-10-batches-py/test_batch with a ragged last batch."""
    ref = orc.resnet56s()
    sd = ref.state_dict()
    assert len(sd) == 335
    ck = tmp_path / "ref.pt"
    torch.save({"state_dict": sd}, str(ck))
    d = tmp_path / "data" / "cifar-10-batches-py"
    d.mkdir(parents=True)
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, (150, 3072), dtype=np.uint8)
    labels = [int(v) for v in rng.integers(0, 10, 150)]
    with open(d / "test_batch", "wb") as f:
        pickle.dump({"data": data, "labels": labels}, f)
    out = _run("main_inference.py", ["--pretrained", str(ck), "--data", str(tmp_path / "data"), "--batch_size", "64",
                                     "--print_freq", "1"])
    assert "Test: [2/3]" in out
    m = _model(pkg, gpu, "resnet56s", sd)
    xt, yt = _mp()._load_cifar10_test(str(tmp_path / "data"))
    loader = _mp().DeviceLoader(xt, yt, 64, gpu, False, drop_last=False)
    buf = io.StringIO()
    with redirect_stdout(buf):
        _eager_validate(_mp(), loader, m, nn.CrossEntropyLoss(), 1)
    assert out.split("\n", 1)[1] == buf.getvalue()


@pytest.mark.parametrize("arch", ["resnet20s", "resnet18"])
def test_validate_output_is_byte_identical_to_the_eager_loop(pkg, gpu, arch):
    mp = _mp()
    torch.manual_seed(0)
    m = _model(pkg, gpu, arch)
    with torch.no_grad():                  # non-trivial running statistics
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
    loader = mp.SyntheticLoader(16 * 5 + 8, 16, gpu)
    args = types.SimpleNamespace(print_freq=1)
    crit = nn.CrossEntropyLoss()
    for epoch in range(3):                 # first pass fused, then captured, then replayed
        lines = []
        got = mp.validate(loader, m, crit, args, lambda *a: lines.append(" ".join(str(v) for v in a)))
        buf = io.StringIO()
        with redirect_stdout(buf):
            want = _eager_validate(mp, loader, m, crit, 1)
        assert "\n".join(lines) + "\n" == buf.getvalue(), epoch
        assert got == want
