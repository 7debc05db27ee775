"""main_inference.py --attack_steps end to end on the GPU: no attack is today's output byte for byte; with one, `Robust:` lines and a
robust accuracy not above the clean one."""
import argparse
import io
import os
import re
import subprocess
import sys
from contextlib import redirect_stdout

import pytest
import torch
import torch.nn as nn

from conftest import ROOT

pytestmark = pytest.mark.gpu
CWD = os.path.join(ROOT, "cv_a-fan_amd")


def _run(args):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-u", "main_inference.py"] + args, cwd=CWD, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def checkpoint(pkg, gpu, tmp_path_factory):
    """A synthetic ResNet-20s checkpoint with non-trivial running statistics."""
    torch.manual_seed(2)
    m = pkg.resnet_s.ARCHS["resnet20s"][0]()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
    path = str(tmp_path_factory.mktemp("ck") / "checkpoint.pt")
    torch.save({"state_dict": m.state_dict()}, path)
    return path


def test_no_attack_is_the_clean_evaluation_byte_for_byte(pkg, gpu, checkpoint):
    """--attack_steps 0 (explicit or by default): the namespace line and every line after it are what main_inference printed before
    the flags existed — the five reference flags and the four earlier additions, then main_perturb.validate's lines."""
    base = ["--pretrained", checkpoint, "--arch", "resnet20s", "--synthetic", "64", "--batch_size", "16", "--print_freq", "1"]
    out = _run(base + ["--attack_steps", "0"])
    assert out == _run(base)
    want_ns = argparse.Namespace(data="../data", print_freq=1, gpu=0, pretrained=checkpoint, batch_size=16, arch="resnet20s", dtype="bf16",
                                 layout="nhwc", synthetic=64)
    assert out.split("\n", 1)[0] == repr(want_ns)
    mp = __import__(pkg.__name__ + ".main_perturb", fromlist=["validate"])
    m = pkg.resnet_s.ARCHS["resnet20s"][0]()
    m.set_compute_dtype(torch.bfloat16)
    m.set_channels_last(True).to(gpu)
    m.load_state_dict(torch.load(checkpoint, map_location=gpu, weights_only=False)["state_dict"])
    buf = io.StringIO()
    with redirect_stdout(buf):
        mp.validate(mp.SyntheticLoader(64, 16, gpu), m, nn.CrossEntropyLoss(), argparse.Namespace(print_freq=1), print)
    assert out.split("\n", 1)[1] == buf.getvalue()
    assert "Robust" not in out and "robust_accuracy" not in out


def test_attack_prints_robust_lines(pkg, gpu, checkpoint):
    out = _run(["--pretrained", checkpoint, "--arch", "resnet20s", "--synthetic", "64", "--batch_size", "16", "--print_freq", "1",
                "--attack_steps", "2"])
    lines = out.splitlines()
    assert lines[0].startswith("Namespace(") and "attack_steps=2" in lines[0]
    robust = [ln for ln in lines if ln.startswith("Robust: [")]
    assert len(robust) == 4
    assert all(re.fullmatch(r"Robust: \[\d/4\]\tLoss \d+\.\d{4} \(\d+\.\d{4}\)\tAccuracy \d+\.\d{3} \(\d+\.\d{3}\)", ln) for ln in robust), robust
    clean = re.findall(r"^valid_accuracy (\S+)$", out, re.M)
    rob = re.findall(r"^robust_accuracy (\S+)$", out, re.M)
    assert len(clean) == 1 and len(rob) == 1 and lines[-1] == "robust_accuracy " + rob[0]
    assert re.fullmatch(r"\d+\.\d{3}", rob[0])
    assert float(rob[0]) <= float(clean[0])
    assert lines.index("valid_accuracy " + clean[0]) < lines.index(robust[0])        # after the clean pass
