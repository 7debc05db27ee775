"""main_base.py (cmd/run_base.sh's entry point) end to end on the GPU: stdout formats, output files, the checkpoint through
main_inference.py, --resume."""
import os
import pickle
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
CWD = os.path.join(ROOT, "cv_a-fan_amd")


def _run(script, args):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-u", script] + args, cwd=CWD, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_train_checkpoint_evaluate_resume(pkg, gpu, tmp_path):
    save = str(tmp_path / "base")
    common = ["--seed", "3", "--save_dir", save, "--synthetic", "256", "--arch", "resnet20s", "--batch_size", "32", "--max_iters", "4",
              "--print_freq", "2"]
    out = _run("main_base.py", common + ["--epochs", "1"])
    lines = out.splitlines()
    assert lines[0].startswith("Namespace(") and "steps=" not in lines[0]
    assert "convolutions outside the library's kernels: 0" in out
    ep = re.compile(r"^Epoch: \[0\]\[(\d+)/8\]\tLoss \d+\.\d{4} \(\d+\.\d{4}\)\tAccuracy \d+\.\d{3} \(\d+\.\d{3}\)\t$")
    assert [int(ep.match(ln).group(1)) for ln in lines if ln.startswith("Epoch:")] == [0, 2]
    assert len(re.findall(r"^train_accuracy \d+\.\d{3}$", out, flags=re.M)) == 1
    assert len(re.findall(r"^valid_accuracy \d+\.\d{3}$", out, flags=re.M)) == 2          # validation and test split
    assert re.search(r"^Test: \[0/1\]\tLoss \d+\.\d{4} \(\d+\.\d{4}\)\tAccuracy \d+\.\d{3} \(\d+\.\d{3}\)$", out, flags=re.M)
    assert "l2 mean" not in out and "linf mean" not in out
    assert lines[lines.index("0.1") + 1].startswith("Epoch: [0][0/8]")                   # the learning-rate line opens the epoch
    ck = torch.load(os.path.join(save, "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "best_prec1", "optimizer", "scheduler"} and ck["epoch"] == 1
    assert len(ck["state_dict"]) == len(pkg.resnet_s.resnet20().state_dict())
    res = pickle.load(open(os.path.join(save, "result.pkl"), "rb"))
    assert set(res) == {"train", "test_ta", "ta"} and all(len(v) == 1 for v in res.values())
    assert not os.path.exists(os.path.join(save, "result_norm.pkl"))
    ev = _run("main_inference.py", ["--pretrained", os.path.join(save, "checkpoint.pt"), "--arch", "resnet20s", "--synthetic", "64",
                                    "--batch_size", "32", "--print_freq", "1"])
    assert "Test: [1/2]\tLoss" in ev and re.search(r"^valid_accuracy \d+\.\d{3}$", ev, flags=re.M)
    out2 = _run("main_base.py", common + ["--epochs", "2", "--resume"])
    assert "resume from checkpoint" in out2
    assert re.search(r"^Epoch: \[1\]\[0/8\]", out2, flags=re.M) and not re.search(r"^Epoch: \[0\]", out2, flags=re.M)
    assert torch.load(os.path.join(save, "checkpoint.pt"), map_location="cpu", weights_only=False)["epoch"] == 2
    assert len(pickle.load(open(os.path.join(save, "result.pkl"), "rb"))["train"]) == 1     # (the lists restart with the process)
