"""Robust-accuracy attack time: the eager attack (infer.Attacker.attack_eager: the model's eval-mode forward and autograd per PGD
step) against infer.Attacker's graph replay, device events around N batches after warm-up.  One JSON line per configuration.
Usage: python tools/probe/attack_time.py [--iters N] [--steps K] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
afan = importlib.import_module("cv_a-fan_amd")

CONFIGS = [("resnet56s", 128, 32, 10), ("resnet20s", 128, 32, 10), ("resnet18", 256, 32, 10)]


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for arch, n, side, classes in CONFIGS:
        if a.only and arch != a.only:
            continue
        torch.manual_seed(0)
        m = afan.resnet_s.ARCHS[arch][0]()
        m.set_compute_dtype(torch.bfloat16)
        m.set_channels_last(True).to(dev).eval()
        x = torch.rand(n, 3, side, side, device=dev)
        y = torch.randint(0, classes, (n,), device=dev)
        at = afan.infer.Attacker(m, nn.CrossEntropyLoss(), 8 / 255, 2 / 255, a.steps)
        at.refresh()
        for _ in range(a.warmup):
            at.attack_eager(x, y)
            at.attack(x, y)
        t_eager = timed(lambda: at.attack_eager(x, y), a.iters)
        t_at = timed(lambda: at.attack(x, y), a.iters)
        rec = {"arch": arch, "batch": n, "image": side, "steps": a.steps, "eager_ms": round(t_eager, 4), "attacker_ms": round(t_at, 4),
               "speedup": round(t_eager / t_at, 3), "fused": at.fused, "graphs": len(at._shapes._graphs)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
