"""Eval forward time: the eager eval pass (model forward + criterion + accuracy, as validate ran it before infer.Evaluator) against
infer.Evaluator's graph replay, device events around N batches after warm-up.  One JSON line per configuration.
Usage: python tools/probe/eval_time.py [--iters N] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
afan = importlib.import_module("cv_a-fan_amd")

CONFIGS = [("resnet56s", 128, 32, 10), ("resnet20s", 128, 32, 10), ("resnet18", 256, 32, 10), ("resnet50", 64, 224, 1000)]


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
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
        crit = nn.CrossEntropyLoss()
        x = torch.rand(n, 3, side, side, device=dev)
        y = torch.randint(0, classes, (n,), device=dev)

        def eager():
            with torch.no_grad():
                out = m(x, end_point=m.layer_number, start_point=0)
                return crit(out, y).float(), afan.infer.accuracy(out.float(), y)

        ev = afan.infer.Evaluator(m, crit)
        ev.refresh()
        for _ in range(a.warmup):
            eager()
            ev.evaluate(x, y)
        t_eager = timed(eager, a.iters)
        t_ev = timed(lambda: ev.evaluate(x, y), a.iters)
        rec = {"arch": arch, "batch": n, "image": side, "eager_ms": round(t_eager, 4), "evaluator_ms": round(t_ev, 4),
               "speedup": round(t_eager / t_ev, 3), "graphs": len(ev._shapes._graphs)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
