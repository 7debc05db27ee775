"""Baseline iteration and loader time.  Two kinds of JSON line:

  kind "step":   ms per iteration of train_step.BaseTrainer (bf16 channels-last, replayed hipGraph) beside AfanTrainer's K = 5 step at
                 the same shape — device events around `iters` iterations, `repeats` times after warm-up; median, min and max reported.
  kind "loader": ms per batch of cls_data.DeviceLoader iteration ALONE (a fake 45 000-image split), kernel path
                 (ops.batch_crop_flip) against the torch chain it replaced (_augment_torch, what the loader ran before) — host wall
                 clock with a final synchronise, and device time from events around the epoch; median, min and max over the repeats.

Usage: python tools/probe/base_time.py [--iters N] [--repeats R] [--out FILE] [--only step|loader]     (default FILE: profiles/base_time.jsonl;
profiles/base_README.md is the table written from it)"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
afan = importlib.import_module("cv_a-fan_amd")
mp = importlib.import_module("cv_a-fan_amd.cls_data")

STEP_CONFIGS = [("resnet20s", 128), ("resnet56s", 128), ("resnet18", 256)]


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def model_for(arch, dev):
    torch.manual_seed(0)
    m = afan.resnet_s.ARCHS[arch][0]()
    m.set_compute_dtype(torch.bfloat16)
    return m.set_channels_last(True).to(dev).train()


def steps(a, dev):
    for arch, n in STEP_CONFIGS:
        x, y = torch.rand(n, 3, 32, 32, device=dev), torch.randint(0, 10, (n,), device=dev)
        rec = {"kind": "step", "arch": arch, "batch": n}
        for name in ("base", "afan_k5"):
            m = model_for(arch, dev)
            if name == "base":
                tr = afan.train_step.BaseTrainer(m, nn.CrossEntropyLoss(), lr=0.01)
            else:
                tr = afan.train_step.AfanTrainer(m, nn.CrossEntropyLoss(), steps=5, gamma=0.5, eps=2.0,
                                                 perturb_idx=afan.resnet_s.ARCHS[arch][1], lr=0.01)
            for _ in range(a.warmup + tr.graph_warmup + 1):
                tr.step(x, y)
            torch.cuda.synchronize()
            assert tr._graph is not None, "the step did not capture"
            rec[name + "_ms"] = spread([timed(lambda: tr.step(x, y), a.iters) for _ in range(a.repeats)])
            del tr, m
        rec["afan_over_base"] = round(rec["afan_k5_ms"]["median"] / rec["base_ms"]["median"], 2)
        yield rec


class TorchChainLoader(mp.DeviceLoader):
    """DeviceLoader as it iterated before the kernel: per-batch index upload, gather, the _augment_torch chain."""

    def __iter__(self):
        perm = torch.randperm(self.x.shape[0]) if self.train else torch.arange(self.x.shape[0])
        for b in range(self.n_batches):
            idx = perm[b * self.batch:(b + 1) * self.batch].to(self.device)
            m = idx.shape[0]
            top = left = flip = None
            if self.train:
                top = torch.randint(0, 2 * self.pad + 1, (m,), device=self.device)
                left = torch.randint(0, 2 * self.pad + 1, (m,), device=self.device)
                flip = torch.rand(m, device=self.device) < 0.5
            yield mp._augment_torch(self.x[idx], top, left, flip, self.pad), self.y[idx]


def loaders(a, dev):
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (45000, 3, 32, 32), dtype=np.uint8)
    y = rng.integers(0, 10, 45000).astype(np.int64)
    for batch in (128, 256):
        rec = {"kind": "loader", "batch": batch, "images": 45000}
        for name, cls in (("kernel", mp.DeviceLoader), ("torch_chain", TorchChainLoader)):
            ld = cls(x, y, batch, dev, True)

            def epoch():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.record()
                for _ in ld:
                    pass
                e.record()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / len(ld), s.elapsed_time(e) / len(ld)
            epoch()                                                        # warm-up: allocator, first launches
            runs = [epoch() for _ in range(a.repeats)]
            rec[name + "_host_ms"] = spread([r[0] for r in runs])
            rec[name + "_device_ms"] = spread([r[1] for r in runs])
            del ld
        for clock in ("host", "device"):
            rec[f"{clock}_ratio"] = round(rec[f"torch_chain_{clock}_ms"]["median"] / rec[f"kernel_{clock}_ms"]["median"], 2)
        yield rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles",
                                                  "base_time.jsonl"))
    ap.add_argument("--only", default="", choices=["", "step", "loader"])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for kind, gen in (("step", steps), ("loader", loaders)):
        if a.only and a.only != kind:
            continue
        for rec in gen(a, dev):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
