"""What one batch of segmentation validation costs with the eval-mode DeepLab on the frozen-BatchNorm forms (deeplab.FROZEN_EVAL) and
without them: one robust-validation batch (seg_eval.pgd_validate: steps_pgd = 3 forward + input-gradient passes, one scoring forward,
one scoring launch) and one clean batch (seg_eval.validate), 4 x 3 x 513 x 513, deeplabv3plus_resnet50, output stride 16, bf16
channels-last.  Off is the layer-by-layer path (every convolution and every BatchNorm its own autograd node): the same kernels, the
same bits — the two paths' confusion matrices are compared before anything is timed.  A third configuration rebuilds the frozen
coefficient blocks and launch plans at every call instead of keeping them (deeplab.COEF_CACHE = False).

Times: `wall_ms` is a host clock around the batch ending in a device synchronise, `device_ms` a HIP-event pair around the same call.
The configurations alternate inside every repeat, each with one untimed call after the switch (coefficient blocks and plans kept per
module belong to one configuration); medians of the repeats with min and max, and (max - min) as the spread.  Appends
one JSON line per (workload, configuration) to profiles/seg_pgd_val_time.jsonl.

    python tools/probe/seg_pgd_val_time.py [--repeats 7] [--steps_pgd 3] [--batch 4] [--side 513] [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = (("on", True, True), ("off", False, True), ("on_rebuild", True, False))       # (name, FROZEN_EVAL, COEF_CACHE)


def _stats(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd), "spread": round(max(v) - min(v), nd)}


def timed(fn):
    """-> (wall ms, device ms) of one call, both ending at the device's last kernel."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps_pgd", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--side", type=int, default=513)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_pgd_val_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("seg_pgd_val_time.py measures on an MI355X; there is nothing to time on a host")
    pkg = importlib.import_module("cv_a-fan_amd")
    deeplab, seg_eval = pkg.deeplab, pkg.seg_eval
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=21, output_stride=16)
    model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).eval()
    gen = torch.Generator().manual_seed(args.batch)
    x = torch.rand((args.batch, 3, args.side, args.side), generator=gen).to(dev)
    y = torch.randint(0, 21, (args.batch, args.side, args.side), generator=gen)
    y[torch.rand(y.shape, generator=gen) < 0.05] = 255
    loader = [(x, y.to(dev))]
    opts = types.SimpleNamespace(steps_pgd=args.steps_pgd, eps_pgd=8.0, gamma_pgd=2.0, randinit_pgd=False, clip_pgd=True, save_val_results=False)
    crit = nn.CrossEntropyLoss(ignore_index=255, reduction="mean")
    metrics = seg_eval.StreamSegMetrics(21, dev)
    work = {"pgd_validate": lambda: seg_eval.pgd_validate(opts, model, loader, dev, metrics, crit),
            "validate": lambda: seg_eval.validate(opts, model, loader, dev, metrics)}

    def configure(frozen, cache):
        deeplab.FROZEN_EVAL, deeplab.COEF_CACHE = frozen, cache

    keep = (deeplab.FROZEN_EVAL, deeplab.COEF_CACHE)
    try:
        records = []
        for name, fn in work.items():
            mats = {}
            for cfg, frozen, cache in CONFIGS:                             # warm every configuration; keep its matrix
                configure(frozen, cache)
                for _ in range(2):
                    fn()
                mats[cfg] = metrics.confusion_matrix
            same = all(np.array_equal(mats["off"], m) for m in mats.values())
            wall, devt = {c[0]: [] for c in CONFIGS}, {c[0]: [] for c in CONFIGS}
            for _ in range(args.repeats):                                  # alternating, same process, same inputs
                for cfg, frozen, cache in CONFIGS:
                    configure(frozen, cache)
                    fn()        # (untimed: a switch of configuration invalidates what the other one kept per module)
                    w, d = timed(fn)
                    wall[cfg].append(w)
                    devt[cfg].append(d)
            for cfg, frozen, cache in CONFIGS:
                records.append({"probe": "seg_pgd_val_time", "device": torch.cuda.get_device_name(0), "workload": name, "config": cfg,
                                "frozen_eval": frozen, "coef_cache": cache, "images": [args.batch, 3, args.side, args.side],
                                "steps_pgd": args.steps_pgd if name == "pgd_validate" else None,
                                "model": "deeplabv3plus_resnet50 os16 bf16 nhwc eval", "matrices_equal": same, "repeats": args.repeats,
                                "wall_ms": _stats(wall[cfg]), "device_ms": _stats(devt[cfg])})
    finally:
        configure(*keep)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in records:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
