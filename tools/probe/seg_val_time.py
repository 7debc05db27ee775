"""What scoring one validation batch costs: the one-launch path (ops.seg_confusion_upsampled on the classifier's low-resolution logits)
against the path it replaces — deeplab.interpolate to the image size, max(dim=1)[1], .cpu() of predictions and labels, numpy's
_fast_hist — and against the eval-mode forward that produces the logits.  Shapes: 1 x 21 x 129 x 129 -> 513 x 513 (one image) and
4 x 21 x 129 x 129 -> 513 x 513 (--val_batch_size 4 at --crop_val, crop 513); forward: deeplabv3plus_resnet50, output stride 16,
bf16 channels-last, "low_res": True.

Times: `*_wall_ms` is a host clock around one batch's scoring ending in a device synchronise (the old path synchronises by itself,
in .cpu()); the two paths alternate inside every repeat.  `launch_device_ms` is a HIP-event time over many back-to-back launches.
Medians of the repeats, with min and max.  The two paths' matrices are compared before anything is timed.  Appends one JSON line per
shape to profiles/seg_val_time.jsonl.

    python tools/probe/seg_val_time.py [--no_forward] [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _stats(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def device_ms(fn, iters, repeats=5, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_forward", action="store_true")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_val_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("seg_val_time.py measures on an MI355X; there is nothing to time on a host")
    pkg = importlib.import_module("cv_a-fan_amd")
    dev = torch.device("cuda:0")
    c, lo_side, side = 21, 129, 513
    model = None
    if not args.no_forward:
        model = pkg.deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=c, output_stride=16)
        model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).eval()
    for n in (1, 4):
        gen = torch.Generator().manual_seed(n)
        logits = torch.randn((n, c, lo_side, lo_side), generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
        target = torch.randint(0, c, (n, side, side), generator=gen)
        target[torch.rand(target.shape, generator=gen) < 0.05] = 255
        target = target.to(dev)
        hist = torch.zeros(c * c, dtype=torch.int64, device=dev)

        def new():
            pkg.ops.seg_confusion_upsampled(logits, target, hist)

        def old():
            up = pkg.deeplab.interpolate(logits, (side, side))
            preds = up.max(dim=1)[1].cpu().numpy()
            return pkg.seg_eval._fast_hist(c, target.cpu().numpy().flatten(), preds.flatten())

        new()
        same = bool(np.array_equal(hist.cpu().numpy().reshape(c, c), old()))
        for _ in range(5):
            new(), old()
        w_new, w_old = [], []
        for _ in range(args.repeats):                                   # alternating, same process, same inputs
            w_new.append(wall_ms(new))
            w_old.append(wall_ms(old))
        rec = {"probe": "seg_val_time", "device": torch.cuda.get_device_name(0), "logits": [n, c, lo_side, lo_side],
               "labels": [n, side, side], "matrices_equal": same, "repeats": args.repeats,
               "new_wall_ms": _stats(w_new), "old_wall_ms": _stats(w_old),
               "launch_device_ms": _stats(device_ms(new, 200), 5), "launches_per_batch": 1}
        if model is not None:
            x = torch.rand((n, 3, side, side), generator=gen).to(dev)
            with torch.no_grad():
                def fwd():
                    return model({"x": x, "adv": None, "out_idx": 0, "flag": "clean", "low_res": True})
                out = fwd()
                assert isinstance(out, pkg.deeplab.LowResLogits) and tuple(out.logits.shape) == (n, c, lo_side, lo_side)
                rec["forward"] = "deeplabv3plus_resnet50 os16 bf16 nhwc eval, low_res"
                rec["forward_device_ms"] = _stats(device_ms(fwd, 10, repeats=5, warm=5), 3)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
