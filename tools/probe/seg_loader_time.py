"""What a segmentation training batch costs: the one-launch loader (ops.seg_batch_aug) at the workload's shape — 2 and 8 images of
513 x 513 from sources of about 375 x 500 — against the same batch built by Pillow on the host, and against the SegTrainer step it
feeds.  Device times are HIP-event times over many back-to-back launches after a warm-up (the launch is far below the event
resolution of a single call), medians of 5 repeats; the host time is wall clock for one batch on one thread.  Appends one JSON line
per batch size to profiles/seg_loader_time.jsonl.

    python tools/probe/seg_loader_time.py [--no_step]
"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


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
    return statistics.median(out), min(out), max(out)


def pillow_batch_ms(images, labels, params, crop):
    try:
        from PIL import Image, ImageOps  # noqa: F401
    except ImportError:
        return None
    spec = importlib.util.spec_from_file_location("gen", os.path.join(ROOT, "tools", "gen_seg_aug_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    t0 = time.perf_counter()
    for k, oh, ow, top, left, flip in params.T:
        a, b = gen.pillow_augment(images[k], labels[k], int(oh), int(ow), int(top), int(left), int(flip), crop, crop)
        torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255), torch.from_numpy(b.astype(np.int64))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_loader_time.jsonl"))
    args = ap.parse_args()
    pkg = importlib.import_module("cv_a-fan_amd")
    dev = torch.device("cuda:0")
    crop = 513
    split = pkg.seg_data.SyntheticSegSplit(32, seed=1, min_side=375, max_side=500)
    for batch in (2, 8):
        loader = pkg.seg_data.SegDeviceLoader(split.images, split.labels, batch, dev, True, crop, seed=3)
        it = iter(loader)
        x, y = next(it)
        p = torch.from_numpy(loader.last_params[:, :batch].copy()).to(dev)

        def launch():
            pkg.ops.seg_batch_aug(loader.images, loader.offsets, loader.labels, loader.d_hs, loader.d_ws, p[0], p[1], p[2], p[3], p[4],
                                  p[5], crop, crop, loader.max_shrink)
        med, lo, hi = device_ms(launch, 50)
        rec = {"probe": "seg_loader_time", "device": torch.cuda.get_device_name(0), "batch": batch, "crop": crop,
               "sources": "32 synthetic images, sides 375..500", "scales": [float(v) for v in (loader.last_params[1, :batch] /
                                                                                              loader.hs[loader.last_params[0, :batch]])],
               "launch_ms_median": round(med, 4), "launch_ms_min": round(lo, 4), "launch_ms_max": round(hi, 4), "launches_per_batch": 1,
               "pillow_host_ms_one_thread": pillow_batch_ms(split.images, split.labels, loader.last_params[:, :batch], crop)}
        if not args.no_step and batch == 2:
            model = pkg.deeplab.MODELS["deeplabv3plus_resnet101"](num_classes=21, output_stride=16)
            model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
            tr = pkg.seg_trainer.SegTrainer(model, steps=3, eps=2.0, gamma_se=0.5, gamma_sd=0.5, pertub_idx_se=3, pertub_idx_sd="aspp",
                                            mix_layer="11", mix_sd=True, lr=0.01)
            s_med, s_lo, s_hi = device_ms(lambda: tr.step(x, y), 10, repeats=3, warm=4)
            rec.update(step="deeplabv3plus_resnet101 K=3 bf16 nhwc", step_ms_median=round(s_med, 3), step_ms_min=round(s_lo, 3),
                       step_ms_max=round(s_hi, 3))
            del tr, model
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
