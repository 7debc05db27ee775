"""What a detection training batch costs: the one-launch loader (ops.det_batch_resize) at the workload's shape — 1 and 2 images of
600 x 904 from sources of 375 x 500, half of them mirrored, with their boxes — against the same batch built by the reference's Pillow
chain on one host thread (ImageOps.mirror, Image.resize, ToTensor, the box arithmetic, the collate function's padding), and against
the DetTrainer step it feeds (Faster-RCNN / ResNet-101, bf16 channels-last, one 600 x 904 image: what bench.py times).

Device times are HIP-event times over 50 back-to-back launches after a warm-up (one launch is far below the event resolution), the
median of 7 repeats taken alternately over the batch sizes; the host time is wall clock for one batch, the median of 7.  The sizes
are given to the kernel directly: preprocess_size of a 375 x 500 source is 600 x 800, and 600 x 904 is the size the step is timed at.
Appends one JSON line per batch size to profiles/det_loader_time.jsonl.

    python tools/probe/det_loader_time.py [--no_step]
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
OH, OW, CALLS, REPEATS = 600, 904, 50, 7


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def pillow_batch_ms(split, idx, flip, scale):
    """The reference's chain for one batch on this thread: voc2007.py:102-114, base.py:75-124."""
    try:
        from PIL import Image, ImageOps
    except ImportError:
        return None
    import torch.nn.functional as F
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ims, bbs = [], []
        for k, fl, sc in zip(idx, flip, scale):
            im = Image.fromarray(split.images[k], "RGB")
            bb = torch.from_numpy(split.boxes[k]).clone()
            if fl:
                im = ImageOps.mirror(im)
                bb[:, [0, 2]] = im.width - bb[:, [2, 0]]
            im = im.resize((OW, OH), Image.BILINEAR)
            ims.append(torch.from_numpy(np.asarray(im, dtype=np.uint8).transpose(2, 0, 1).copy()).float().div(255))
            bbs.append(bb * torch.tensor(float(sc)))
        g = max(len(b) for b in bbs)
        torch.stack([F.pad(i, (0, OW - i.shape[2], 0, OH - i.shape[1])) for i in ims])
        torch.stack([torch.cat([b, torch.zeros(g - len(b), 4)]) for b in bbs])
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_loader_time.jsonl"))
    args = ap.parse_args()
    pkg = importlib.import_module("cv_a-fan_amd")
    if not torch.cuda.is_available():
        raise RuntimeError("det_loader_time.py times a HIP kernel: it needs an MI355X")
    dev = torch.device("cuda:0")
    split = pkg.det_data.SyntheticDetSplit(16, seed=1, min_side=375, max_side=500)
    rng = np.random.default_rng(1)
    for k in range(len(split)):                                 # every source 375 x 500, three boxes of 60 to 260 pixels a side
        split.images[k] = rng.integers(0, 256, (375, 500, 3), dtype=np.uint8)
        xy = rng.integers(0, 110, (3, 2))
        split.boxes[k] = np.concatenate([xy, xy + rng.integers(60, 261, (3, 2))], axis=1).astype(np.float32)
        split.classes[k] = rng.integers(1, 21, 3).astype(np.int64)
    t = [torch.from_numpy(a).to(dev) for a in pkg.det_data.pack_det_split(split.images, split.boxes, split.classes)]
    g_max = max(len(b) for b in split.boxes)
    scale = np.float32(1.6)
    runs = {}
    for batch in (1, 2):
        idx = np.arange(batch, dtype=np.int64) + 3
        flip = (np.arange(batch) % 2 == 0).astype(np.int64)
        p = torch.from_numpy(np.stack([idx, np.full(batch, OH), np.full(batch, OW), flip]).astype(np.int64)).to(dev)
        s = torch.full((batch,), float(scale), device=dev)
        runs[batch] = (lambda p=p, s=s: pkg.ops.det_batch_resize(*t, p[0], p[1], p[2], p[3], s, OH, OW, g_max, 1.0), idx, flip)
    for fn, _, _ in runs.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {b: [] for b in runs}
    for _ in range(REPEATS):                                   # alternately: a drift of the machine lands on both
        for b, (fn, _, _) in runs.items():
            times[b].append(window_ms(fn, CALLS))
    step = {}
    if not args.no_step:
        torch.manual_seed(3)
        model = pkg.det_model.fasterrcnn_resnet101(21, pooler_mode="align")
        for blk in model.modules():
            if isinstance(blk, pkg.det_model.Bottleneck):
                blk.bn3.weight.data.mul_(0.2)
        model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
        tr = pkg.det_trainer.DetTrainer(model, lr=0.001, momentum=0.9, weight_decay=0.0005, loss_settings=1, noise_ahead=True)
        x, bb, lb = runs[1][0]()
        for _ in range(3):
            tr.step(x, bb, lb)
        torch.cuda.synchronize()
        ts = [window_ms(lambda: tr.step(x, bb, lb), 5) for _ in range(3)]
        step = dict(step="fasterrcnn_resnet101 bf16 nhwc, one 600 x 904 image", step_ms_median=round(statistics.median(ts), 3),
                    step_ms_min=round(min(ts), 3), step_ms_max=round(max(ts), 3))
    for b, (fn, idx, flip) in runs.items():
        rec = {"probe": "det_loader_time", "device": torch.cuda.get_device_name(0), "batch": b, "result": [OH, OW], "source": [375, 500],
               "flips": flip.tolist(), "g_max": g_max, "calls_per_window": CALLS, "repeats": REPEATS,
               "launch_ms_median": round(statistics.median(times[b]), 4), "launch_ms_min": round(min(times[b]), 4),
               "launch_ms_max": round(max(times[b]), 4), "launches_per_batch": 1,
               "pillow_host_ms_one_thread": pillow_batch_ms(split, idx, flip, [scale] * b)}
        if b == 1:
            rec.update(step)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
