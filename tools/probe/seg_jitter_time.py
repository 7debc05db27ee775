"""What the Cityscapes batch costs.  One process, one JSON line appended to profiles/seg_jitter_time.jsonl:

  jitter_ms / plain_ms:  ops.seg_batch_aug_jitter (clear + statistics launch + batch launch) and ops.seg_batch_aug on the SAME draws at
                         the workload's shape — 4 crops of 768 x 768 from 1024 x 2048 sources — device events around `iters` calls and a
                         host clock around the same calls ending in a synchronise, the two alternating, `repeats` times after warm-up;
                         median, min and max.  jitter - plain is the price of the colour jitter itself.
  pillow_ms:             the same batch on the host: crop, ImageEnhance x 3 in the drawn order, flip, /255, per image in turn (what one
                         DataLoader worker of the reference does); "skipped" where Pillow is not importable.
  step_ms:               one seg_trainer.SegBaseTrainer step (DeepLabv3+ ResNet-50, 19 classes, bf16 channels-last, replayed graph) on a
                         batch of that shape, for scale.

Usage: python tools/probe/seg_jitter_time.py [--iters N] [--repeats R] [--out FILE] [--no-step]"""
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
afan = importlib.import_module("cv_a-fan_amd")
sd, ops = afan.seg_data, afan.ops

BATCH, CROP, SRC_H, SRC_W, N_SRC = 4, 768, 1024, 2048, 8


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn, iters):
    """(device ms, host wall ms) per call"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters, (time.perf_counter() - t0) * 1e3 / iters


def pillow_batch(images, p, order, fac):
    from PIL import Image, ImageEnhance
    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    out = []
    for k in range(p.shape[1]):
        im = Image.fromarray(images[p[0, k]], "RGB").crop((int(p[4, k]), int(p[3, k]), int(p[4, k]) + CROP, int(p[3, k]) + CROP))
        for op in sd.JITTER_ORDERS[order[k]]:
            im = enh[op](im).enhance(float(fac[op, k]))
        if p[5, k]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        out.append(torch.from_numpy(np.asarray(im, dtype=np.uint8).transpose(2, 0, 1).copy()).float().div(255))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_jitter_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_jitter_time.py measures on an MI355X; there is nothing to measure without one")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(N_SRC)]
    labels = [rng.integers(0, 19, (SRC_H, SRC_W), dtype=np.uint8) for _ in range(N_SRC)]
    loader = sd.SegDeviceLoader(images, labels, BATCH, dev, True, CROP, seed=1, jitter=(0.5, 0.5, 0.5), scale_range=(1, 1))
    p, _ = loader._draw()
    p = p[:, :BATCH]
    order, fac = (v[..., :BATCH] for v in loader._jitter_draw)
    d = [t for t in torch.from_numpy(p).to(dev)]
    d_order, d_fac = torch.from_numpy(order).to(dev), [t for t in torch.from_numpy(np.ascontiguousarray(fac)).to(dev)]
    ws = torch.empty(BATCH, dtype=torch.int64, device=dev)
    res = (loader.images, loader.offsets, loader.labels, loader.d_hs, loader.d_ws)

    def jitter():
        return ops.seg_batch_aug_jitter(*res, *d, d_order, *d_fac, CROP, CROP, loader.max_shrink, workspace=ws)

    def plain():
        return ops.seg_batch_aug(*res, *d, CROP, CROP, loader.max_shrink)

    want = sd._augment_jitter_numpy(images[p[0, 0]], labels[p[0, 0]], *p[1:, 0], order[0], fac[:, 0], CROP, CROP)
    got = jitter()
    assert np.array_equal(got[0][0].cpu().numpy(), want[0]) and np.array_equal(got[1][0].cpu().numpy(), want[1]), "kernel != restatement"
    for _ in range(a.warmup):
        jitter(), plain()
    rows = {"jitter": [], "plain": []}
    for _ in range(a.repeats):                                     # alternating, so that drift hits both alike
        rows["jitter"].append(timed(jitter, a.iters))
        rows["plain"].append(timed(plain, a.iters))
    rec = {"kind": "seg_jitter", "batch": BATCH, "crop": CROP, "source": [SRC_H, SRC_W], "iters": a.iters, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0)}
    for k, v in rows.items():
        rec[k + "_device_ms"], rec[k + "_wall_ms"] = spread([x[0] for x in v]), spread([x[1] for x in v])
    rec["jitter_minus_plain_device_ms"] = round(rec["jitter_device_ms"]["median"] - rec["plain_device_ms"]["median"], 4)
    try:
        import PIL
        ref = pillow_batch(images, p, order, fac)
        assert torch.equal(ref, got[0].cpu()), "Pillow's batch != the kernel's"
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            pillow_batch(images, p, order, fac)
            t.append((time.perf_counter() - t0) * 1e3)
        rec["pillow_ms"], rec["pillow_version"] = spread(t), PIL.__version__
    except ImportError:
        rec["pillow_ms"] = "skipped: Pillow is not importable here"
    if not a.no_step:
        torch.manual_seed(0)
        m = afan.deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=19, output_stride=16)
        m.set_compute_dtype(torch.bfloat16)
        m.set_channels_last(True).to(dev).train()
        tr = afan.seg_trainer.SegBaseTrainer(m, lr=0.1, total_itrs=1000)
        x, y = got[0].clone(), got[1].clone()
        for _ in range(tr.graph_warmup + 3):
            tr.step(x, y)
        tr.flush_guard()
        rec["step_graph"] = tr._graph is not None
        it = max(a.iters // 5, 5)
        rec["step_ms"] = spread([timed(lambda: tr.step(x, y), it)[0] for _ in range(3)])
        tr.flush_guard()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
