"""What the detection tail of an eval-mode forward costs: Model.Detection.generate_detections with the one-launch tail
(det_ops.class_nms: softmax + afan_det_class_nms + afan_det_pack + one read of the counts) against the per-class loop it replaces
(AFAN_DET_CLASS_NMS=0: the decode over all classes, then per class a sort, afan_nms's three launches, a read-back and two gathers), at
the evaluation's shape — one image, 300 proposals (EvalConfig.RPN_POST_NMS_TOP_N), 21 classes — on random head outputs sharpened
enough that no list is empty; and one whole eval-mode forward of Faster-RCNN / ResNet-101 (bf16 channels-last, 600 x 904, 6000 / 300
proposals) with the switch on and off.

Both arms end in a host read, so a call is timed whole: HIP events round a window of back-to-back calls and wall clock round the same
window ending in a synchronise, the median of 7 repeats taken alternately over the two arms (tools/probe/det_loader_time.py's
protocol).  Appends JSON lines to profiles/det_eval_time.jsonl.

    python tools/probe/det_eval_time.py [--no_forward] [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
N, C, W, H, CALLS, REPEATS = 300, 21, 904, 600, 20, 7


def window_ms(fn, iters):
    """(HIP-event ms, wall-clock ms) per call over `iters` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, (time.perf_counter() - t0) * 1e3 / iters


def alternately(arms, iters, warm):
    for fn in arms.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in arms}
    for _ in range(REPEATS):                                   # alternately: a drift of the machine lands on both
        for k, fn in arms.items():
            times[k].append(window_ms(fn, iters))
    out = {}
    for k, ts in times.items():
        ev, wall = [t[0] for t in ts], [t[1] for t in ts]
        out[k] = {"event_ms_median": round(statistics.median(ev), 4), "event_ms_min": round(min(ev), 4), "event_ms_max": round(max(ev), 4),
                  "wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_eval_time.jsonl"))
    args = ap.parse_args()
    pkg = importlib.import_module("cv_a-fan_amd")
    if not torch.cuda.is_available():
        raise RuntimeError("det_eval_time.py times HIP kernels: it needs an MI355X")
    dev = torch.device("cuda:0")
    Model = pkg.det_model.Model
    recs = []

    def switch(on, fn):
        def run():
            Model.CLASS_NMS = on
            return fn()
        return run

    # ---- the tail alone
    g = torch.Generator().manual_seed(1)
    xy = torch.rand(1, N, 2, generator=g) * torch.tensor([W - 260., H - 260.])
    wh = torch.rand(1, N, 2, generator=g) * 220 + 40
    proposals = torch.cat([xy, xy + wh], dim=-1).to(dev)
    logits = (torch.randn(1, N, C, generator=g) * 3).to(dev)
    transformers = torch.randn(1, N, C * 4, generator=g).to(dev)
    det = Model.Detection("align", nn.Sequential(), 8, C, 1.0).to(dev).eval()
    tail = lambda: det.generate_detections(proposals, logits, transformers, W, H)
    Model.CLASS_NMS = True
    on = tail()
    Model.CLASS_NMS = False
    off = tail()
    assert all(torch.equal(a, b) for a, b in zip(on, off)), "the two arms disagree"
    counts = torch.bincount(on[1].long(), minlength=C)[1:]
    r = alternately({"one_launch": switch(True, tail), "per_class_loop": switch(False, tail)}, CALLS, 5)
    recs.append({"probe": "det_eval_time", "what": "generate_detections", "device": torch.cuda.get_device_name(0), "B": 1, "N": N, "C": C,
                 "detections": int(on[0].shape[0]), "smallest_list": int(counts.min()), "calls_per_window": CALLS, "repeats": REPEATS, **r,
                 "ratio_wall_loop_over_one_launch": round(r["per_class_loop"]["wall_ms_median"] / r["one_launch"]["wall_ms_median"], 3)})

    # ---- one whole eval-mode forward
    if not args.no_forward:
        torch.manual_seed(3)
        model = pkg.det_model.fasterrcnn_resnet101(21, pooler_mode="align", rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300)
        for blk in model.modules():
            if isinstance(blk, pkg.det_model.Bottleneck):
                blk.bn3.weight.data.mul_(0.2)
        model.detection._proposal_class.weight.data.mul_(40.0)
        model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).eval()
        x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)

        def forward():
            with torch.no_grad():
                return model({"x": x, "adv": None, "out_idx": None, "flag": "clean"})
        Model.CLASS_NMS = True
        n_det = int(forward()[0].shape[0])
        r = alternately({"one_launch": switch(True, forward), "per_class_loop": switch(False, forward)}, 5, 3)
        recs.append({"probe": "det_eval_time", "what": "eval forward, fasterrcnn_resnet101 bf16 nhwc, one 600 x 904 image, 6000 / 300 proposals",
                     "device": torch.cuda.get_device_name(0), "detections": n_det, "calls_per_window": 5, "repeats": REPEATS, **r,
                     "ratio_wall_loop_over_one_launch": round(r["per_class_loop"]["wall_ms_median"] / r["one_launch"]["wall_ms_median"], 3)})
    Model.CLASS_NMS = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for rec in recs:
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
