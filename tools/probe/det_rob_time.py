"""What the image end of the backbone costs a robust evaluation of Detection (eval_rob_ori.py), and what the one-launch stem image
gradient (frozen.STEM_IMAGE_GRAD, afan_frozen_stem_image_grad) changes:

  (a) the stem's backward alone at 1 x 3 x 600 x 904 — from the gradient at the max pool's output to the fp32 image gradient — as the
      one launch of frozen._FrozenStemFn against the layer-by-layer chain (pool backward, affine backward, 1x1 MFMA problem into the
      bf16 column tensor, col2im, the normaliser's division, casts), both through autograd on a graph kept alive;
  (b) one image's 10-step attack (det_attack_algo.eval_PGD, eps 2 / 255, gamma 0.5 / 255, clip) plus its detection (the eval-mode
      forward and the host copy) on the full Faster-RCNN / ResNet-101 with untrained weights, bf16 channels-last, 600 x 904, 6000 / 300
      proposals, one ground-truth box list of 3, with the switch on and off.

HIP events round a window of back-to-back calls and wall clock round the same window ending in a synchronise, the median of 7 repeats
taken alternately over the two arms, min and max reported (tools/probe/det_eval_time.py's protocol).  Appends JSON lines to
profiles/det_rob_time.jsonl; each record carries `gain_ms` (wall medians), `spread_ms` (the two arms' min-max spreads added) and
`switch_on` = gain > spread, the project's rule for every switch.

    python tools/probe/det_rob_time.py [--no_attack] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from det_eval_time import REPEATS, alternately  # noqa: E402

W, H, STEPS = 904, 600, 10


def verdict(r, on="one_launch", off="chain"):
    gain = r[off]["wall_ms_median"] - r[on]["wall_ms_median"]
    spread = (r[on]["wall_ms_max"] - r[on]["wall_ms_min"]) + (r[off]["wall_ms_max"] - r[off]["wall_ms_min"])
    return {"gain_ms": round(gain, 4), "spread_ms": round(spread, 4), "switch_on": bool(gain > spread),
            "ratio_wall_chain_over_one_launch": round(r[off]["wall_ms_median"] / r[on]["wall_ms_median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_attack", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_rob_time.jsonl"))
    args = ap.parse_args()
    pkg = importlib.import_module("cv_a-fan_amd")
    if not torch.cuda.is_available():
        raise RuntimeError("det_rob_time.py times HIP kernels: it needs an MI355X")
    dev = torch.device("cuda:0")
    fz = pkg.frozen
    torch.manual_seed(3)
    model = pkg.det_model.fasterrcnn_resnet101(21, pooler_mode="align", rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300)
    for blk in model.modules():
        if isinstance(blk, pkg.det_model.Bottleneck):
            blk.bn3.weight.data.mul_(0.2)
    model.detection._proposal_class.weight.data.mul_(40.0)
    model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).eval()
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    recs = []

    # ---- (a) the stem's backward alone
    net, arms = model.features, {}
    for name, on in (("one_launch", True), ("chain", False)):
        leaf = x.clone().requires_grad_(True)
        with pkg.resnet_s.dgrad_only(), fz.stem_image_grad(on):
            y = net._stem(leaf)
        g = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)).to(dev).to(y.dtype).contiguous(memory_format=torch.channels_last)

        def backward(y=y, leaf=leaf, g=g):
            with pkg.resnet_s.dgrad_only():
                return torch.autograd.grad(y, leaf, g, retain_graph=True)[0]
        arms[name] = backward
    r = alternately(arms, 20, 5)
    recs.append({"probe": "det_rob_time", "what": "stem backward, 1 x 3 x 600 x 904: pooled gradient -> fp32 image gradient",
                 "device": torch.cuda.get_device_name(0), "calls_per_window": 20, "repeats": REPEATS, **r, **verdict(r)})

    # ---- (b) one image's attack + detection
    if not args.no_attack:
        bb = torch.tensor([[[40., 60., 400., 500.], [300., 100., 800., 420.], [500., 30., 620., 200.]]], device=dev)
        lb = torch.tensor([[3, 8, 15]], device=dev)

        def image(on):
            def run():
                with torch.enable_grad(), fz.stem_image_grad(on):
                    adv = pkg.det_attack_algo.eval_PGD(x=x, y={"bb": bb, "lb": lb}, model=model, steps=STEPS, eps=2.0 / 255, gamma=0.5 / 255,
                                                       clip=True)
                with torch.no_grad():
                    boxes, classes, probs, _ = model.eval().forward({"x": adv.detach(), "adv": None, "out_idx": None, "flag": "clean",
                                                                     "min_prob": 0.05})
                    return torch.cat([boxes, probs.unsqueeze(-1)], dim=1).cpu(), classes.cpu()
            return run
        before = pkg.ops.CALLS["frozen_stem_image_grad"]
        image(True)()
        assert pkg.ops.CALLS["frozen_stem_image_grad"] - before == STEPS
        r = alternately({"one_launch": image(True), "chain": image(False)}, 2, 2)
        recs.append({"probe": "det_rob_time", "what": "10-step eval_PGD + detection of one 600 x 904 image, fasterrcnn_resnet101 bf16 nhwc, untrained",
                     "device": torch.cuda.get_device_name(0), "steps": STEPS, "calls_per_window": 2, "repeats": REPEATS, **r, **verdict(r)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for rec in recs:
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
