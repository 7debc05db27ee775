"""What the sample points cost a layer-wise SAT evaluation of Detection (eval_sat_layers.py), and what the one launch
(afan_sat_points_nhwc, ops.sat_points_block) and the ten-setting table change:

  (a) the launch alone: one 1 x 512 x 75 x 113 and one 1 x 1024 x 38 x 57 fp32 channels-last pair (the maps behind layer2 / layer3 of a
      600 x 904 image) to the ten bf16 outputs of the table, fused against the composed launches (one lerp_points, five mix_feature, ten
      casts: ops.sat_points(fused=False));
  (b) one image's ten-setting table (SatLayerEvaluator(table=True): one head pass, one 10-step feature PGD, one launch, ten eval tails
      with their host copies) on the full Faster-RCNN / ResNet-101 with untrained weights, bf16 channels-last, 600 x 904, 6000 / 300
      proposals, one ground-truth box list of 3, against ten single-setting passes (ten attacks);
  (c) one single-setting image (--sat_layer 2 --mix) with det_attack_algo.SAT_POINTS_FUSED on and off: the switch's own decision.

HIP events round a window of back-to-back calls and wall clock round the same window ending in a synchronise, the median of 7 repeats
taken alternately over the two arms, min and max reported (tools/probe/det_eval_time.py's protocol).  Appends JSON lines to
profiles/det_sat_time.jsonl; each record carries `gain_ms` (wall medians), `spread_ms` (the two arms' min-max spreads added) and
`switch_on` = gain > spread, the project's rule for every switch.

    python tools/probe/det_sat_time.py [--no_model] [--idx 2] [--out FILE]
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


def verdict(r, on, off):
    gain = r[off]["wall_ms_median"] - r[on]["wall_ms_median"]
    spread = (r[on]["wall_ms_max"] - r[on]["wall_ms_min"]) + (r[off]["wall_ms_max"] - r[off]["wall_ms_min"])
    return {"gain_ms": round(gain, 4), "spread_ms": round(spread, 4), "switch_on": bool(gain > spread),
            "ratio_wall_{}_over_{}".format(off, on): round(r[off]["wall_ms_median"] / r[on]["wall_ms_median"], 3)}


class _OneImage:
    """A loader of one prepared image: what SatLayerEvaluator iterates over."""
    train, batch, n = False, 1, 1

    def __init__(self, image, bb, lb):
        self.item, self.counts = (image, bb, lb, torch.ones(1, device=image.device)), [int(bb.shape[1])]

    def __iter__(self):
        yield self.item


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_model", action="store_true", help="(a) only")
    ap.add_argument("--idx", type=int, default=2, help="--pertub_idx of (b) and (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_sat_time.jsonl"))
    args = ap.parse_args()
    pkg = importlib.import_module("cv_a-fan_amd")
    if not torch.cuda.is_available():
        raise RuntimeError("det_sat_time.py times HIP kernels: it needs an MI355X")
    dev = torch.device("cuda:0")
    ops, aa, de = pkg.ops, pkg.det_attack_algo, pkg.det_eval
    name = torch.cuda.get_device_name(0)
    recs = []
    weights, mix = [j * (1.0 / 4) for j, _ in de.SAT_TABLE], [m for _, m in de.SAT_TABLE]

    # ---- (a) the launch alone
    for shape in ((1, 512, 75, 113), (1, 1024, 38, 57)):
        g = torch.Generator().manual_seed(shape[1])
        clean = torch.relu(torch.randn(shape, generator=g) * 0.5 + 0.7).to(dev).contiguous(memory_format=torch.channels_last)
        adv = (clean + (2.0 / 255) * (2 * torch.rand(shape, generator=g).to(dev) - 1)).contiguous(memory_format=torch.channels_last)
        fused = lambda c=clean, a=adv: ops.sat_points(c, a, weights, mix, torch.bfloat16)
        composed = lambda c=clean, a=adv: ops.sat_points(c, a, weights, mix, torch.bfloat16, fused=False)
        assert all(torch.equal(p, q) for p, q in zip(fused(), composed()))
        r = alternately({"fused": fused, "composed": composed}, 20, 5)
        nbytes = clean.numel() * (8 + 2 * 10)
        recs.append({"probe": "det_sat_time", "what": "ten bf16 (point, mix) outputs from one fp32 nhwc pair {} x {} x {} x {}".format(*shape),
                     "device": name, "calls_per_window": 20, "repeats": REPEATS, "algorithmic_bytes": nbytes,
                     "fused_GBps_event": round(nbytes / r["fused"]["event_ms_median"] * 1e-6, 1), **r, **verdict(r, "fused", "composed")})

    # ---- (b), (c) one image on the full model
    if not args.no_model:
        torch.manual_seed(3)
        model = pkg.det_model.fasterrcnn_resnet101(21, pooler_mode="align", rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300)
        for blk in model.modules():
            if isinstance(blk, pkg.det_model.Bottleneck):
                blk.bn3.weight.data.mul_(0.2)
        model.detection._proposal_class.weight.data.mul_(40.0)
        model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).eval()
        x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
        bb = torch.tensor([[[40., 60., 400., 500.], [300., 100., 800., 420.], [500., 30., 620., 200.]]], device=dev)
        lb = torch.tensor([[3, 8, 15]], device=dev)
        loader, gt = _OneImage(x, bb, lb), (["probe"], {})
        quiet = type("Quiet", (), {"i": staticmethod(lambda line: None)})()
        kw = dict(steps=STEPS, eps=2.0, gamma=0.5, pertub_idx=args.idx, clip=True, log=quiet)

        table = de.SatLayerEvaluator(loader, gt, table=True, **kw)
        singles = [de.SatLayerEvaluator(loader, gt, sat_layer=j, mix=m, **kw) for j, m in de.SAT_TABLE]
        before = ops.CALLS["sat_points"]
        rows = table.detect(model)
        assert ops.CALLS["sat_points"] - before == 1 and len(rows) == 10
        r = alternately({"table": lambda: table.detect(model), "ten_passes": lambda: [s.detect(model) for s in singles]}, 1, 1)
        recs.append({"probe": "det_sat_time", "what": "ten-setting table of one 600 x 904 image, fasterrcnn_resnet101 bf16 nhwc, untrained, "
                     "10-step feature PGD behind layer {}".format(args.idx), "device": name, "steps": STEPS, "pertub_idx": args.idx,
                     "calls_per_window": 1, "repeats": REPEATS, **r, **verdict(r, "table", "ten_passes")})

        single = de.SatLayerEvaluator(loader, gt, sat_layer=2, mix=True, **kw)

        def arm(on):
            def run():
                aa.SAT_POINTS_FUSED = on
                return single.detect(model)
            return run
        keep = aa.SAT_POINTS_FUSED
        try:
            r = alternately({"fused": arm(True), "composed": arm(False)}, 2, 1)
        finally:
            aa.SAT_POINTS_FUSED = keep
        recs.append({"probe": "det_sat_time", "what": "one single-setting image (--sat_layer 2 --mix), same model and attack, AFAN_DET_SAT_POINTS on / off",
                     "device": name, "steps": STEPS, "pertub_idx": args.idx, "calls_per_window": 2, "repeats": REPEATS, **r,
                     **verdict(r, "fused", "composed")})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for rec in recs:
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
