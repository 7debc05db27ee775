"""What the end of the image attack and the random start cost Detection PGD training (train_baseline_advtrain.py), and what the one
launch (afan_pgd_step_clamp, pgd.step(clamp=(0, 1))) and the device-drawn start change:

  (a) the last step alone at 1 x 3 x 600 x 904 and 8 x 3 x 600 x 904 (fp32 iterate, fp32 gradient, clip): the fused launch against
      pgd.step + pgd.clamp01_ (the step, two fills, afan_tensor_clamp), each behind the same restoring copy of the iterate;
  (b) one DetTrainer(phases="adv") step (--steps 1 --randinit --clip) on Faster-RCNN / ResNet-101 with untrained weights, bf16
      channels-last, 600 x 904, at batch 1 and at the README's batch 8: noise host, host with noise_ahead, device, each with
      det_attack_algo.ADV_FUSED_CLAMP on and off (learning rate 0: every window sees the same weights).

HIP events round a window of back-to-back calls and wall clock round the same window ending in a synchronise, nothing read back
inside a window, the median of 7 repeats taken alternately over the arms, min and max reported (tools/probe/det_eval_time.py's
protocol).  Appends JSON lines to profiles/det_adv_time.jsonl; each record carries, per decision, `gain_ms` (wall medians),
`spread_ms` (the two arms' min-max spreads added) and `switch_on` = gain > spread, the project's rule for every switch.

    python tools/probe/det_adv_time.py [--no_model] [--batches 1 8] [--out FILE]
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

W, H = 904, 600
GAMMA, EPS = 0.5 / 255, 2.0 / 255


def verdict(r, on, off):
    gain = r[off]["wall_ms_median"] - r[on]["wall_ms_median"]
    spread = (r[on]["wall_ms_max"] - r[on]["wall_ms_min"]) + (r[off]["wall_ms_max"] - r[off]["wall_ms_min"])
    return {"on": on, "off": off, "gain_ms": round(gain, 4), "spread_ms": round(spread, 4), "switch_on": bool(gain > spread),
            "ratio_wall_off_over_on": round(r[off]["wall_ms_median"] / r[on]["wall_ms_median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_model", action="store_true", help="(a) only")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_adv_time.jsonl"))
    args = ap.parse_args()
    pkg = importlib.import_module("cv_a-fan_amd")
    if not torch.cuda.is_available():
        raise RuntimeError("det_adv_time.py times HIP kernels: it needs an MI355X")
    dev = torch.device("cuda:0")
    ops, pgd, aa = pkg.ops, pkg.pgd, pkg.det_attack_algo
    name = torch.cuda.get_device_name(0)
    out = args.out
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    # ---- (a) the last step alone
    for batch in args.batches:
        g = torch.Generator().manual_seed(batch)
        x = torch.rand(batch, 3, H, W, generator=g).to(dev)
        x0 = (x + EPS * (2 * torch.rand(x.shape, generator=g).to(dev) - 1)).contiguous()
        grad = torch.randn(x.shape, generator=g).to(dev)
        xa = x0.clone()

        def fused():
            xa.copy_(x0)
            pgd.step(xa, grad, GAMMA, x, EPS, True, clamp=(0.0, 1.0))

        def composed():
            xa.copy_(x0)
            pgd.step(xa, grad, GAMMA, x, EPS, True)
            pgd.clamp01_(xa)

        def copy_only():
            xa.copy_(x0)
        fused()
        a = xa.clone()
        composed()
        assert torch.equal(a, xa)
        r = alternately({"fused": fused, "composed": composed, "copy_only": copy_only}, 20, 5)
        n = x.numel()
        emit({"probe": "det_adv_time", "arm": "a", "what": "last image-PGD step + clamp to [0, 1], fp32 {} x 3 x {} x {}, fp32 gradient, clip; "
              "each call behind the same restoring copy (copy_only: the copy alone)".format(batch, H, W), "device": name, "batch": batch,
              "calls_per_window": 20, "repeats": REPEATS, "algorithmic_bytes_fused": n * 16, "algorithmic_bytes_composed": n * 40,
              "fused_GBps_event_less_copy": round(n * 16 / max(r["fused"]["event_ms_median"] - r["copy_only"]["event_ms_median"], 1e-6) * 1e-6, 1),
              **r, "decision_fused_clamp": verdict(r, "fused", "composed")})
        del x, x0, grad, xa, a

    # ---- (b) one training step on the full model
    if not args.no_model:
        torch.manual_seed(3)
        model = pkg.det_model.fasterrcnn_resnet101(21, pooler_mode="align")
        for blk in model.modules():
            if isinstance(blk, pkg.det_model.Bottleneck):
                blk.bn3.weight.data.mul_(0.2)
        model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
        arena = None
        ops.noise_state(dev)
        for batch in args.batches:
            x = torch.rand(batch, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
            bb = torch.tensor([[[40., 60., 400., 500.], [300., 100., 800., 420.], [500., 30., 620., 200.]]], device=dev).repeat(batch, 1, 1).contiguous()
            lb = torch.tensor([[3, 8, 15]], device=dev).repeat(batch, 1).contiguous()
            trainers = {}
            for mode, noise, ahead in (("host", "host", False), ("host_ahead", "host", True), ("device", "device", False)):
                tr = pkg.det_trainer.DetTrainer(model, lr=0.0, phases="adv", arena=arena, noise_ahead=ahead,
                                                adv=dict(steps=1, eps=2.0, gamma=0.5, randinit=True, clip=True, noise=noise))
                arena = tr.arena
                trainers[mode] = tr

            def arm(mode, on):
                tr = trainers[mode]

                def run():
                    aa.ADV_FUSED_CLAMP = on
                    tr.step(x, bb, lb)
                return run
            keep = aa.ADV_FUSED_CLAMP
            try:
                arms = {"{}_{}".format(m, "fused" if on else "composed"): arm(m, on) for m in trainers for on in (True, False)}
                r = alternately(arms, 2 if batch == 1 else 1, 2)
            finally:
                aa.ADV_FUSED_CLAMP = keep
            emit({"probe": "det_adv_time", "arm": "b", "what": "one DetTrainer(phases='adv') step, --steps 1 --randinit --clip, fasterrcnn_resnet101 bf16 "
                  "nhwc, untrained, {} x 3 x {} x {}, 3 boxes per image, lr 0".format(batch, H, W), "device": name, "batch": batch,
                  "calls_per_window": 2 if batch == 1 else 1, "repeats": REPEATS, **r,
                  "decision_fused_clamp": {m: verdict(r, m + "_fused", m + "_composed") for m in trainers},
                  "decision_noise_device": {"against_host": verdict(r, "device_composed", "host_composed"),
                                            "against_host_ahead": verdict(r, "device_composed", "host_ahead_composed")}})
            del trainers, x


if __name__ == "__main__":
    main()
