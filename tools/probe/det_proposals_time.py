"""What the training-mode proposal layer costs for a batch: from the RPN's head outputs to the padded proposal block — decode + clip,
softmax, sort, NMS, rows — with det_ops.rpn_proposals (three launches for the whole batch) against the per-image loop it replaces
(per image a two-launch gather, afan_nms_top's memset / mask / scan / compact, afan_proposal_rows), kept here as
RegionProposalNetwork.forward_and_propose ran it before, at the Detection step's shape: the 38 x 57 x 9 anchors of a 600 x 904 image,
12 000 candidates, 2 000 proposals, random head outputs, B = 2, 4, 8.  Neither arm reads anything back.  And one DetTrainer step of
each new iteration (train_aug_final.py's README setting, train_baseline.py) on Faster-RCNN / ResNet-101, bf16 channels-last, batch 8,
with det_model.BATCH_PROPOSALS on and off.

HIP events round a window of back-to-back calls and wall clock round the same window ending in a synchronise, the median of 7
repeats taken alternately over the two arms, min and max reported (tools/probe/det_loader_time.py's protocol).  `wins`: both medians
(event and wall) of the new path are below the loop's by more than the two arms' combined min-max spread.  Appends JSON lines to
profiles/det_proposals_time.jsonl.

    python tools/probe/det_proposals_time.py [--no_step] [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H, FW, FH, PRE, POST, CALLS, REPEATS = 904, 600, 57, 38, 12000, 2000, 50, 7


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


def verdict(r, new, old):
    """new beats old by more than the two arms' combined min-max spread, on both clocks."""
    res = {}
    for clock in ("event", "wall"):
        gain = r[old][f"{clock}_ms_median"] - r[new][f"{clock}_ms_median"]
        spread = sum(r[k][f"{clock}_ms_max"] - r[k][f"{clock}_ms_min"] for k in (new, old))
        res[clock] = {"gain_ms": round(gain, 4), "combined_spread_ms": round(spread, 4), "wins": bool(gain > spread)}
    return {"verdict": res, "wins": res["event"]["wins"] and res["wall"]["wins"],
            "ratio_wall_loop_over_batched": round(r[old]["wall_ms_median"] / r[new]["wall_ms_median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_proposals_time.jsonl"))
    args = ap.parse_args()
    pkg = importlib.import_module("cv_a-fan_amd")
    if not torch.cuda.is_available():
        raise RuntimeError("det_proposals_time.py times HIP kernels: it needs an MI355X")
    dev = torch.device("cuda:0")
    dm, do = pkg.det_model, pkg.det_ops
    recs = []
    rpn = dm.RegionProposalNetwork(8, [(1, 2), (1, 1), (2, 1)], [128, 256, 512], PRE, POST, 1.0)
    anchors1 = rpn.generate_anchors(W, H, num_x_anchors=FW, num_y_anchors=FH).to(dev)
    A = anchors1.shape[0]
    assert A == FW * FH * 9

    # ---- the proposal layer alone
    for B in (2, 4, 8):
        g = torch.Generator().manual_seed(B)
        anchors = anchors1.repeat(B, 1, 1)
        objectnesses = torch.randn(B, A, 2, generator=g).to(dev)
        transformers = (torch.randn(B, A, 4, generator=g) * 0.2).to(dev)

        def front():
            boxes = do.box_decode_clip(anchors, transformers.float(), W, H)
            probs = F.softmax(objectnesses.float()[:, :, 1], dim=-1)
            _, order = torch.sort(probs, dim=-1, descending=True)
            return boxes, order

        def batched():
            boxes, order = front()
            return do.rpn_proposals(boxes, order, PRE, 0.7, POST)

        def loop():                                             # (forward_and_propose's loop as it ran before rpn_proposals)
            boxes, order = front()
            cand, keeps = [], []
            for b in range(anchors.shape[0]):
                sb = boxes[b][order[b][:PRE]]
                keeps.append(do.nms(sb, None, 0.7, max_keep=POST, presorted=True, padded=True))
                cand.append(sb)
            return do.proposal_rows(cand, keeps, POST)
        (pa, ka), (pb, kb) = batched(), loop()
        assert torch.equal(pa, pb) and torch.equal(ka, kb), "the two arms disagree"
        r = alternately({"batched": batched, "per_image_loop": loop}, CALLS, 5)
        recs.append({"probe": "det_proposals_time", "what": "head outputs -> padded proposals", "device": torch.cuda.get_device_name(0), "B": B,
                     "anchors": A, "pre_nms": PRE, "post_nms": POST, "kept": ka.tolist(), "calls_per_window": CALLS, "repeats": REPEATS, **r,
                     **verdict(r, "batched", "per_image_loop")})
        print(json.dumps(recs[-1]), flush=True)

    # ---- one trainer step of each new iteration at batch 8
    if not args.no_step:
        B = 8
        final = dict(pertub_idx_se=2, mix_layer="0011", gamma_se=1.0, gamma_sd=0.1, sd_adv_loss_weight=0.3, only_roi_sd=True)
        gen = torch.Generator().manual_seed(3)
        images = torch.rand(B, 3, H, W, generator=gen).to(dev)
        x0, y0 = torch.rand(B, 6, 1, generator=gen) * 640, torch.rand(B, 6, 1, generator=gen) * 340
        wh = 60 + torch.rand(B, 6, 2, generator=gen) * 200
        bboxes = torch.cat([x0, y0, x0 + wh[..., :1], y0 + wh[..., 1:]], dim=-1).to(dev)
        labels = torch.randint(1, 21, (B, 6), generator=gen).to(dev)
        for phases in ("final", "base"):
            torch.manual_seed(7)
            model = dm.fasterrcnn_resnet101(21, pooler_mode="align")
            for blk in model.modules():
                if isinstance(blk, dm.Bottleneck):
                    blk.bn3.weight.data.mul_(0.2)
            model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
            tr = pkg.det_trainer.DetTrainer(model, lr=1e-5, phases=phases, final=final if phases == "final" else None)

            def step(on):
                def run():
                    dm.BATCH_PROPOSALS = on
                    return tr.step(images, bboxes, labels)
                return run
            iters = 3 if phases == "final" else 6
            r = alternately({"batched": step(True), "per_image_loop": step(False)}, iters, 2)
            dm.BATCH_PROPOSALS = True
            recs.append({"probe": "det_proposals_time", "what": f"DetTrainer(phases={phases!r}).step, fasterrcnn_resnet101 bf16 nhwc, 600 x 904",
                         "device": torch.cuda.get_device_name(0), "B": B, "calls_per_window": iters, "repeats": REPEATS, **r,
                         **verdict(r, "batched", "per_image_loop")})
            print(json.dumps(recs[-1]), flush=True)
            del tr, model
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
