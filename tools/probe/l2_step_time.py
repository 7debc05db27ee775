"""L2 PGD step time.  Three comparisons, each the median of 7 alternating repeats with the min-max, a repeat = one window of 50 calls
timed by HIP events (device time) and by the wall clock (around the window and its final synchronisation):

  1. afan_pgd_step_l2 against afan_pgd_step on the same tensors (fp32 gradient, clip, shadow) at 256 x 3 x 32 x 32,
     64 x 3 x 224 x 224 and 4 x 3 x 513 x 513;
  2. the same L2 step against the torch composition of the identical formula (the arm the kernel replaces);
  3. one 10-step Attacker.attack on ResNet-20s at batch 256 under each norm (graph replay).

One JSON line per record.  Usage: python tools/probe/l2_step_time.py [--out profiles/l2_step_time.jsonl]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
afan = importlib.import_module("cv_a-fan_amd")
ops = afan.ops

SHAPES = [(256, 3, 32, 32), (64, 3, 224, 224), (4, 3, 513, 513)]
WINDOW, REPEATS = 50, 7


def window(fn, calls=WINDOW):
    """(device ms, wall ms) per call over one window."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / calls
    return s.elapsed_time(e) / calls, wall


def alternate(arms, calls=WINDOW):
    """arms: {name: fn}.  REPEATS rounds, the arms in turn inside each; {name: {"dev_us": [median, min, max], "wall_us": [...]}}."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    got = {k: ([], []) for k in arms}
    for _ in range(REPEATS):
        for k, fn in arms.items():
            d, w = window(fn, calls)
            got[k][0].append(d * 1e3)
            got[k][1].append(w * 1e3)
    summ = lambda v: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]
    return {k: {"dev_us": summ(d), "wall_us": summ(w)} for k, (d, w) in got.items()}


def torch_l2_step(x_adv, grad, gamma, x, eps, shadow):
    """The formula of afan_pgd_step_l2 composed from torch operations, in place."""
    b = x_adv.shape[0]
    ng = grad.flatten(1).norm(dim=1).view(b, 1, 1, 1)
    a = torch.where(ng == 0, torch.zeros_like(ng), gamma / ng)
    x_adv.add_(a * grad)
    d = x_adv - x
    nd = d.flatten(1).norm(dim=1).view(b, 1, 1, 1)
    s = torch.where(nd > eps, eps / nd, torch.ones_like(nd))
    torch.where(nd > eps, x + d * s, x_adv, out=x_adv)
    shadow.copy_(x_adv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--skip_attack", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    eps, gamma = 0.5, 0.125
    for shape in SHAPES:
        torch.manual_seed(0)
        x = torch.rand(shape, device=dev)
        # half the samples start inside the ball, half outside (so the projection launch does half its work)
        dl = torch.randn(shape, device=dev)
        dl = dl / dl.flatten(1).norm(dim=1).view(-1, 1, 1, 1) * (eps * torch.where(torch.arange(shape[0], device=dev) % 2 == 0, 0.3, 3.0)).view(-1, 1, 1, 1)
        start = (x + dl).contiguous()
        grad = torch.randn(shape, device=dev)
        x_adv = start.clone()
        shadow = torch.empty_like(x_adv, dtype=torch.bfloat16)

        def l2():
            x_adv.copy_(start)
            ops.pgd_step_l2_(x_adv, grad, gamma, x, eps, True, shadow)

        def linf():
            x_adv.copy_(start)
            ops.pgd_step_(x_adv, grad, 2 / 255, x, 8 / 255, True, shadow)

        def composed():
            x_adv.copy_(start)
            torch_l2_step(x_adv, grad, gamma, x, eps, shadow)

        def reset():
            x_adv.copy_(start)

        r = alternate({"l2_step": l2, "sign_step": linf, "torch_l2": composed, "reset_copy": reset})
        n = x.numel()
        emit({"probe": "step", "shape": list(shape), "elements": n, "window": WINDOW, "repeats": REPEATS,
              "note": "every arm restores x_adv first (reset_copy: 8 B/elt); [median, min, max]", **r})

    if not a.skip_attack:
        torch.manual_seed(0)
        m = afan.resnet_s.ARCHS["resnet20s"][0]()
        m.set_compute_dtype(torch.bfloat16)
        m.set_channels_last(True).to(dev).eval()
        x = torch.rand(256, 3, 32, 32, device=dev)
        y = torch.randint(0, 10, (256,), device=dev)
        crit = nn.CrossEntropyLoss()
        ats = {"linf": afan.infer.Attacker(m, crit, 8 / 255, 2 / 255, 10), "l2": afan.infer.Attacker(m, crit, 0.5, 0.125, 10, norm="l2")}
        for at in ats.values():
            at.refresh()
        r = alternate({k: (lambda at=at: at.attack(x, y)) for k, at in ats.items()}, calls=10)
        emit({"probe": "attack", "arch": "resnet20s", "batch": 256, "steps": 10, "window": 10, "repeats": REPEATS,
              "fused": {k: at.fused for k, at in ats.items()}, **r})

    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
