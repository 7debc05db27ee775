"""What one iteration of Segmentation PGD training (seg_trainer.SegAdvTrainer, main_advtrain.py's loop) costs, and what drawing the
random start on the device buys: deeplabv3plus_resnet50, output stride 16, bf16 channels-last, one 4 x 3 x 513 x 513 batch,
--steps_pgd 1 --randinit_pgd --clip_pgd.  Arms, one trainer (and one model) each:

    host_eager      the start drawn by torch.rand on the CPU generator and uploaded, launches issued one by one — the only form a
                    random start allowed before afan_pgd_rand_start
    device_eager    the start drawn in its own launch, launches issued one by one
    device_graph    the same, the whole iteration replayed from one hipGraph (main_advtrain.py's default)
    norand_graph    no random start, replayed graph (the floor: what the start costs at all)

and the start alone, `calls` times in a row: ops.pgd_rand_start against clone + ops.axpy_noise_ with u already on the device
(`start_clone_axpy`) and against the whole host path — torch.rand, upload, clone, axpy_noise_ (`start_host_draw`).

Times: `wall_ms` is a host clock around `iters` iterations ending in a device synchronise, `device_ms` a HIP-event pair around the same
calls, both divided by `iters`.  The arms alternate inside every repeat; medians of the repeats with min and max, and (max - min) as
the spread.  Appends one JSON line per arm to profiles/seg_adv_time.jsonl.

    python tools/probe/seg_adv_time.py [--repeats 7] [--iters 3] [--batch 4] [--side 513] [--out FILE]
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

ARMS = (("host_eager", dict(randinit=True, noise="host", use_graph=False)),
        ("device_eager", dict(randinit=True, noise="device", use_graph=False)),
        ("device_graph", dict(randinit=True, noise="device", use_graph=True)),
        ("norand_graph", dict(randinit=False, noise="device", use_graph=True)))


def _stats(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd), "spread": round(max(v) - min(v), nd)}


def timed(fn, n):
    """-> (wall ms, device ms) per call of n calls, both ending at the device's last kernel."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, a.elapsed_time(b) / n


def measure(fns, repeats, n):
    wall, devt = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(repeats):                                            # alternating, same process, same inputs
        for k, fn in fns.items():
            w, d = timed(fn, n)
            wall[k].append(w)
            devt[k].append(d)
    return wall, devt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3, help="iterations per timed call")
    ap.add_argument("--calls", type=int, default=20, help="random starts per timed call")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--side", type=int, default=513)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_adv_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("seg_adv_time.py measures on an MI355X; there is nothing to time on a host")
    pkg = importlib.import_module("cv_a-fan_amd")
    deeplab, ops = pkg.deeplab, pkg.ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(args.batch)
    shape = (args.batch, 3, args.side, args.side)
    x = torch.rand(shape, generator=gen).to(dev)
    y = torch.randint(0, 21, (args.batch, args.side, args.side), generator=gen)
    y[torch.rand(y.shape, generator=gen) < 0.05] = 255
    y = y.to(dev)
    common = {"device": torch.cuda.get_device_name(0), "probe": "seg_adv_time", "images": list(shape), "repeats": args.repeats}

    trainers = {}
    for name, kw in ARMS:
        torch.manual_seed(0)
        model = deeplab.MODELS["deeplabv3plus_resnet50"](num_classes=21, output_stride=16)
        model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
        trainers[name] = pkg.seg_trainer.SegAdvTrainer(model, nn.CrossEntropyLoss(ignore_index=255, reduction="mean"), steps_pgd=1, eps_pgd=2.0,
                                                       gamma_pgd=0.5, clip=True, total_itrs=30000, graph_warmup=2, **kw)
    last = {}

    def stepper(name):
        def fn():
            last[name] = trainers[name].step(x, y)["loss"]
        return fn
    fns = {name: stepper(name) for name, _ in ARMS}
    for name, fn in fns.items():                                        # the eager iterations, the capture, one replay
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    graphs = {name: trainers[name]._graph is not None for name, _ in ARMS}
    wall, devt = measure(fns, args.repeats, args.iters)
    records = []
    for name, kw in ARMS:
        records.append(dict(common, workload="iteration", arm=name, randinit=kw["randinit"], noise=kw["noise"] if kw["randinit"] else None,
                            graph=graphs[name], steps_pgd=1, clip=True, model="deeplabv3plus_resnet50 os16 bf16 nhwc train",
                            iters_per_call=args.iters, last_loss=round(float(last[name]), 4), wall_ms=_stats(wall[name]),
                            device_ms=_stats(devt[name])))
    del trainers, fns
    torch.cuda.empty_cache()

    # ---- the start alone
    eps, u_dev = 2.0 / 255, torch.rand(shape, generator=gen).to(dev)
    starts = {"start_device_draw": lambda: ops.pgd_rand_start(x, eps),
              "start_clone_axpy": lambda: ops.axpy_noise_(x.clone(), u_dev, eps),
              "start_host_draw": lambda: ops.axpy_noise_(x.clone(), torch.rand(shape).to(dev, non_blocking=True), eps)}
    for fn in starts.values():
        fn()
    wall, devt = measure(starts, args.repeats, args.calls)
    for name in starts:
        records.append(dict(common, workload="start", arm=name, calls_per_call=args.calls, bytes=x.numel() * (8 if name == "start_device_draw" else 20),
                            wall_ms=_stats(wall[name], 4), device_ms=_stats(devt[name], 4)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in records:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
