"""Baseline training entry point — same flags, defaults, stdout lines and output files as the reference's
Classification/main_base.py (flags :28-41, loop :87-137, train :140-180), so `bash cmd/run_base.sh` works: the network every A-FAN
number is compared against, and the checkpoint main_inference.py's default --pretrained names.  Additions (all optional): --arch,
--dtype, --layout, --synthetic, --max_iters; launched under torch.distributed.run it trains data parallel, one rank per MI355X.

The iteration body is train_step.BaseTrainer.step (one train-mode forward, criterion, backward, one fused SGD launch; captured and
replayed as a hipGraph); metrics stay on the device and are read back every --print_freq iterations.  Data loading, validation
(infer.Evaluator), the meters and the seeding are main_perturb.py's.  No perturbation, so no `l2 mean` / `linf mean` lines and no
result_norm.pkl."""
import argparse
import os
import pickle
import sys

import torch
import torch.distributed as dist
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_base.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    resnet_s, train_step, host, mp = _pkg.resnet_s, _pkg.train_step, _pkg.host, importlib.import_module("cv_a-fan_amd.main_perturb")
else:
    from . import host, resnet_s, train_step
    from . import main_perturb as mp

parser = argparse.ArgumentParser(description="Baseline CIFAR-10 training on MI355X")
# ---- base setting (main_base.py:28-33)
parser.add_argument("--data", type=str, default="../data", help="location of the data corpus (cifar-10-batches-py)")
parser.add_argument("--print_freq", default=50, type=int, help="print frequency")
parser.add_argument("--seed", default=None, type=int, help="random seed")
parser.add_argument("--gpu", type=int, default=0, help="gpu device id")
parser.add_argument("--resume", action="store_true", help="resume from checkpoint")
parser.add_argument("--save_dir", help="The directory used to save the trained models", default="res56s_cifar10_baseline", type=str)
# ---- optimizer setting (main_base.py:36-41)
parser.add_argument("--batch_size", type=int, default=128, help="batch size (global; split across ranks)")
parser.add_argument("--lr", default=0.1, type=float, help="initial learning rate")
parser.add_argument("--momentum", default=0.9, type=float, help="momentum")
parser.add_argument("--weight_decay", default=5e-4, type=float, help="weight decay")
parser.add_argument("--epochs", default=200, type=int, help="number of total epochs to run")
parser.add_argument("--decreasing_lr", default="50,150", help="decreasing strategy")
# ---- additions
parser.add_argument("--arch", default="resnet56s", choices=sorted(resnet_s.ARCHS))
parser.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="backbone compute dtype")
parser.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"],
                    help="internal activation / weight layout (nhwc: the library's MFMA convolutions; nchw: the general fp32-arithmetic kernels)")
parser.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images instead of CIFAR-10")
parser.add_argument("--max_iters", type=int, default=0, help="stop each epoch after this many iterations (0 = all)")


def train(train_loader, trainer, optimizer, epoch, args, log):
    """main_base.py:140-180.  Device-side accumulation; one read-back per print_freq iterations, in iteration order, so the printed
    values are those of the per-batch reads."""
    losses, top1 = mp.AverageMeter(), mp.AverageMeter()
    trainer.model.train()
    wp_steps = len(train_loader)
    pending = []

    def flush():
        # (the host reads results here anyway: every step issued so far is verified against a given-up grid barrier of the in-launch
        # BatchNorm, and run again on the two-launch forms if one did — grid_guard.GuardedTrainer.flush_guard)
        if trainer.flush_guard():
            log("in-launch BatchNorm: a grid barrier gave up; the affected steps were run again on the two-launch forms "
                "(their logged loss / accuracy values are invalid)")
        for loss_t, prec_t, n in pending:
            losses.update(loss_t.item(), n)
            top1.update(prec_t.item(), n)
        pending.clear()

    for i, (inp, target) in enumerate(train_loader):
        if args.max_iters and i >= args.max_iters:
            break
        if epoch == 0:
            train_step.warmup_lr(i, optimizer, warm_up_steps=wp_steps, max_lr=args.lr)
        r = trainer.step(inp, target)
        pending.append((r["loss"], r["prec1"], inp.size(0)))
        if i % args.print_freq == 0:
            flush()
            log("Epoch: [{0}][{1}/{2}]\t"
                "Loss {loss.val:.4f} ({loss.avg:.4f})\t"
                "Accuracy {top1.val:.3f} ({top1.avg:.3f})\t".format(epoch, i, len(train_loader), loss=losses, top1=top1))
    flush()
    log("train_accuracy {top1.avg:.3f}".format(top1=top1))
    return top1.avg, losses.avg


def main(argv=None):
    args = parser.parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(args.gpu)))
    placement = host.place_rank(local)         # this rank's threads on one block of cores of its GPU's NUMA node (before the GPU is touched)
    if not torch.cuda.is_available():
        raise RuntimeError("main_base.py needs an MI355X: this build has no CPU path (oracle/ is test infrastructure)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)

    def log(*a):
        if rank == 0:
            print(*a, flush=True)

    log(args)
    log("host placement:", {k: v for k, v in placement.items() if k != "restore"})
    if args.seed:
        mp.setup_seed(args.seed)
    if args.arch == "resnet50" and not args.synthetic:
        raise SystemExit("--arch resnet50 is the ImageNet-shape synthetic configuration: pass --synthetic N")
    ctor, _ = resnet_s.ARCHS[args.arch]
    model = ctor()                      # constructed after seeding, on the host generator, like main_base.py:56
    model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model.set_channels_last(args.layout == "nhwc").to(dev)
    criterion = nn.CrossEntropyLoss()
    trainer = train_step.BaseTrainer(model, criterion, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    optimizer = trainer.optimizer
    vendor = resnet_s.general_convs(model)
    log("convolutions outside the library's kernels: {}{}".format(
        len(vendor), " (general f32-MFMA kernels; --dtype bf16 --layout nhwc is the tuned bf16 MFMA path)" if vendor else ""))
    decreasing_lr = list(map(int, args.decreasing_lr.split(",")))
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=decreasing_lr, gamma=0.1)

    if args.synthetic:
        side, classes = (224, 1000) if args.arch == "resnet50" else (32, 10)
        train_loader = mp.SyntheticLoader(args.synthetic, args.batch_size, dev, rank, world, side=side, classes=classes)
        val_loader = test_loader = mp.SyntheticLoader(max(args.synthetic // 10, args.batch_size), args.batch_size, dev,
                                                      side=side, classes=classes)
    else:
        tr, va, te = mp._load_cifar10(args.data)
        shared = torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64)     # rank 0's draw (seeded or not) for everyone
        if world > 1:
            shared = shared.to(dev)
            dist.broadcast(shared, src=0)
        train_loader = mp.DeviceLoader(tr[0], tr[1], args.batch_size, dev, True, rank, world, seed=int(shared.item()))
        val_loader = mp.DeviceLoader(va[0], va[1], args.batch_size, dev, False, drop_last=False)
        test_loader = mp.DeviceLoader(te[0], te[1], args.batch_size, dev, False, drop_last=False)

    best_prec1, start_epoch = 0, 0
    if args.resume:
        log("resume from checkpoint")
        ck = torch.load(os.path.join(args.save_dir, "checkpoint.pt"), map_location=dev)
        best_prec1, start_epoch = ck["best_prec1"], ck["epoch"]
        model.load_state_dict(ck["state_dict"])
        trainer.arena.refresh_shadow()
        optimizer.load_state_dict(ck["optimizer"])
        scheduler.load_state_dict(ck["scheduler"])

    all_result, train_acc, ta, test_ta = {}, [], [], []
    os.makedirs(args.save_dir, exist_ok=True)
    for epoch in range(start_epoch, args.epochs):
        log(optimizer.state_dict()["param_groups"][0]["lr"])
        acc, _ = train(train_loader, trainer, optimizer, epoch, args, log)
        tacc, _ = mp.validate(val_loader, model, criterion, args, log)
        test_tacc, _ = mp.validate(test_loader, model, criterion, args, log)
        scheduler.step()
        train_acc.append(acc), ta.append(tacc), test_ta.append(test_tacc)
        is_best = tacc > best_prec1
        best_prec1 = max(tacc, best_prec1)
        if rank == 0:
            state = {"epoch": epoch + 1, "state_dict": model.state_dict(), "best_prec1": best_prec1,
                     "optimizer": optimizer.state_dict(), "scheduler": scheduler.state_dict()}
            if is_best:
                torch.save(state, os.path.join(args.save_dir, "best_model.pt"))
            torch.save(state, os.path.join(args.save_dir, "checkpoint.pt"))
            try:
                import matplotlib
                matplotlib.use("Agg")
                import matplotlib.pyplot as plt
                plt.plot(train_acc, label="train_acc"), plt.plot(ta, label="TA"), plt.plot(test_ta, label="test_TA")
                plt.legend()
                plt.savefig(os.path.join(args.save_dir, "net_train.png"))
                plt.close()
            except ImportError:
                pass
            all_result.update(train=train_acc, test_ta=test_ta, ta=ta)
            pickle.dump(all_result, open(os.path.join(args.save_dir, "result.pkl"), "wb"))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
