"""Baseline training entry point — same flags, defaults, stdout lines and output files as the reference's
Classification/main_base.py (flags :28-41, loop :87-137, train :140-180), so `bash cmd/run_base.sh` works: the network every A-FAN
number is compared against, and the checkpoint main_inference.py's default --pretrained names.  Additions (all optional): --arch,
--dtype, --layout, --synthetic, --max_iters; launched under torch.distributed.run it trains data parallel, one rank per MI355X.

The iteration body is train_step.BaseTrainer.step (one train-mode forward, criterion, backward, one fused SGD launch; captured and
replayed as a hipGraph); metrics stay on the device and are read back every --print_freq iterations.  The loops, the checkpoint
layout and the loaders are cls_entry.py's and cls_data.py's.  No perturbation, so no `l2 mean` / `linf mean` lines and no
result_norm.pkl."""
import argparse
import os
import sys

import torch
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_base.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    resnet_s, train_step, cls_entry = _pkg.resnet_s, _pkg.train_step, importlib.import_module("cv_a-fan_amd.cls_entry")
else:
    from . import cls_entry, resnet_s, train_step

parser = argparse.ArgumentParser(description="Baseline CIFAR-10 training on MI355X")
cls_entry.add_base_flags(parser, save_dir="res56s_cifar10_baseline")       # main_base.py:28-33
cls_entry.add_optimizer_flags(parser)                                      # main_base.py:36-41
cls_entry.add_addition_flags(parser)


def main(argv=None):
    args = parser.parse_args(argv)
    dev, rank, world, placement, log = cls_entry.setup("main_base.py", args.gpu, distributed=True)
    log(args)
    log("host placement:", cls_entry.shown_placement(placement))
    if args.seed:
        cls_entry.setup_seed(args.seed)
    cls_entry.check_arch(args)
    ctor, _ = resnet_s.ARCHS[args.arch]
    model = cls_entry.prepare_model(ctor(), args, dev)       # constructed after seeding, on the host generator, like main_base.py:56
    criterion = nn.CrossEntropyLoss()
    trainer = train_step.BaseTrainer(model, criterion, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    cls_entry.log_general_convs(model, log)
    decreasing_lr = list(map(int, args.decreasing_lr.split(",")))
    scheduler = torch.optim.lr_scheduler.MultiStepLR(trainer.optimizer, milestones=decreasing_lr, gamma=0.1)
    loaders = cls_entry.build_loaders(args, dev, rank, world)
    cls_entry.run_epochs(args, dev, rank, log, model, criterion, trainer, {"optimizer": trainer.optimizer}, scheduler, loaders,
                         cls_entry.validate)
    cls_entry.close(world)


if __name__ == "__main__":
    main()
