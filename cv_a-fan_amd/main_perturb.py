"""A-FAN training entry point — same flags, stdout lines and output files as the reference's
Classification/main_perturb.py (flags :28-49, loop :97-150, train :153-225, validate :227-263), so
`bash cmd/run_perturb.sh` keeps working.  Additions (all optional): --arch, --dtype, --synthetic,
--max_iters; launched under torch.distributed.run it trains data parallel, one rank per MI355X.

What differs from the reference is execution only: the iteration body is train_step.AfanTrainer.step
(HIP kernels, no host sync), metrics stay on the device and are read back every --print_freq iterations,
the perturbation norms come out of the last PGD kernel instead of a host-side reduction.  The loops, the
checkpoint layout and the loaders are cls_entry.py's and cls_data.py's.
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_perturb.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    resnet_s, train_step = _pkg.resnet_s, _pkg.train_step
    cls_data, cls_entry = importlib.import_module("cv_a-fan_amd.cls_data"), importlib.import_module("cv_a-fan_amd.cls_entry")
else:
    from . import cls_data, cls_entry, resnet_s, train_step

parser = argparse.ArgumentParser(description="A-FAN CIFAR-10 training on MI355X")
cls_entry.add_base_flags(parser, save_dir="res56s_adv_aug")                # main_perturb.py:28-33
cls_entry.add_optimizer_flags(parser)                                      # main_perturb.py:36-41
# ---- A-FAN setting (main_perturb.py:44-49)
parser.add_argument("--steps", default=5, type=int, help="PGD-steps")
parser.add_argument("--perturb_idx", help="index of perturb layers", default=13, type=int)
parser.add_argument("--gamma", help="index of PGD gamma", default=1.5, type=float)
parser.add_argument("--eps", default=2, type=float)
parser.add_argument("--randinit", action="store_true", help="whether using randinit")
parser.add_argument("--clip", action="store_true", help="whether using clip")
cls_entry.add_addition_flags(parser, dual_bn=True)

validate = cls_entry.validate          # (main() looks it up here at call time: tools/diag_main.py stands in its own)
# what tests written before cls_data.py / cls_entry.py reach through this module: the same objects, not copies
AverageMeter, accuracy = cls_entry.AverageMeter, cls_entry.accuracy
DeviceLoader, SyntheticLoader = cls_data.DeviceLoader, cls_data.SyntheticLoader
_augment_torch, _load_cifar10_test = cls_data._augment_torch, cls_data._load_cifar10_test


def main(argv=None):
    args = parser.parse_args(argv)
    dev, rank, world, placement, log = cls_entry.setup("main_perturb.py", args.gpu, distributed=True)
    log(args)
    log("host placement:", cls_entry.shown_placement(placement))
    if args.seed:
        cls_entry.setup_seed(args.seed)
    cls_entry.check_arch(args)
    ctor, _ = resnet_s.ARCHS[args.arch]
    model = cls_entry.prepare_model(ctor(), args, dev)       # constructed after seeding, on the host generator, like main_perturb.py:64
    criterion = nn.CrossEntropyLoss()
    trainer = train_step.AfanTrainer(model, criterion, steps=args.steps, gamma=args.gamma, eps=args.eps,
                                     perturb_idx=args.perturb_idx, layer_number=model.layer_number, randinit=args.randinit,
                                     clip=args.clip, lr=args.lr, momentum=args.momentum,
                                     weight_decay=args.weight_decay, dual_bn=args.dual_bn)
    cls_entry.log_general_convs(model, log)
    decreasing_lr = list(map(int, args.decreasing_lr.split(",")))
    scheduler = torch.optim.lr_scheduler.MultiStepLR(trainer.optimizer, milestones=decreasing_lr, gamma=0.1)
    loaders = cls_entry.build_loaders(args, dev, rank, world)
    cls_entry.run_epochs(args, dev, rank, log, model, criterion, trainer, {"optimizer": trainer.optimizer}, scheduler, loaders,
                         lambda *a: validate(*a), norms="cat")
    cls_entry.close(world)


if __name__ == "__main__":
    main()
