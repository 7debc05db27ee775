"""Learnable multi-layer A-FAN entry point — flags, stdout lines and output files of the reference's
Classification/main_learnable.py (flags :28-56, loop :110-170, train :175-277, sum_project :369-378); single GPU, like
the reference.  Additions (optional): --dtype, --synthetic, --max_iters.  The iteration body is
learnable.LearnableTrainer.step; the loops, the checkpoint layout and the loaders are cls_entry.py's and cls_data.py's."""
import argparse
import os
import sys

import torch
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script: import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    resnet_s, learnable, cls_entry = _pkg.resnet_s, _pkg.learnable, importlib.import_module("cv_a-fan_amd.cls_entry")
else:
    from . import cls_entry, learnable, resnet_s

parser = argparse.ArgumentParser(description="Learnable multi-layer A-FAN CIFAR-10 training on MI355X")
cls_entry.add_base_flags(parser, save_dir="res56s_aug_learnable", data_help="location of the data corpus")     # main_learnable.py:28-35
cls_entry.add_optimizer_flags(parser, batch_help="batch size")                                                 # :38-44
# ---- A-FAN setting (:47-56)
parser.add_argument("--steps", default=3, type=int, help="PGD-steps")
parser.add_argument("--gamma", help="index of PGD gamma", default=1, type=float)
parser.add_argument("--eps", default=2, type=float)
parser.add_argument("--randinit", action="store_true", help="whether using randinit")
parser.add_argument("--clip", action="store_true", help="whether using clip")
parser.add_argument("--w_lr", default=0.01, type=float, help="learning rate of the mixing weights")
parser.add_argument("--init_weight", default=(1 / 9), type=float, help="initial weight for ETA")
parser.add_argument("--l1_coef", default=1, type=float, help="coefficient of the L1 penalty on the mixing weights")
cls_entry.add_addition_flags(parser, arch=False)


def main(argv=None):
    args = parser.parse_args(argv)
    dev, rank, _, _, log = cls_entry.setup("main_learnable.py", args.gpu)
    log(args)
    if args.seed:
        cls_entry.setup_seed(args.seed)
    model = cls_entry.prepare_model(resnet_s.resnet56(init_weight_eta=args.init_weight), args, dev)       # :73
    criterion = nn.CrossEntropyLoss()
    trainer = learnable.LearnableTrainer(model, criterion, steps=args.steps, gamma=args.gamma, eps=args.eps,
                                         randinit=args.randinit, clip=args.clip, lr=args.lr, w_lr=args.w_lr,
                                         l1_coef=args.l1_coef, momentum=args.momentum, weight_decay=args.weight_decay)
    optimizer, optimizer_w = trainer.optimizer, trainer.optimizer_w
    cls_entry.log_general_convs(model, log)
    decreasing_lr = list(map(int, args.decreasing_lr.split(",")))
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=decreasing_lr, gamma=0.1)
    loaders = cls_entry.build_loaders(args, dev, shared_seed=False)

    def header(log, lr):
        for num in range(9):
            log("weight" + str(num + 1) + " = ", model.w[num].item())
        log(lr)
        log(optimizer_w.state_dict()["param_groups"][0]["lr"])

    cls_entry.run_epochs(args, dev, rank, log, model, criterion, trainer, {"optimizer": optimizer, "optimizer_w": optimizer_w},
                         scheduler, loaders, cls_entry.validate, norms="layers", plot=False, header=header)


if __name__ == "__main__":
    main()
