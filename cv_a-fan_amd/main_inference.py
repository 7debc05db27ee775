"""Checkpoint evaluation entry point — same flags, defaults and stdout lines as the reference's Classification/main_inference.py
(flags :28-32, main :38-53, validate :57-96), so `bash cmd/run_test.sh` works.  Additions (all optional): --arch, --dtype,
--layout, --synthetic, and robust accuracy: --attack_steps N (> 0: after the clean pass, an N-step L-inf PGD on every test image
through the eval-mode model, infer.Attacker; `Robust:` lines in the format of the `Test:` lines and a final `robust_accuracy` line),
--attack_eps, --attack_gamma (radius and step size in /255 pixel units), --attack_randinit, --attack_norm {linf,l2} (the threat
model; l2: normalised-gradient steps projected onto the L2 ball, eps and gamma are L2 lengths in the same /255 units, so the usual
CIFAR-10 L2 setting eps = 0.5 is --attack_eps 127.5).  --attack_steps 0 (the default) is the clean evaluation alone, its output
unchanged.

The checkpoint's `state_dict` is a main_perturb.py checkpoint's or one in the reference's layout (the same keys).  The
CIFAR-10 test split is evaluated in file order with its last partial batch; the evaluation is cls_entry.validate
(infer.Evaluator: one fused launch per convolution, per-batch results read back at --print_freq batches)."""
import argparse
import os
import sys

import torch
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_test.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    resnet_s, infer = _pkg.resnet_s, _pkg.infer
    cls_data, cls_entry = importlib.import_module("cv_a-fan_amd.cls_data"), importlib.import_module("cv_a-fan_amd.cls_entry")
else:
    from . import cls_data, cls_entry, infer, resnet_s

parser = argparse.ArgumentParser(description="A-FAN CIFAR-10 checkpoint evaluation on MI355X")
# ---- base setting (main_inference.py:28-32)
parser.add_argument("--data", type=str, default="../data", help="location of the data corpus (cifar-10-batches-py)")
parser.add_argument("--print_freq", default=50, type=int, help="print frequency")
parser.add_argument("--gpu", type=int, default=0, help="gpu device id")
parser.add_argument("--pretrained", help="pretrained_model", default="res56s_cifar10_baseline", type=str)
parser.add_argument("--batch_size", type=int, default=128, help="batch size")
cls_entry.add_addition_flags(parser, max_iters=False, synthetic_help="evaluate on N synthetic images instead of the CIFAR-10 test split")
# ---- robust accuracy (image-space L-inf PGD on the eval-mode model)
parser.add_argument("--attack_steps", type=int, default=0, help="PGD steps of the robust-accuracy pass (0: clean evaluation only)")
parser.add_argument("--attack_eps", type=float, default=8.0, help="L-inf radius of the attack, in /255 pixel units")
parser.add_argument("--attack_gamma", type=float, default=2.0, help="PGD step size, in /255 pixel units")
parser.add_argument("--attack_randinit", action="store_true", help="start the attack at a uniform random point of the eps-ball")
parser.add_argument("--attack_norm", choices=("linf", "l2"), default="linf",
                    help="threat model of the attack; l2: --attack_eps and --attack_gamma are L2 lengths, still in /255 pixel units "
                         "(eps = 0.5 is --attack_eps 127.5), and --attack_randinit starts on the eps-sphere")


def robust_validate(val_loader, model, criterion, args, log):
    """The robust counterpart of cls_entry.validate: every batch attacked (infer.Attacker), the adversarial loss and precision
    kept on the device and read back at --print_freq batches and at the end, in batch order."""
    model.eval()
    norm = getattr(args, "attack_norm", "linf")
    how = {} if norm == "linf" else {"norm": norm}          # (the L-inf attack is constructed as it always was)
    at = infer.Attacker(model, criterion, args.attack_eps / 255.0, args.attack_gamma / 255.0, args.attack_steps, args.attack_randinit, **how)
    at.refresh()
    return cls_entry.evaluate(val_loader, lambda inp, target: at.attack(inp, target)[1:], "Robust", "robust_accuracy", args, log)


def main(argv=None):
    args = parser.parse_args(argv)
    if args.attack_steps < 0:
        parser.error("--attack_steps must be >= 0")
    # (without an attack the printed namespace is the clean evaluation's own: the attack flags are not part of it)
    shown = args if args.attack_steps else argparse.Namespace(**{k: v for k, v in vars(args).items() if not k.startswith("attack_")})
    print(shown, flush=True)
    dev, _, _, _, log = cls_entry.setup("main_inference.py", args.gpu, place=False)
    cls_entry.check_arch(args)
    ctor, _ = resnet_s.ARCHS[args.arch]
    model = cls_entry.prepare_model(ctor(), args, dev)
    criterion = nn.CrossEntropyLoss()

    checkpoint = torch.load(args.pretrained, map_location=dev, weights_only=False)
    state = checkpoint["state_dict"]
    if any(".adv." in k for k in state):        # a --dual_bn checkpoint: the auxiliary sets load too, evaluation uses the main one
        resnet_s.enable_dual_bn(model)
    model.load_state_dict(state)

    if args.synthetic:
        side, classes = cls_entry.synthetic_shape(args)
        loader = cls_data.SyntheticLoader(args.synthetic, args.batch_size, dev, side=side, classes=classes)
    else:
        xt, yt = cls_data._load_cifar10_test(args.data)
        loader = cls_data.DeviceLoader(xt, yt, args.batch_size, dev, False, drop_last=False)

    cls_entry.validate(loader, model, criterion, args, log)
    if args.attack_steps:
        robust_validate(loader, model, criterion, args, log)


if __name__ == "__main__":
    main()
