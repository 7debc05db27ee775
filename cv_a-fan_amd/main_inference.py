"""Checkpoint evaluation entry point — same flags, defaults and stdout lines as the reference's Classification/main_inference.py
(flags :28-32, main :38-53, validate :57-96), so `bash cmd/run_test.sh` works.  Additions (all optional): --arch, --dtype,
--layout, --synthetic.

The checkpoint's `state_dict` is a main_perturb.py checkpoint's or one in the reference's layout (the same keys).  The
CIFAR-10 test split is evaluated in file order with its last partial batch; the evaluation is main_perturb.validate
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
    resnet_s, main_perturb = _pkg.resnet_s, importlib.import_module("cv_a-fan_amd.main_perturb")
else:
    from . import main_perturb, resnet_s

parser = argparse.ArgumentParser(description="A-FAN CIFAR-10 checkpoint evaluation on MI355X")
# ---- base setting (main_inference.py:28-32)
parser.add_argument("--data", type=str, default="../data", help="location of the data corpus (cifar-10-batches-py)")
parser.add_argument("--print_freq", default=50, type=int, help="print frequency")
parser.add_argument("--gpu", type=int, default=0, help="gpu device id")
parser.add_argument("--pretrained", help="pretrained_model", default="res56s_cifar10_baseline", type=str)
parser.add_argument("--batch_size", type=int, default=128, help="batch size")
# ---- additions
parser.add_argument("--arch", default="resnet56s", choices=sorted(resnet_s.ARCHS))
parser.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="backbone compute dtype")
parser.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"],
                    help="internal activation / weight layout (nhwc: the library's MFMA convolutions; nchw: the general fp32-arithmetic kernels)")
parser.add_argument("--synthetic", type=int, default=0, help="evaluate on N synthetic images instead of the CIFAR-10 test split")


def main(argv=None):
    args = parser.parse_args(argv)
    print(args, flush=True)
    if not torch.cuda.is_available():
        raise RuntimeError("main_inference.py needs an MI355X: this build has no CPU path (oracle/ is test infrastructure)")
    torch.cuda.set_device(int(args.gpu))
    dev = torch.device("cuda", int(args.gpu))
    if args.arch == "resnet50" and not args.synthetic:
        raise SystemExit("--arch resnet50 is the ImageNet-shape synthetic configuration: pass --synthetic N")
    ctor, _ = resnet_s.ARCHS[args.arch]
    model = ctor()
    model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model.set_channels_last(args.layout == "nhwc").to(dev)
    criterion = nn.CrossEntropyLoss()

    checkpoint = torch.load(args.pretrained, map_location=dev, weights_only=False)
    state = checkpoint["state_dict"]
    if any(".adv." in k for k in state):        # a --dual_bn checkpoint: the auxiliary sets load too, evaluation uses the main one
        resnet_s.enable_dual_bn(model)
    model.load_state_dict(state)

    if args.synthetic:
        side, classes = (224, 1000) if args.arch == "resnet50" else (32, 10)
        loader = main_perturb.SyntheticLoader(args.synthetic, args.batch_size, dev, side=side, classes=classes)
    else:
        xt, yt = main_perturb._load_cifar10_test(args.data)
        loader = main_perturb.DeviceLoader(xt, yt, args.batch_size, dev, False, drop_last=False)

    def log(*a):
        print(*a, flush=True)

    main_perturb.validate(loader, model, criterion, args, log)


if __name__ == "__main__":
    main()
