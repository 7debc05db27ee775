"""Segmentation A-FAN training entry point — the flags, defaults, stdout lines and checkpoint layout of the reference's
Segmentation/main_aug_final.py (flags args.py:14-105, loop :146-289), so `bash cmd/run_seg.sh` works.  Additions (all optional):
--dtype, --layout, --synthetic N, --max_side, --graph.

What differs from the reference is execution only: the iteration body is seg_trainer.SegTrainer.step (HIP kernels, replayed as a
hipGraph), the batch is built on the device by seg_data.SegDeviceLoader in one launch, and the loss stays on the device until the
`Epoch:[..], Itrs:[..], Loss:[..]` line needs it, every 10 iterations.

Validation (seg_eval.validate: one eager low-resolution forward and one scoring launch per batch) runs at every --val_interval on the
`val` image set and keeps best_*; a --synthetic run has no validation split and skips it.  Scoring a checkpoint on its own
(the reference's --test_only) is main_seg_val.py.  Not built here: --test_only, --eval_pgd, --save_val_results (they raise),
--dataset cityscapes (its ExtColorJitter has no kernel), visdom and tensorboard (accepted, ignored)."""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_seg.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    deeplab, seg_trainer, seg_data, seg_eval, host = _pkg.deeplab, _pkg.seg_trainer, _pkg.seg_data, _pkg.seg_eval, _pkg.host
else:
    from . import deeplab, host, seg_data, seg_eval, seg_trainer

UNBUILT_VALIDATION = {"test_only": "validation of a checkpoint on its own is main_seg_val.py (cmd/run_seg_val.sh), not a flag of this program",
                      "eval_pgd": "validation under an image-space PGD attack (args.pgd_validate) is not built; main_seg_val.py scores clean images",
                      "save_val_results": "writing validation images is not built; validation itself runs at --val_interval and in main_seg_val.py"}
NO_VAL_SPLIT = "a --synthetic run has no validation split (main_seg_val.py --synthetic N scores a checkpoint on a synthetic one)"
# network/modeling.py's map without the mobilenets, which main_aug_final.py can name but this build has no kernels for
MODEL_MAP = deeplab.MODELS


def get_argparser():
    """args.py:10-106, option for option."""
    parser = argparse.ArgumentParser()
    parser.add_argument("exp", type=str, default='', help="path to exp")
    parser.add_argument('--loss_settings', default=0, type=int, help='loss setting')
    parser.add_argument("--eval_pgd", type=str, default='', help="path to ckpt")
    parser.add_argument("--test_only", type=str, default='', help="path to ckpt")
    # se settings
    parser.add_argument("--mix_layer", type=str, default='', help="from clean to adv")
    parser.add_argument('--steps', default=1, type=int, help='PGD-steps')
    parser.add_argument('--pertub_idx_se', help='index of perturb layers', default=3, type=int)
    parser.add_argument('--gamma_se', help='index of PGD gamma', default=0.5, type=float)
    parser.add_argument('--randinit', action="store_true", help="whether using randinit")
    parser.add_argument('--clip', action="store_true", help="whether using clip")
    parser.add_argument('--mix_all', action="store_true", help="whether using clip")
    parser.add_argument('--eps', default=2, type=float)
    # sd settings
    parser.add_argument('--pertub_idx_sd', help='index of perturb layers', default="", type=str)
    parser.add_argument('--gamma_sd', help='index of PGD gamma', default=0.5, type=float)
    parser.add_argument('--noise_sd', help='if use noise', default=0, type=float)
    parser.add_argument('--adv_loss_weight_sd', help='loss', default=0.5, type=float)
    parser.add_argument('--mix_sd', action="store_true", help="whether using mix")
    # input-PGD settings
    parser.add_argument('--steps_pgd', default=1, type=int, help='PGD-steps')
    parser.add_argument('--gamma_pgd', help='index of PGD gamma', default=0.5, type=float)
    parser.add_argument('--eps_pgd', default=2, type=float)
    parser.add_argument('--randinit_pgd', action="store_true", help="whether using randinit")
    parser.add_argument('--clip_pgd', action="store_true", help="whether using clip")
    parser.add_argument('--adv_type', default="baseline", help="whether test baseline")
    # Dataset Options
    parser.add_argument("--data_root", type=str, default='./datasets/data', help="path to Dataset")
    parser.add_argument("--dataset", type=str, default='voc', choices=['voc', 'cityscapes'], help='Name of dataset')
    parser.add_argument("--num_classes", type=int, default=None, help="num classes (default: None)")
    # Deeplab Options
    parser.add_argument("--model", type=str, default='deeplabv3plus_resnet50',
                        choices=['deeplabv3_resnet50', 'deeplabv3plus_resnet50', 'deeplabv3_resnet101', 'deeplabv3plus_resnet101',
                                 'deeplabv3_mobilenet', 'deeplabv3plus_mobilenet'], help='model name')
    parser.add_argument("--separable_conv", action='store_true', default=False, help="apply separable conv to decoder and aspp")
    parser.add_argument("--output_stride", type=int, default=16, choices=[8, 16])
    # Train Options
    parser.add_argument("--save_val_results", action='store_true', default=False, help="save segmentation results to \"./results\"")
    parser.add_argument("--total_itrs", type=int, default=30e3, help="epoch number (default: 30k)")
    parser.add_argument("--lr", type=float, default=0.01, help="learning rate (default: 0.01)")
    parser.add_argument("--lr_policy", type=str, default='poly', choices=['poly', 'step'], help="learning rate scheduler policy")
    parser.add_argument("--step_size", type=int, default=10000)
    parser.add_argument("--crop_val", action='store_true', default=False, help='crop validation (default: False)')
    parser.add_argument("--batch_size", type=int, default=16, help='batch size (default: 16)')
    parser.add_argument("--val_batch_size", type=int, default=4, help='batch size for validation (default: 4)')
    parser.add_argument("--crop_size", type=int, default=513)
    parser.add_argument("--ckpt", default=None, type=str, help="restore from checkpoint")
    parser.add_argument("--continue_training", action='store_true', default=False)
    parser.add_argument("--loss_type", type=str, default='cross_entropy', choices=['cross_entropy', 'focal_loss'],
                        help="loss type (default: False)")
    parser.add_argument("--gpu_id", type=str, default='0', help="GPU ID")
    parser.add_argument("--weight_decay", type=float, default=1e-4, help='weight decay (default: 1e-4)')
    parser.add_argument("--random_seed", type=int, default=1, help="random seed (default: 1)")
    parser.add_argument("--print_interval", type=int, default=10, help="print interval of loss (default: 10)")
    parser.add_argument("--val_interval", type=int, default=100, help="epoch interval for eval (default: 100)")
    parser.add_argument("--download", action='store_true', default=False, help="download datasets")
    # PASCAL VOC Options
    parser.add_argument("--year", type=str, default='2012', choices=['2012_aug', '2012', '2011', '2009', '2008', '2007'],
                        help='year of VOC')
    # Visdom options
    parser.add_argument("--enable_vis", action='store_true', default=False, help="use visdom for visualization")
    parser.add_argument("--vis_port", type=str, default='13570', help='port for visdom')
    parser.add_argument("--vis_env", type=str, default='main', help='env for visdom')
    parser.add_argument("--vis_num_samples", type=int, default=8, help='number of samples for visualization (default: 8)')
    return parser


ADDITIONS = ("dtype", "layout", "synthetic", "max_side", "graph")


def get_full_argparser():
    parser = get_argparser()
    parser.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="backbone compute dtype")
    parser.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"], help="internal activation / weight layout")
    parser.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images of random sizes instead of VOC")
    parser.add_argument("--max_side", type=int, default=0, help="--synthetic: the longest image side (0: 500, VOC's; the shortest is 3/4 of it)")
    parser.add_argument("--graph", type=int, default=1, choices=[0, 1], help="replay the iteration as a hipGraph (1) or launch it eagerly (0)")
    return parser


def print_args(args, str_num=80):
    """args.py:259-262"""
    for arg, val in args.__dict__.items():
        print(arg + '.' * (str_num - len(arg) - len(str(val))) + str(val))
    print()


def exp_name(opts):
    """main_aug_final.py:106"""
    return (opts.dataset.lower() + "_" + opts.exp + "_selayer_" + str(opts.pertub_idx_se) + "_sdlayer_" + str(opts.pertub_idx_sd)
            + "_gamma_se" + str(opts.gamma_se) + "_gamma_sd" + str(opts.gamma_sd) + "_advweight" + str(opts.adv_loss_weight_sd)
            + "MIX" + str(opts.mix_layer))


def ckpt_path(opts):
    """main_aug_final.py:250-251 (opts.exp already holds exp_name)"""
    return 'checkpoints/' + opts.exp + '/latest_%s_%s_os%d.pth' % (opts.model, opts.dataset, opts.output_stride)


def check_unbuilt(opts):
    """The reference's options this build has nothing behind: raise before any work is done."""
    for flag in ("test_only", "eval_pgd", "save_val_results"):
        if getattr(opts, flag):
            raise NotImplementedError(f"--{flag}: {UNBUILT_VALIDATION[flag]}")
    if opts.dataset.lower() == "cityscapes":
        raise NotImplementedError("--dataset cityscapes: its training transform has ExtColorJitter, which the batch kernel does not do")
    if opts.model not in MODEL_MAP:
        raise NotImplementedError(f"--model {opts.model}: the mobilenet backbones are not built (no kernels for depthwise convolutions)")
    if opts.separable_conv:
        raise NotImplementedError("--separable_conv: depthwise-separable convolutions are not built")
    if opts.loss_type != "cross_entropy":
        raise NotImplementedError("--loss_type focal_loss: only the cross-entropy kernel is built")
    if len(opts.mix_layer) != 2 or not opts.mix_layer.isdigit():
        raise ValueError("--mix_layer takes two digits, e.g. 11 (main_aug_final.py:26-27)")


def main(argv=None):
    opts = get_full_argparser().parse_args(argv)
    print_args(opts)
    check_unbuilt(opts)
    opts.num_classes = 21                                                # (voc; main_aug_final.py:29-32)
    if opts.enable_vis:
        print("INFO: --enable_vis is accepted and ignored (no visdom, no tensorboard in this build)")
    local = int(opts.gpu_id.split(",")[0])
    placement = host.place_rank(local)
    if not torch.cuda.is_available():
        raise RuntimeError("main_aug_final.py needs an MI355X: this build has no CPU path (oracle/ is test infrastructure)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    print("Device: %s" % device)
    print("host placement:", {k: v for k, v in placement.items() if k != "restore"})

    torch.manual_seed(opts.random_seed)
    np.random.seed(opts.random_seed)
    random.seed(opts.random_seed)

    # ---- data: resident on the device, one launch per batch
    if opts.synthetic:
        hi = opts.max_side or 500
        split = seg_data.SyntheticSegSplit(opts.synthetic, seed=opts.random_seed, min_side=max(3 * hi // 4, 1), max_side=hi,
                                           classes=opts.num_classes)
        images, labels = split.images, split.labels
        val_loader, n_val = None, 0
    else:
        images, labels = seg_data.load_voc(opts.data_root, opts.year, "train")
        val_images, val_labels = seg_data.load_voc(opts.data_root, opts.year, "val")
        val_loader = seg_data.SegDeviceLoader(val_images, val_labels, opts.val_batch_size, device, False, opts.crop_size,
                                              crop_val=opts.crop_val)      # (without --crop_val: batches of 1, :50-51)
        n_val = len(val_images)
    train_loader = seg_data.SegDeviceLoader(images, labels, opts.batch_size, device, True, opts.crop_size, seed=opts.random_seed)
    if len(train_loader) == 0:
        raise ValueError(f"{len(images)} images make no batch of {opts.batch_size} (drop_last)")
    print("Dataset: %s, Train set: %d, Val set: %d" % (opts.dataset, len(images), n_val))

    # ---- model, trainer (optimizer + scheduler), criterion
    model = MODEL_MAP[opts.model](num_classes=opts.num_classes, output_stride=opts.output_stride)
    model.set_compute_dtype(torch.bfloat16 if opts.dtype == "bf16" else torch.float32)
    model.set_channels_last(opts.layout == "nhwc").to(device).train()
    metrics = seg_eval.StreamSegMetrics(opts.num_classes, device)
    criterion = nn.CrossEntropyLoss(ignore_index=255, reduction='mean')
    trainer = seg_trainer.SegTrainer(model, criterion, steps=opts.steps, eps=opts.eps, gamma_se=opts.gamma_se, gamma_sd=opts.gamma_sd,
                                     pertub_idx_se=opts.pertub_idx_se, pertub_idx_sd=opts.pertub_idx_sd, mix_layer=opts.mix_layer,
                                     mix_sd=opts.mix_sd, noise_sd=opts.noise_sd, randinit=opts.randinit, clip=opts.clip, lr=opts.lr,
                                     weight_decay=opts.weight_decay, total_itrs=opts.total_itrs, lr_policy=opts.lr_policy,
                                     step_size=opts.step_size, use_graph=bool(opts.graph))
    optimizer, scheduler = trainer.optimizer, trainer.scheduler

    best_score = 0.0
    cur_itrs = 0
    cur_epochs = 0

    def save_ckpt(path):
        torch.save({
            "cur_itrs": cur_itrs,
            "model_state": model.state_dict(),                            # (un-wrapped: what model.module.state_dict() is)
            "optimizer_state": optimizer.state_dict(),
            "scheduler_state": scheduler.state_dict(),
            "best_score": best_score,
        }, path)
        print("Model saved as %s" % path)

    opts.exp = exp_name(opts)
    print("INFO: Save dir:[{}]".format(opts.exp))
    os.makedirs('checkpoints/' + opts.exp, exist_ok=True)
    if opts.ckpt is not None and os.path.isfile(opts.ckpt):
        checkpoint = torch.load(opts.ckpt, map_location=torch.device('cpu'))
        model.load_state_dict(checkpoint["model_state"])
        trainer.arena.refresh_shadow()
        if opts.continue_training:
            optimizer.load_state_dict(checkpoint["optimizer_state"])
            scheduler.load_state_dict(checkpoint["scheduler_state"])
            cur_itrs = checkpoint["cur_itrs"]
            best_score = checkpoint['best_score']
            print("Training state restored from %s" % opts.ckpt)
        print("Model restored from %s" % opts.ckpt)
        del checkpoint
    else:
        print("[!] Retrain")

    pending = []                                                        # device-side losses since the last print
    total_time = 0
    while True:
        model.train()
        cur_epochs += 1
        for images_b, labels_b in train_loader:
            t0 = time.time()
            cur_itrs += 1
            r = trainer.step(images_b, labels_b)
            pending.append(r["loss"])
            if cur_itrs % 10 == 0:
                if trainer.flush_guard():
                    print("in-launch BatchNorm: a grid barrier gave up; the affected steps were run again on the two-launch forms")
                interval_loss = float(torch.stack([p.detach().float().reshape(()) for p in pending]).sum()) / 10    # the one read-back
                pending.clear()
                print(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime()) + ' | ' +
                      "Epoch:[{}], Itrs:[{}/{}], Loss:[{:.4f}], Time:[{:.4f} min], Best IOU:[{:.4f}]"
                      .format(cur_epochs, cur_itrs, int(opts.total_itrs), interval_loss, total_time / 60, best_score), flush=True)
                total_time = 0.0
            if cur_itrs % opts.val_interval == 0:
                trainer.flush_guard()
                save_ckpt(ckpt_path(opts))
                if val_loader is None:
                    print("validation skipped: " + NO_VAL_SPLIT)
                else:
                    # main_aug_final.py:252-263,276 — eager, outside the step's graph and its buffers
                    print("validation...")
                    model.eval()
                    val_score, _ = seg_eval.validate(opts=opts, model=model, loader=val_loader, device=device, metrics=metrics)
                    print(metrics.to_str(val_score))
                    if val_score['Mean IoU'] > best_score:                # save best model
                        best_score = float(val_score['Mean IoU'])
                        save_ckpt('checkpoints/' + opts.exp + '/best_%s_%s_os%d.pth' % (opts.model, opts.dataset, opts.output_stride))
                    model.train()
            scheduler.step()
            total_time += time.time() - t0
            if cur_itrs >= opts.total_itrs:
                trainer.flush_guard()
                print("syd: --------------------[SD]--------------------")
                print("syd: Model dir:[{}]".format(opts.exp))
                print("syd: Setting: Layer:[{}] Gamma:[{}] Best IOU:[{}]".format(opts.pertub_idx_sd, opts.gamma_sd, best_score))
                print("syd: --------------------[SD]--------------------")
                return


if __name__ == '__main__':
    main()
