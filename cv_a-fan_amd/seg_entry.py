"""What the three Segmentation programs share, as plain functions: the reference's parser (args.py:10-106 is one parser for
main_aug_final.py and main_ori.py) and the additions, print_args, device set-up, seeding, the synthetic splits, the model build, the
checkpoint writer, the restore block, validation and the iteration loop.  main_aug_final.py, main_ori.py and main_seg_val.py keep their
trainers, their loaders, their lists of unbuilt flags and what only they print; the loop takes any trainer with step(), flush_guard(),
model, optimizer and scheduler, so it runs on a stub without a GPU (tests/test_seg_entry_loop.py)."""
import argparse
import os
import random
import time

import numpy as np
import torch

from . import deeplab, host, seg_data, seg_eval

# network/modeling.py's map without the mobilenets, which the parser can name but this build has no kernels for
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



def check_model(opts):
    if opts.model not in MODEL_MAP:
        raise NotImplementedError(f"--model {opts.model}: the mobilenet backbones are not built (no kernels for depthwise convolutions)")


def setup_device(program, gpu_id, place=True):
    """-> (device, placement).  place: this process's threads go on one block of cores of its GPU's NUMA node, before the GPU is
    touched; the placement is returned for the program to print."""
    local = int(gpu_id.split(",")[0])
    placement = host.place_rank(local) if place else None
    if not torch.cuda.is_available():
        raise RuntimeError(f"{program} needs an MI355X: this build has no CPU path (oracle/ is test infrastructure)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    print("Device: %s" % device)
    return device, placement


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def synthetic_split(opts, seed=None, classes=21, floor=0):
    """--synthetic N: N images with sides in [3/4 max_side, max_side], never below `floor`, drawn from `seed` (--random_seed)."""
    hi = opts.max_side or 500
    lo = max(3 * hi // 4, 1)
    return seg_data.SyntheticSegSplit(opts.synthetic, seed=opts.random_seed if seed is None else seed, min_side=max(lo, floor),
                                      max_side=max(hi, floor), classes=classes)


def synthetic_splits(opts):
    """--synthetic N: a training and a validation split of N images each, from two seeds; never below the crop for Cityscapes, which
    does not pad."""
    floor = opts.crop_size if opts.dataset.lower() == "cityscapes" else 0
    return [synthetic_split(opts, opts.random_seed + k, opts.num_classes, floor) for k in (0, 1)]


def build_model(opts, num_classes):
    model = MODEL_MAP[opts.model](num_classes=num_classes, output_stride=opts.output_stride)
    model.set_compute_dtype(torch.bfloat16 if opts.dtype == "bf16" else torch.float32)
    return model.set_channels_last(opts.layout == "nhwc")


def save_ckpt(path, trainer, cur_itrs, best_score):
    torch.save({
        "cur_itrs": cur_itrs,
        "model_state": trainer.model.state_dict(),                        # (un-wrapped: what model.module.state_dict() is)
        "optimizer_state": trainer.optimizer.state_dict(),
        "scheduler_state": trainer.scheduler.state_dict(),
        "best_score": best_score,
    }, path)
    print("Model saved as %s" % path)


def restore(opts, model, trainer=None):
    """--ckpt into the model and, with a trainer and --continue_training, into its optimizer and scheduler -> (cur_itrs, best_score)."""
    cur_itrs, best_score = 0, 0.0
    if opts.ckpt is not None and os.path.isfile(opts.ckpt):
        checkpoint = torch.load(opts.ckpt, map_location=torch.device('cpu'))
        model.load_state_dict(checkpoint["model_state"])
        if trainer is not None:
            trainer.arena.refresh_shadow()
            if opts.continue_training:
                trainer.optimizer.load_state_dict(checkpoint["optimizer_state"])
                trainer.scheduler.load_state_dict(checkpoint["scheduler_state"])
                cur_itrs = checkpoint["cur_itrs"]
                best_score = checkpoint['best_score']
                print("Training state restored from %s" % opts.ckpt)
        print("Model restored from %s" % opts.ckpt)
        del checkpoint
    else:
        print("[!] Retrain")
    return cur_itrs, best_score


def validation(opts, model, loader, device, metrics):
    """main_aug_final.py:252-263 — eager, outside the step's graph and its buffers"""
    model.eval()
    val_score, _ = seg_eval.validate(opts=opts, model=model, loader=loader, device=device, metrics=metrics)
    print(metrics.to_str(val_score))
    return val_score


def train_loop(trainer, train_loader, total_itrs, validate, should_validate, latest_path, best_path, closing, cur_itrs=0,
               best_score=0.0, skipped=""):
    """main_aug_final.py:146-289, main_ori.py:144-216.  The loss stays on the device until the `Epoch:[..], Itrs:[..], Loss:[..]` line
    needs it, every 10 iterations.  should_validate(cur_itrs): checkpoint to latest_path, then validate() -> scores (None: the
    `validation skipped: <skipped>` line) and best_path on a better Mean IoU.  closing(best_score) prints the last lines."""
    model, scheduler = trainer.model, trainer.scheduler
    cur_epochs = 0
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
                      .format(cur_epochs, cur_itrs, int(total_itrs), interval_loss, total_time / 60, best_score), flush=True)
                total_time = 0.0
            if should_validate(cur_itrs):
                trainer.flush_guard()
                save_ckpt(latest_path, trainer, cur_itrs, best_score)
                if validate is None:
                    print("validation skipped: " + skipped)
                else:
                    print("validation...")
                    val_score = validate()
                    if val_score['Mean IoU'] > best_score:                # save best model
                        best_score = float(val_score['Mean IoU'])
                        save_ckpt(best_path, trainer, cur_itrs, best_score)
                    model.train()
            scheduler.step()
            total_time += time.time() - t0
            if cur_itrs >= total_itrs:
                trainer.flush_guard()
                closing(best_score)
                return {"best_score": best_score, "cur_itrs": cur_itrs, "loss": r["loss"]}
