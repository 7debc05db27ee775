"""Segmentation baseline training entry point — the flags, defaults, stdout lines and checkpoint layout of the reference's
Segmentation/main_ori.py (flags args.py:10-106, loop :144-216), so `bash cmd/run_seg_base.sh` works.  It is the mIoU every A-FAN number
of main_aug_final.py is compared against.  Additions (all optional): --dtype, --layout, --synthetic N, --max_side, --graph.

What differs from the reference is execution only: the iteration body is seg_trainer.SegBaseTrainer.step (one train-mode forward, the
upsampled cross-entropy, backward and the two-group SGD on HIP kernels, replayed as a hipGraph), the batch is built on the device by
seg_data.SegDeviceLoader in one call, and the loss stays on the device until the `Epoch:[..], Itrs:[..], Loss:[..]` line needs it,
every 10 iterations.

--dataset cityscapes (19 classes) trains on seg_data.load_cityscapes through the loader's colour-jitter kernel (ExtRandomCrop ->
ExtColorJitter(0.5, 0.5, 0.5) -> flip, args.py:143-148) and validates on the images as they are, one per batch (the confusion matrix is a
sum and the model is in eval mode, so the scores are those of the reference's --val_batch_size 4).  --test_only scores --ckpt and returns.
Not built here: the mobilenet models, --separable_conv, --loss_type focal_loss, --save_val_results (they raise); visdom and tensorboard
(accepted, ignored)."""
import os
import random
import sys
import time

import numpy as np
import torch
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_seg_base.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    deeplab, seg_trainer, seg_data, seg_eval, host = _pkg.deeplab, _pkg.seg_trainer, _pkg.seg_data, _pkg.seg_eval, _pkg.host
    _args = importlib.import_module("cv_a-fan_amd.main_aug_final")
else:
    from . import deeplab, host, seg_data, seg_eval, seg_trainer
    from . import main_aug_final as _args

# args.py:10-106 is one parser for both programs: main_aug_final.py restates it, this program imports it
get_argparser, get_full_argparser, print_args, ADDITIONS = _args.get_argparser, _args.get_full_argparser, _args.print_args, _args.ADDITIONS
MODEL_MAP = deeplab.MODELS
NUM_CLASSES = {"voc": 21, "cityscapes": 19}                              # main_ori.py:25-28
JITTER = (0.5, 0.5, 0.5)                                                 # args.py:146


def ckpt_path(opts, kind="latest"):
    """main_ori.py:181-182,193-194: checkpoints/<exp>/<kind>_<model>_<dataset>_os<stride>.pth, the experiment name as given"""
    return 'checkpoints/' + opts.exp + '/%s_%s_%s_os%d.pth' % (kind, opts.model, opts.dataset, opts.output_stride)


def check_unbuilt(opts):
    """The reference's options this build has nothing behind: raise before any work is done."""
    if opts.model not in MODEL_MAP:
        raise NotImplementedError(f"--model {opts.model}: the mobilenet backbones are not built (no kernels for depthwise convolutions)")
    if opts.separable_conv:
        raise NotImplementedError("--separable_conv: depthwise-separable convolutions are not built")
    if opts.loss_type != "cross_entropy":
        raise NotImplementedError("--loss_type focal_loss: only the cross-entropy kernel is built")
    if opts.save_val_results:
        raise NotImplementedError("--save_val_results: writing validation images is not built; validation itself runs at --val_interval")


def synthetic_splits(opts):
    """--synthetic N: a training and a validation split of N images each, drawn as main_seg_val.synthetic_split draws (sides in
    [3/4 max_side, max_side]; never below the crop for Cityscapes, which does not pad), from two seeds."""
    hi = opts.max_side or 500
    lo = max(3 * hi // 4, 1)
    if opts.dataset.lower() == "cityscapes":
        lo, hi = max(lo, opts.crop_size), max(hi, opts.crop_size)
    return [seg_data.SyntheticSegSplit(opts.synthetic, seed=opts.random_seed + k, min_side=lo, max_side=hi, classes=opts.num_classes)
            for k in (0, 1)]


def build_loaders(opts, device):
    """args.py:109-164 as two SegDeviceLoaders -> (train loader, validation loader, train size, validation size)."""
    city = opts.dataset.lower() == "cityscapes"
    if opts.synthetic:
        train, val = synthetic_splits(opts)
        (images, labels), (val_images, val_labels) = (train.images, train.labels), (val.images, val.labels)
    elif city:
        images, labels = seg_data.load_cityscapes(opts.data_root, "train")
        val_images, val_labels = seg_data.load_cityscapes(opts.data_root, "val")
    else:
        images, labels = seg_data.load_voc(opts.data_root, opts.year, "train")
        val_images, val_labels = seg_data.load_voc(opts.data_root, opts.year, "val")
    if city:
        train_loader = seg_data.SegDeviceLoader(images, labels, opts.batch_size, device, True, opts.crop_size, seed=opts.random_seed,
                                                jitter=JITTER, scale_range=(1, 1))
        val_loader = seg_data.SegDeviceLoader(val_images, val_labels, opts.val_batch_size, device, False, opts.crop_size)
    else:
        train_loader = seg_data.SegDeviceLoader(images, labels, opts.batch_size, device, True, opts.crop_size, seed=opts.random_seed)
        val_loader = seg_data.SegDeviceLoader(val_images, val_labels, opts.val_batch_size, device, False, opts.crop_size,
                                              crop_val=opts.crop_val)      # (without --crop_val: batches of 1, main_ori.py:46-47)
    return train_loader, val_loader, len(images), len(val_images)


def main(argv=None):
    opts = get_full_argparser().parse_args(argv)
    print_args(opts)
    check_unbuilt(opts)
    opts.num_classes = NUM_CLASSES[opts.dataset.lower()]
    if opts.enable_vis:
        print("INFO: --enable_vis is accepted and ignored (no visdom, no tensorboard in this build)")
    local = int(opts.gpu_id.split(",")[0])
    placement = host.place_rank(local)
    if not torch.cuda.is_available():
        raise RuntimeError("main_ori.py needs an MI355X: this build has no CPU path (oracle/ is test infrastructure)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    print("Device: %s" % device)
    print("host placement:", {k: v for k, v in placement.items() if k != "restore"})

    torch.manual_seed(opts.random_seed)
    np.random.seed(opts.random_seed)
    random.seed(opts.random_seed)

    # ---- data: resident on the device, one call per batch
    train_loader, val_loader, n_train, n_val = build_loaders(opts, device)
    if len(train_loader) == 0 and not opts.test_only:
        raise ValueError(f"{n_train} images make no batch of {opts.batch_size} (drop_last)")
    print("Dataset: %s, Train set: %d, Val set: %d" % (opts.dataset, n_train, n_val))

    # ---- model, trainer (optimizer + scheduler), criterion
    model = MODEL_MAP[opts.model](num_classes=opts.num_classes, output_stride=opts.output_stride)
    model.set_compute_dtype(torch.bfloat16 if opts.dtype == "bf16" else torch.float32)
    model.set_channels_last(opts.layout == "nhwc").to(device).train()
    metrics = seg_eval.StreamSegMetrics(opts.num_classes, device)
    criterion = nn.CrossEntropyLoss(ignore_index=255, reduction='mean')
    trainer = seg_trainer.SegBaseTrainer(model, criterion, lr=opts.lr, weight_decay=opts.weight_decay, total_itrs=opts.total_itrs,
                                         lr_policy=opts.lr_policy, step_size=opts.step_size, use_graph=bool(opts.graph))
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

    def validation():
        # main_ori.py:183-187 — eager, outside the step's graph and its buffers
        model.eval()
        val_score, _ = seg_eval.validate(opts=opts, model=model, loader=val_loader, device=device, metrics=metrics)
        print(metrics.to_str(val_score))
        return val_score

    if opts.test_only:                                                    # main_ori.py:137-142
        return validation()

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
            if cur_itrs % opts.val_interval == 0 and cur_itrs >= opts.total_itrs / 2:
                trainer.flush_guard()
                save_ckpt(ckpt_path(opts))
                print("validation...")
                val_score = validation()
                if val_score['Mean IoU'] > best_score:                    # save best model
                    best_score = float(val_score['Mean IoU'])
                    save_ckpt(ckpt_path(opts, "best"))
                model.train()
            scheduler.step()
            total_time += time.time() - t0
            if cur_itrs >= opts.total_itrs:
                trainer.flush_guard()
                print("syd Best IOU:[{}]".format(best_score))
                return {"best_score": best_score, "cur_itrs": cur_itrs, "loss": r["loss"]}


if __name__ == '__main__':
    main()
