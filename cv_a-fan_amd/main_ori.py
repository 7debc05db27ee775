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
import functools
import os
import sys

import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_seg_base.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    seg_trainer, seg_data, seg_eval = _pkg.seg_trainer, _pkg.seg_data, _pkg.seg_eval
    seg_entry = importlib.import_module("cv_a-fan_amd.seg_entry")
else:
    from . import seg_data, seg_entry, seg_eval, seg_trainer

# args.py:10-106 is one parser for both programs
get_argparser, get_full_argparser, print_args, ADDITIONS = (seg_entry.get_argparser, seg_entry.get_full_argparser, seg_entry.print_args,
                                                            seg_entry.ADDITIONS)
synthetic_splits = seg_entry.synthetic_splits
NUM_CLASSES = {"voc": 21, "cityscapes": 19}                              # main_ori.py:25-28
JITTER = (0.5, 0.5, 0.5)                                                 # args.py:146


def ckpt_path(opts, kind="latest"):
    """main_ori.py:181-182,193-194: checkpoints/<exp>/<kind>_<model>_<dataset>_os<stride>.pth, the experiment name as given"""
    return 'checkpoints/' + opts.exp + '/%s_%s_%s_os%d.pth' % (kind, opts.model, opts.dataset, opts.output_stride)


def check_unbuilt(opts):
    """The reference's options this build has nothing behind: raise before any work is done."""
    seg_entry.check_model(opts)
    if opts.separable_conv:
        raise NotImplementedError("--separable_conv: depthwise-separable convolutions are not built")
    if opts.loss_type != "cross_entropy":
        raise NotImplementedError("--loss_type focal_loss: only the cross-entropy kernel is built")
    if opts.save_val_results:
        raise NotImplementedError("--save_val_results: writing validation images is not built; validation itself runs at --val_interval")


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


def should_validate(opts, cur_itrs):
    return cur_itrs % opts.val_interval == 0 and cur_itrs >= opts.total_itrs / 2


def closing(opts, best_score):
    print("syd Best IOU:[{}]".format(best_score))


def main(argv=None):
    opts = get_full_argparser().parse_args(argv)
    print_args(opts)
    check_unbuilt(opts)
    opts.num_classes = NUM_CLASSES[opts.dataset.lower()]
    if opts.enable_vis:
        print("INFO: --enable_vis is accepted and ignored (no visdom, no tensorboard in this build)")
    device, placement = seg_entry.setup_device("main_ori.py", opts.gpu_id)
    print("host placement:", {k: v for k, v in placement.items() if k != "restore"})
    seg_entry.seed_all(opts.random_seed)

    # ---- data: resident on the device, one call per batch
    train_loader, val_loader, n_train, n_val = build_loaders(opts, device)
    if len(train_loader) == 0 and not opts.test_only:
        raise ValueError(f"{n_train} images make no batch of {opts.batch_size} (drop_last)")
    print("Dataset: %s, Train set: %d, Val set: %d" % (opts.dataset, n_train, n_val))

    # ---- model, trainer (optimizer + scheduler), criterion
    model = seg_entry.build_model(opts, opts.num_classes).to(device).train()
    metrics = seg_eval.StreamSegMetrics(opts.num_classes, device)
    criterion = nn.CrossEntropyLoss(ignore_index=255, reduction='mean')
    trainer = seg_trainer.SegBaseTrainer(model, criterion, lr=opts.lr, weight_decay=opts.weight_decay, total_itrs=opts.total_itrs,
                                         lr_policy=opts.lr_policy, step_size=opts.step_size, use_graph=bool(opts.graph))

    os.makedirs('checkpoints/' + opts.exp, exist_ok=True)
    cur_itrs, best_score = seg_entry.restore(opts, model, trainer)

    def validation():
        return seg_entry.validation(opts, model, val_loader, device, metrics)

    if opts.test_only:                                                    # main_ori.py:137-142
        return validation()
    return seg_entry.train_loop(trainer, train_loader, opts.total_itrs, validation, functools.partial(should_validate, opts),
                                ckpt_path(opts), ckpt_path(opts, "best"), functools.partial(closing, opts), cur_itrs, best_score)


if __name__ == '__main__':
    main()
