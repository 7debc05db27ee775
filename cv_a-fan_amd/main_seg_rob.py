"""Robust mIoU of a segmentation checkpoint: what the reference's Segmentation/main_advtrain.py does under --eval_pgd (:151-168), as a
program of its own, so `bash cmd/run_seg_rob.sh` works: every validation batch is attacked in image space by sign-PGD
(seg_attack_algo.adv_input) and the predictions on the adversarial images are scored (seg_eval.pgd_validate).  The flags it shares
with the reference keep the reference's names and defaults (args.py:14-105): --eval_pgd --steps_pgd --gamma_pgd --eps_pgd
--randinit_pgd --clip_pgd --dataset --model --output_stride --data_root --year --crop_val --crop_size --val_batch_size --gpu_id
--random_seed.  Additions: --dtype, --layout, --synthetic N, --max_side (as main_aug_final.py's).

Per batch: SegDeviceLoader's one launch, steps_pgd eval-mode forward + input-gradient passes (deeplab.FROZEN_EVAL: a bottleneck is one
node, a convolution and its BatchNorm one launch), one forward up to the classifier's low-resolution logits and one scoring launch;
the confusion matrix is read back once, for the printed scores."""
import argparse
import os
import sys

import torch
import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_seg_rob.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    seg_data, seg_eval, seg_entry = _pkg.seg_data, _pkg.seg_eval, importlib.import_module("cv_a-fan_amd.seg_entry")
    main_ori = importlib.import_module("cv_a-fan_amd.main_ori")
else:
    from . import main_ori, seg_data, seg_entry, seg_eval

NUM_CLASSES = {"voc": 21, "cityscapes": 19}                          # (main_advtrain.py:43-46)
ADDITIONS = ("dtype", "layout", "synthetic", "max_side")


def _checkpoint(path):
    if path == "":
        raise argparse.ArgumentTypeError("--eval_pgd needs the path of a checkpoint")
    return path


def get_argparser():
    parser = argparse.ArgumentParser()
    # the reference's options (args.py), names and defaults unchanged
    parser.add_argument("--eval_pgd", type=_checkpoint, default='', required=True, help="path to ckpt")
    parser.add_argument('--steps_pgd', default=1, type=int, help='PGD-steps')
    parser.add_argument('--gamma_pgd', help='index of PGD gamma', default=0.5, type=float)
    parser.add_argument('--eps_pgd', default=2, type=float)
    parser.add_argument('--randinit_pgd', action="store_true", help="whether using randinit")
    parser.add_argument('--clip_pgd', action="store_true", help="whether using clip")
    parser.add_argument("--data_root", type=str, default='./datasets/data', help="path to Dataset")
    parser.add_argument("--dataset", type=str, default='voc', choices=['voc', 'cityscapes'], help='Name of dataset')
    parser.add_argument("--model", type=str, default='deeplabv3plus_resnet50',
                        choices=['deeplabv3_resnet50', 'deeplabv3plus_resnet50', 'deeplabv3_resnet101', 'deeplabv3plus_resnet101',
                                 'deeplabv3_mobilenet', 'deeplabv3plus_mobilenet'], help='model name')
    parser.add_argument("--output_stride", type=int, default=16, choices=[8, 16])
    parser.add_argument("--crop_val", action='store_true', default=False, help='crop validation (default: False)')
    parser.add_argument("--val_batch_size", type=int, default=4, help='batch size for validation (default: 4)')
    parser.add_argument("--crop_size", type=int, default=513)
    parser.add_argument("--gpu_id", type=str, default='0', help="GPU ID")
    parser.add_argument("--random_seed", type=int, default=1, help="random seed (default: 1)")
    parser.add_argument("--year", type=str, default='2012', choices=['2012_aug', '2012', '2011', '2009', '2008', '2007'],
                        help='year of VOC')
    # additions
    parser.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="backbone compute dtype")
    parser.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"], help="internal activation / weight layout")
    parser.add_argument("--synthetic", type=int, default=0, help="attack N synthetic images of random sizes instead of the validation set")
    parser.add_argument("--max_side", type=int, default=0, help="--synthetic: the longest image side (0: 500, VOC's; the shortest is 3/4 of it)")
    return parser


def load_overlap(model, path):
    """main_advtrain.py:156-161: of the checkpoint's "model_state", the entries whose keys the model has; the rest of the model keeps
    what it had.  Prints the `Overlap:[k/n]` line and returns (k, n)."""
    checkpoint = torch.load(path, map_location=torch.device('cpu'))["model_state"]
    model_state_dict = model.state_dict()
    overlap_dict = {k: v for k, v in checkpoint.items() if k in model_state_dict.keys()}
    model_state_dict.update(overlap_dict)
    model.load_state_dict(model_state_dict)
    print("Overlap:[{}/{}]".format(len(overlap_dict.keys()), len(model_state_dict.keys())))
    return len(overlap_dict), len(model_state_dict)


def val_loader(opts, device):
    """The validation split as a SegDeviceLoader -> (loader, number of images); main_advtrain.py scores the same one."""
    if opts.dataset.lower() == "cityscapes":
        opts.batch_size = opts.val_batch_size                                    # (build_loaders builds the training loader too)
        _, loader, _, n_val = main_ori.build_loaders(opts, device)
        return loader, n_val
    if opts.synthetic:
        split = seg_entry.synthetic_split(opts)
        images, labels = split.images, split.labels
    else:
        images, labels = seg_data.load_voc(opts.data_root, opts.year, "val")
    return seg_data.SegDeviceLoader(images, labels, opts.val_batch_size, device, False, opts.crop_size, crop_val=opts.crop_val), len(images)


def _settings(opts):
    print("Attack Settings: Step[{}] Gamma[{}] Eps[{}] Randinit[{}] Clip[{}]"
          .format(opts.steps_pgd, opts.gamma_pgd, opts.eps_pgd, opts.randinit_pgd, opts.clip_pgd))


def main(argv=None):
    opts = get_argparser().parse_args(argv)
    seg_entry.print_args(opts)
    seg_entry.check_model(opts)
    opts.num_classes = NUM_CLASSES[opts.dataset.lower()]
    device, _ = seg_entry.setup_device("main_seg_rob.py", opts.gpu_id, place=False)
    seg_entry.seed_all(opts.random_seed)

    model = seg_entry.build_model(opts, opts.num_classes)
    criterion = nn.CrossEntropyLoss(ignore_index=255, reduction='mean')          # (main_advtrain.py:92)
    print("Test Attack :[{}]".format(opts.eval_pgd))
    _settings(opts)
    load_overlap(model, opts.eval_pgd)
    model.to(device)
    model.eval()

    loader, n_val = val_loader(opts, device)
    print("Dataset: %s, Val set: %d" % (opts.dataset, n_val))

    metrics = seg_eval.StreamSegMetrics(opts.num_classes, device)
    val_score, _ = seg_eval.pgd_validate(opts=opts, model=model, loader=loader, device=device, metrics=metrics, criterion=criterion)
    _settings(opts)
    print(metrics.to_str(val_score))
    return val_score


if __name__ == '__main__':
    main()
