"""Segmentation PGD training entry point — the flags, defaults, stdout lines and checkpoint layout of the reference's
Segmentation/main_advtrain.py (flags args.py:10-106), so `bash cmd/run_seg_adv.sh` works.  It trains the checkpoints a robust mIoU is
compared against.  Three modes, as in the reference:

    (default)          the loop of :170-254: image-space sign-PGD on every batch with the model in training mode (--steps_pgd --eps_pgd
                       --gamma_pgd --randinit_pgd --clip_pgd), one SGD step on the adversarial images; checkpoints under adv_training/<exp>/
    --test_only CKPT   :136-149: the clean scores of CKPT (main_seg_val.py is the same evaluation as a program of its own)
    --eval_pgd CKPT    :151-168: its scores under image PGD (main_seg_rob.py likewise)

Additions (all optional): --dtype, --layout, --synthetic N, --max_side, --graph as in main_aug_final.py, and --noise {device,host}: where
--randinit_pgd's start is drawn.  `device` draws it inside the start's own launch from a device-resident generator (afan_pgd_rand_start),
so the whole iteration — attack passes, start, training pass, SGD — is one replayed hipGraph; `host` is the reference's torch.rand on the
CPU generator with its upload in every step, which keeps the iteration eager.  The evaluations draw on the host either way.

What differs from the reference is execution only: the iteration body is seg_trainer.SegAdvTrainer.step, the batch is built on the device
by seg_data.SegDeviceLoader in one call, and the loss stays on the device until the `Epoch:[..], Itrs:[..], Loss:[..]` line needs it.
The reference skips every batch that is not 4 images (:184) and with another --batch_size never reaches its exit: that raises here.
Not built: the mobilenet models, --separable_conv, --loss_type focal_loss, --save_val_results (they raise); visdom and tensorboard
(accepted, ignored)."""
import functools
import os
import sys

import torch.nn as nn

if __package__ in (None, ""):  # executed as a script (cmd/run_seg_adv.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("cv_a-fan_amd")
    seg_trainer, seg_eval = _pkg.seg_trainer, _pkg.seg_eval
    seg_entry = importlib.import_module("cv_a-fan_amd.seg_entry")
    main_ori = importlib.import_module("cv_a-fan_amd.main_ori")
    main_seg_rob = importlib.import_module("cv_a-fan_amd.main_seg_rob")
else:
    from . import main_ori, main_seg_rob, seg_entry, seg_eval, seg_trainer

get_argparser, print_args = seg_entry.get_argparser, seg_entry.print_args        # args.py:10-106 is one parser for every program
ADDITIONS = seg_entry.ADDITIONS + ("noise",)
NUM_CLASSES = main_ori.NUM_CLASSES                                               # main_advtrain.py:26-29
BATCH = 4                                                                        # main_advtrain.py:184


def get_full_argparser():
    parser = seg_entry.get_full_argparser()
    parser.add_argument("--noise", default="device", choices=["device", "host"],
                        help="--randinit_pgd in training: draw the start in its own launch on the device (graph replay) or on the host generator (eager)")
    return parser


def ckpt_path(opts, kind="latest"):
    """main_advtrain.py:219-220,231-232: adv_training/<exp>/<kind>_<model>_<dataset>_os<stride>.pth, the experiment name as given"""
    return 'adv_training/' + opts.exp + '/%s_%s_%s_os%d.pth' % (kind, opts.model, opts.dataset, opts.output_stride)


def training(opts):
    return opts.test_only == "" and opts.eval_pgd == ""


def check_unbuilt(opts):
    """What this build has nothing behind, and the batch size the reference's loop cannot finish with: raise before any work is done."""
    main_ori.check_unbuilt(opts)
    if training(opts) and opts.batch_size != BATCH:
        raise ValueError(f"--batch_size {opts.batch_size}: the reference skips every batch that is not {BATCH} images "
                         f"(main_advtrain.py:184: `if images.shape[0] != 4: continue`) and would never reach --total_itrs; train with --batch_size {BATCH}")


def closing(best_score):
    print("Final Best mIOU:[{:.4f}]".format(best_score))                        # main_advtrain.py:252


def evaluate(opts, device):
    """--test_only (:136-149) and --eval_pgd (:151-168) -> the scores.  The lines and their order are main_seg_rob.py's (model, then
    data: the host generator is in the same state when --randinit_pgd draws, so the two programs print the same scores)."""
    model = seg_entry.build_model(opts, opts.num_classes)
    seg_entry.restore(opts, model)                                               # (--ckpt first, as :112-129 run before either branch)
    pgd = opts.test_only == ""
    if pgd:
        print("Test Attack :[{}]".format(opts.eval_pgd))
        main_seg_rob._settings(opts)
    else:
        print("Test Clean baseline:[{}]".format(opts.test_only))
    main_seg_rob.load_overlap(model, opts.eval_pgd if pgd else opts.test_only)
    model.to(device)
    model.eval()
    loader, n_val = main_seg_rob.val_loader(opts, device)
    print("Dataset: %s, Val set: %d" % (opts.dataset, n_val))
    metrics = seg_eval.StreamSegMetrics(opts.num_classes, device)
    if pgd:
        criterion = nn.CrossEntropyLoss(ignore_index=255, reduction='mean')      # (main_advtrain.py:92)
        val_score, _ = seg_eval.pgd_validate(opts=opts, model=model, loader=loader, device=device, metrics=metrics, criterion=criterion)
        main_seg_rob._settings(opts)
    else:
        val_score, _ = seg_eval.validate(opts=opts, model=model, loader=loader, device=device, metrics=metrics)
    print(metrics.to_str(val_score))
    return val_score


def main(argv=None):
    opts = get_full_argparser().parse_args(argv)
    print_args(opts)
    check_unbuilt(opts)
    opts.num_classes = NUM_CLASSES[opts.dataset.lower()]
    if opts.enable_vis:
        print("INFO: --enable_vis is accepted and ignored (no visdom, no tensorboard in this build)")
    if training(opts) and opts.noise == "host":
        print("INFO: --noise host: --randinit_pgd draws its start with torch.rand on the CPU generator, as the reference does, and uploads "
              "it in every step; with --randinit_pgd the iteration is launched eagerly (no hipGraph)")
    device, placement = seg_entry.setup_device("main_advtrain.py", opts.gpu_id, place=training(opts))
    seg_entry.seed_all(opts.random_seed)
    if not training(opts):
        return evaluate(opts, device)
    print("host placement:", {k: v for k, v in placement.items() if k != "restore"})

    # ---- data: resident on the device, one call per batch
    train_loader, val_loader, n_train, n_val = main_ori.build_loaders(opts, device)
    if len(train_loader) == 0:
        raise ValueError(f"{n_train} images make no batch of {opts.batch_size} (drop_last)")
    print("Dataset: %s, Train set: %d, Val set: %d" % (opts.dataset, n_train, n_val))

    # ---- model, trainer (optimizer + scheduler), criterion
    model = seg_entry.build_model(opts, opts.num_classes).to(device).train()
    metrics = seg_eval.StreamSegMetrics(opts.num_classes, device)
    criterion = nn.CrossEntropyLoss(ignore_index=255, reduction='mean')
    trainer = seg_trainer.SegAdvTrainer(model, criterion, steps_pgd=opts.steps_pgd, eps_pgd=opts.eps_pgd, gamma_pgd=opts.gamma_pgd,
                                        randinit=opts.randinit_pgd, clip=opts.clip_pgd, noise=opts.noise, lr=opts.lr,
                                        weight_decay=opts.weight_decay, total_itrs=opts.total_itrs, lr_policy=opts.lr_policy,
                                        step_size=opts.step_size, use_graph=bool(opts.graph))

    os.makedirs('adv_training/' + opts.exp, exist_ok=True)
    cur_itrs, best_score = seg_entry.restore(opts, model, trainer)

    def validation():
        return seg_entry.validation(opts, model, val_loader, device, metrics)

    return seg_entry.train_loop(trainer, train_loader, opts.total_itrs, validation, functools.partial(main_ori.should_validate, opts),
                                ckpt_path(opts), ckpt_path(opts, "best"), closing, cur_itrs, best_score)


if __name__ == '__main__':
    main()
