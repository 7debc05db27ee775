"""What the Detection programs share, as plain functions: the reference's parser (Detection/train_aug_sat_muti_advt.py:220-256) with
config/config.py and config/train_config.py folded into the defaults, the additions, print_args, the refusals, the data set-up, the
learning-rate schedule in closed form, the checkpoint writer and reader, the log and the iteration loop.  The loop takes the model
and the loader as arguments, so it runs on a small network (tests/test_det_entry_gpu.py).

No summaries are written: tensorboardX is not installed, and the reference's `train/loss` scalar is the `Avg. Loss` of the log."""
import argparse
import ast
import bisect
import os
import time
from collections import deque

import torch

from . import det_data, det_model, det_trainer

# dataset/base.py:20, backbone/base.py:8, roi/pooler.py:16: what the reference's parser accepts
DATASET_OPTIONS = ['voc2007', 'voc20072012', 'coco2017', 'voc2007-cat-dog', 'coco2017-person', 'coco2017-car', 'coco2017-animal']
BACKBONE_OPTIONS = ['resnet18', 'resnet50', 'resnet101']
POOLER_OPTIONS = ['pooling', 'align']

# config/config.py:9-14 and config/train_config.py:9-26, by the name of the flag that overrides each
DEFAULTS = dict(image_min_side=600.0, image_max_side=1000.0, anchor_ratios=[(1, 2), (1, 1), (2, 1)], anchor_sizes=[128, 256, 512],
                pooler_mode='align', rpn_pre_nms_top_n=12000, rpn_post_nms_top_n=2000, anchor_smooth_l1_loss_beta=1.0,
                proposal_smooth_l1_loss_beta=1.0, batch_size=1, learning_rate=0.001, momentum=0.9, weight_decay=0.0005,
                step_lr_sizes=[50000, 70000], step_lr_gamma=0.1, warm_up_factor=0.3333, warm_up_num_iters=500,
                num_steps_to_display=20, num_steps_to_snapshot=10000, num_steps_to_finish=90000)
_LITERALS = ("anchor_ratios", "anchor_sizes", "step_lr_sizes")            # Config.setup: ast.literal_eval of the flag's string

REFUSED_BACKBONES = {
    "resnet18": "--backbone resnet18: its BasicBlock stages have no frozen-BatchNorm block in det_model, which builds Bottleneck stages only",
    "resnet50": "--backbone resnet50: only the (3, 4, 23, 3) ResNet-101 is pinned to the reference's model (tests/golden/det_frcnn_*), and no other depth is built",
}
_COCO = "it reads its annotations through pycocotools, which the project does not depend on"
REFUSED_DATASETS = {
    "coco2017": "--dataset coco2017: " + _COCO,
    "coco2017-person": "--dataset coco2017-person: " + _COCO,
    "coco2017-car": "--dataset coco2017-car: " + _COCO,
    "coco2017-animal": "--dataset coco2017-animal: " + _COCO,
    "voc2007-cat-dog": "--dataset voc2007-cat-dog: its cat / dog subset of VOC 2007 has no loader here (det_data.load_voc_det reads the 20-class lists)",
}


def get_argparser():
    """train_aug_sat_muti_advt.py:220-256, flag for flag."""
    parser = argparse.ArgumentParser()
    # PGD Setting
    parser.add_argument('--steps', default=1, type=int, help='PGD-steps')
    parser.add_argument('--pertub_idx', help='index of perturb layers', default=3, type=int)
    parser.add_argument('--gamma', help='index of PGD gamma', default=0.5, type=float)

    parser.add_argument('--eps', default=2, type=float)
    parser.add_argument('--randinit', action="store_true", help="whether using apex")
    parser.add_argument('--clip', action="store_true", help="whether using apex")

    parser.add_argument('--loss_settings', default=0, type=int, help='loss setting')
    return _common_flags(parser)


def _common_flags(parser):
    """The flags the three Detection training parsers end with (train_aug_sat_muti_advt.py:230-256 == train_aug_final.py:213-238 ==
    train_baseline.py:140-165)."""
    parser.add_argument('-s', '--dataset', type=str, choices=DATASET_OPTIONS, required=True, help='name of dataset')
    parser.add_argument('-b', '--backbone', type=str, choices=BACKBONE_OPTIONS, required=True, help='name of backbone model')
    parser.add_argument('-d', '--data_dir', type=str, default='./data', help='path to data directory')
    parser.add_argument('-o', '--outputs_dir', type=str, default='./outputs', help='path to outputs directory')
    parser.add_argument('-r', '--resume_checkpoint', type=str, help='path to resuming checkpoint')
    parser.add_argument('--image_min_side', type=float, help='default: {:g}'.format(DEFAULTS["image_min_side"]))
    parser.add_argument('--image_max_side', type=float, help='default: {:g}'.format(DEFAULTS["image_max_side"]))
    parser.add_argument('--anchor_ratios', type=str, help='default: "{!s}"'.format(DEFAULTS["anchor_ratios"]))
    parser.add_argument('--anchor_sizes', type=str, help='default: "{!s}"'.format(DEFAULTS["anchor_sizes"]))
    parser.add_argument('--pooler_mode', type=str, choices=POOLER_OPTIONS, help='default: {:s}'.format(DEFAULTS["pooler_mode"]))
    parser.add_argument('--rpn_pre_nms_top_n', type=int, help='default: {:d}'.format(DEFAULTS["rpn_pre_nms_top_n"]))
    parser.add_argument('--rpn_post_nms_top_n', type=int, help='default: {:d}'.format(DEFAULTS["rpn_post_nms_top_n"]))
    parser.add_argument('--anchor_smooth_l1_loss_beta', type=float, help='default: {:g}'.format(DEFAULTS["anchor_smooth_l1_loss_beta"]))
    parser.add_argument('--proposal_smooth_l1_loss_beta', type=float, help='default: {:g}'.format(DEFAULTS["proposal_smooth_l1_loss_beta"]))
    parser.add_argument('--batch_size', type=int, help='default: {:g}'.format(DEFAULTS["batch_size"]))
    parser.add_argument('--learning_rate', type=float, help='default: {:g}'.format(DEFAULTS["learning_rate"]))
    parser.add_argument('--momentum', type=float, help='default: {:g}'.format(DEFAULTS["momentum"]))
    parser.add_argument('--weight_decay', type=float, help='default: {:g}'.format(DEFAULTS["weight_decay"]))
    parser.add_argument('--step_lr_sizes', type=str, help='default: {!s}'.format(DEFAULTS["step_lr_sizes"]))
    parser.add_argument('--step_lr_gamma', type=float, help='default: {:g}'.format(DEFAULTS["step_lr_gamma"]))
    parser.add_argument('--warm_up_factor', type=float, help='default: {:g}'.format(DEFAULTS["warm_up_factor"]))
    parser.add_argument('--warm_up_num_iters', type=int, help='default: {:d}'.format(DEFAULTS["warm_up_num_iters"]))
    parser.add_argument('--num_steps_to_display', type=int, help='default: {:d}'.format(DEFAULTS["num_steps_to_display"]))
    parser.add_argument('--num_steps_to_snapshot', type=int, help='default: {:d}'.format(DEFAULTS["num_steps_to_snapshot"]))
    parser.add_argument('--num_steps_to_finish', type=int, help='default: {:d}'.format(DEFAULTS["num_steps_to_finish"]))
    return parser


def get_final_argparser():
    """train_aug_final.py:196-238, flag for flag."""
    parser = argparse.ArgumentParser()
    # se settings
    parser.add_argument('--steps', default=1, type=int, help='PGD-steps')
    parser.add_argument('--pertub_idx_se', help='index of perturb layers', default=None, type=int)
    parser.add_argument('--pertub_idx_sd', help='index of perturb layers', default='roi', type=str)
    parser.add_argument('--gamma_se', help='index of PGD gamma', default=0.5, type=float)
    parser.add_argument('--gamma_sd', help='index of PGD gamma', default=0.1, type=float)
    parser.add_argument('--eps', default=2, type=float)
    parser.add_argument('--randinit', action="store_true", help="whether using apex")
    parser.add_argument('--clip', action="store_true", help="whether using apex")
    parser.add_argument('--mix_layer', type=str, help="")
    # sd settings
    parser.add_argument('--noise_sd', help='if use noise', default=0, type=float)
    parser.add_argument('--only_roi_sd', action="store_true", help="whether only using roi loss")
    parser.add_argument('--mix_sd', action="store_true", help="whether using mix")
    parser.add_argument('--sd_adv_loss_weight', help='loss', default=0.5, type=float)
    return _common_flags(parser)


def get_base_argparser():
    """train_baseline.py:132-165, flag for flag (its PGD flags are parsed and never read)."""
    parser = argparse.ArgumentParser()
    # PGD Setting
    parser.add_argument('--steps', default=1, type=int, help='PGD-steps')
    parser.add_argument('--pertub_idx', help='index of perturb layers', default=3, type=int)
    parser.add_argument('--gamma', help='index of PGD gamma', default=0.5, type=float)
    parser.add_argument('--eps', default=2, type=float)
    parser.add_argument('--randinit', action="store_true", help="whether using apex")
    parser.add_argument('--clip', action="store_true", help="whether using apex")
    return _common_flags(parser)


def get_adv_argparser():
    """train_baseline_advtrain.py:127-160, flag for flag (no --pertub_idx: the attack is on the image)."""
    parser = argparse.ArgumentParser()
    # PGD Setting
    parser.add_argument('--steps', default=1, type=int, help='PGD-steps')
    parser.add_argument('--gamma', help='index of PGD gamma', default=0.5, type=float)
    parser.add_argument('--eps', default=2, type=float)
    parser.add_argument('--randinit', action="store_true", help="whether using apex")
    parser.add_argument('--clip', action="store_true", help="whether using apex")
    return _common_flags(parser)


ADDITIONS = ("synthetic", "dtype", "layout", "seed")
ADV_ADDITIONS = ADDITIONS + ("noise",)
# Where train_baseline_advtrain.py draws --randinit's start when --noise is not given.  Decided by the project's rule for every switch:
# "device" only where one iteration gains more than the two arms' combined min-max spread (tools/probe/det_adv_time.py (b),
# profiles/det_adv_time.jsonl; README "Detection PGD training").  Measured at 600 x 904: 10.1 ms against 12.7 ms (host) and 20.0 ms
# (host, drawn ahead) at batch 1, spreads 2.5 and 4.3 ms; 30.6 ms against 68.0 and 61.7 ms at batch 8, spreads 3.9 and 15.4 ms: device.
ADV_NOISE_DEFAULT = "device"


def get_full_adv_argparser():
    parser = get_full_argparser(get_adv_argparser())
    parser.add_argument("--noise", default=ADV_NOISE_DEFAULT, choices=["host", "device"],
                        help="where --randinit's start is drawn: torch's CPU generator as the reference does, or inside the start's own launch")
    return parser


def get_full_argparser(parser=None):
    parser = parser if parser is not None else get_argparser()
    parser.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images with boxes instead of VOC")
    parser.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="backbone compute dtype")
    parser.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"], help="internal activation / weight layout")
    parser.add_argument("--seed", type=int, default=None, help="seeds the weights, the loader's epochs and every iteration's draws")
    return parser


def print_args(args, str_num=80):
    """attack_algo.py:248-251"""
    for arg, val in args.__dict__.items():
        print(arg + '.' * (str_num - len(arg) - len(str(val))) + str(val))
    print()


def config(args):
    """Config.setup (config/train_config.py:28-71): the defaults, each replaced by its flag where one was given."""
    cfg = dict(DEFAULTS)
    for k in cfg:
        v = getattr(args, k, None)
        if v is not None:
            cfg[k] = ast.literal_eval(v) if k in _LITERALS else v
    return cfg


def describe(cfg):
    """Config.describe (config/config.py:16-22)"""
    return '\nConfig:\n' + '\n'.join('\t{:s} = {:s}'.format(k.upper(), str(v)) for k, v in sorted(cfg.items())) + '\n'


def exp_name(args):
    """train_aug_sat_muti_advt.py:262-264"""
    name = "s" + str(args.steps) + "p" + str(args.pertub_idx) + "g" + str(args.gamma) + "e" + str(args.eps)
    if args.randinit:
        name += "_rand"
    if args.clip:
        name += "_clip"
    return name


def checkpoints_dir(args):
    """train_aug_sat_muti_advt.py:270-271"""
    return os.path.join(args.outputs_dir, 'ckpt-{:s}-{:s}-{:s}'.format(exp_name(args), args.dataset, args.backbone))


def final_exp_name(args):
    """train_aug_final.py:245-247"""
    name = ("s" + str(args.steps) + "se_" + str(args.pertub_idx_se) + "_sd_" + str(args.pertub_idx_sd) + "_g" + str(args.gamma_se) + "e" +
            str(args.eps) + "_MIX" + args.mix_layer)
    if args.randinit:
        name += "_rand"
    if args.clip:
        name += "_clip"
    return name


def final_checkpoints_dir(args):
    """train_aug_final.py:253-254"""
    return os.path.join(args.outputs_dir, 'ckpt-{:s}-{:s}-{:s}'.format(final_exp_name(args), args.dataset, args.backbone))


def base_checkpoints_dir(args):
    """train_baseline.py:176-177"""
    return os.path.join(args.outputs_dir, 'checkpoints-{:s}-{:s}_baseline'.format(args.dataset, args.backbone))


def check_unbuilt_model(args):
    if args.backbone in REFUSED_BACKBONES:
        raise NotImplementedError(REFUSED_BACKBONES[args.backbone])
    if args.dataset in REFUSED_DATASETS:
        raise NotImplementedError(REFUSED_DATASETS[args.dataset])


def check_unbuilt_final(args):
    """train_aug_final.py: the choices nothing stands behind — here or in the reference — raise before any work is done.  (--clip is
    none of them: it runs into the reference's own NameError inside rpn_roi_PGD, attack_algo.py:110, in the first iteration.)"""
    check_unbuilt_model(args)
    if args.pertub_idx_se not in (1, 2, 3):
        raise ValueError(f"--pertub_idx_se {args.pertub_idx_se}: the feature map behind backbone layer 1, 2 or 3 is perturbed (the reference's "
                         "default of None fails in its first forward, backbone/resnet101_ori.py:203-262)")
    s = args.mix_layer
    if s is None or len(s) != 4 or any(c not in "01" for c in s):
        raise ValueError(f"--mix_layer {s}: four 0/1 digits, one per sample point 1..4 (the reference's default of None fails when it is "
                         "unpacked, train_aug_final.py:67)")
    if args.pertub_idx_sd != "roi":
        raise ValueError(f"--pertub_idx_sd {args.pertub_idx_sd}: only 'roi' (the reference reads ['roi_output_dict'] at train_aug_final.py:85, "
                         "which the dict of no other head pass holds)")


def final_settings(args):
    """The keyword settings of det_attack_algo.det_final_phases from the parsed flags."""
    return dict(pertub_idx_se=args.pertub_idx_se, mix_layer=args.mix_layer, gamma_se=args.gamma_se, gamma_sd=args.gamma_sd,
                sd_adv_loss_weight=args.sd_adv_loss_weight, only_roi_sd=args.only_roi_sd, mix_sd=args.mix_sd, noise_sd=args.noise_sd,
                randinit=args.randinit, clip=args.clip)


def check_unbuilt(args):
    """The reference's choices this build has nothing behind: raise before any work is done."""
    check_unbuilt_model(args)
    if args.loss_settings not in (1, 2, 3, 4):
        raise ValueError(f"--loss_settings {args.loss_settings}: the iteration knows settings 1 to 4 (the reference's default of 0 "
                         "asserts in its first iteration, train_aug_sat_muti_advt.py:165)")


def setup_device(program):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{program} needs an MI355X: this build has no CPU path (oracle/ is test infrastructure)")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------ the learning rate
def warmup_multistep_lr(t, base, milestones, gamma, factor, num_iters):
    """The reference's WarmUpMultiStepLR (extension/lr_scheduler.py) in closed form, t = the number of completed iterations: the first
    iteration runs at base * factor.  The reference was written against the closed-form MultiStepLR.get_lr; subclassing today's
    recursive one would compound the warm-up factors from step to step, which is not reproduced."""
    return base * gamma ** bisect.bisect_right(milestones, t) * (factor + (1 - factor) * t / num_iters if t < num_iters else 1)


def scheduler_state(step, cfg):
    """What stands in for scheduler.state_dict(): last_epoch and the five settings the closed form takes."""
    return {"last_epoch": int(step), "base_lr": cfg["learning_rate"], "milestones": list(cfg["step_lr_sizes"]), "gamma": cfg["step_lr_gamma"],
            "factor": cfg["warm_up_factor"], "num_iters": cfg["warm_up_num_iters"]}


def lr_at(step, cfg):
    return warmup_multistep_lr(step, cfg["learning_rate"], cfg["step_lr_sizes"], cfg["step_lr_gamma"], cfg["warm_up_factor"],
                               cfg["warm_up_num_iters"])


# ------------------------------------------------------------------------------------ checkpoints
def save_checkpoint(path_to_checkpoints_dir, step, model, optimizer, cfg):
    """Model.save (model.py:189-198)"""
    path_to_checkpoint = os.path.join(path_to_checkpoints_dir, f'model-{step}.pth')
    torch.save({'state_dict': model.state_dict(), 'step': step, 'optimizer_state_dict': optimizer.state_dict(),
                'scheduler_state_dict': scheduler_state(step, cfg)}, path_to_checkpoint)
    return path_to_checkpoint


def convert_dict(ori_dict):
    """model.py:420-437 as written: the keys of a checkpoint whose backbone was an nn.Sequential (`features.0.` .. `features.6`) renamed
    to this model's (`features.conv1.` .. `features.layer3`).  `str.replace` replaces EVERY occurrence of the digit, so a key that holds
    it twice (layer3's blocks 6 and 16, `features.4.2.conv1...` keeps its `conv1` only because the digit there is 1) comes out mangled
    and is then dropped by load_checkpoint's overlap rule: the `Load Weight:[k/n]` line shows it."""
    new_dict = {}
    for k, v in ori_dict.items():
        if "features.0." in k and "rpn" not in k:
            j = k.replace("0", "conv1")
        elif "features.1." in k:
            j = k.replace("1", "bn1")
        elif "features.4" in k:
            j = k.replace("4", "layer1")
        elif "features.5" in k:
            j = k.replace("5", "layer2")
        elif "features.6" in k:
            j = k.replace("6", "layer3")
        else:
            j = k
        new_dict[j] = v
    return new_dict


def load_checkpoint(path_to_checkpoint, model, optimizer=None, arena=None, convert=False):
    """Model.load (model.py:200-217): the keys the checkpoint and the model share are loaded, the rest keep their values -> step.
    convert: `convert_dict` on the checkpoint's keys first (:203-204)."""
    checkpoint = torch.load(path_to_checkpoint, map_location="cpu", weights_only=False)
    if convert:
        checkpoint['state_dict'] = convert_dict(checkpoint['state_dict'])
    model_state_dict = model.state_dict()
    overlap_dict = {k: v for k, v in checkpoint['state_dict'].items() if k in model_state_dict.keys()}
    model_state_dict.update(overlap_dict)
    model.load_state_dict(model_state_dict)
    if arena is not None:
        arena.refresh_shadow()
    print("Load Weight:[{}/{}], DIR:[{}]".format(len(overlap_dict.keys()), len(model_state_dict.keys()), path_to_checkpoint))
    if optimizer is not None:
        optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
    return checkpoint['step']


# ------------------------------------------------------------------------------------ the log
class Log:
    """logger.py: `%(asctime)s %(levelname)-8s %(message)s` on the console and appended to a file (no logging.basicConfig: a process
    may run the loop more than once)."""

    def __init__(self, path_to_log_file=None):
        self.path = path_to_log_file

    def i(self, message):
        line = '{} {:<8s} {}'.format(time.strftime('%Y-%m-%d %H:%M:%S', time.localtime()), 'INFO', message)
        print(line, flush=True)
        if self.path is not None:
            with open(self.path, 'a') as f:
                f.write(line + '\n')


# ------------------------------------------------------------------------------------ data and model
def build_split(args, cfg):
    """-> (images, boxes, classes, num_classes).  --synthetic N: sources of 5/8 of the sides asked for (600 x 1000 gives VOC's 375 x 500
    at most), so that the resize enlarges as it does on VOC."""
    if args.synthetic:
        hi = max(int(cfg["image_max_side"] * 0.5), 8)
        lo = max(min(int(cfg["image_min_side"] * 0.625), hi - 1), 7)
        s = det_data.SyntheticDetSplit(args.synthetic, seed=args.seed or 0, min_side=lo, max_side=hi)
        return s.images, s.boxes, s.classes, s.num_classes
    images, boxes, classes = det_data.load_voc_det(args.data_dir, args.dataset, True)
    return images, boxes, classes, 21


def build_model(args, cfg, num_classes):
    """train_aug_sat_muti_advt.py:35-43.  There are no ImageNet weights to download here (`pretrained=True`): the backbone starts from
    its seeded initialisation unless -r names a checkpoint, with every block's last BatchNorm weight x 0.2, which keeps the 33 residual
    blocks of an untrained network from overflowing (what bench.py and tests/golden/det_frcnn_* do)."""
    model = det_model.fasterrcnn_resnet101(num_classes, pooler_mode=cfg["pooler_mode"], anchor_ratios=tuple(tuple(r) for r in cfg["anchor_ratios"]),
                                           anchor_sizes=tuple(cfg["anchor_sizes"]), rpn_pre_nms_top_n=cfg["rpn_pre_nms_top_n"],
                                           rpn_post_nms_top_n=cfg["rpn_post_nms_top_n"],
                                           anchor_smooth_l1_loss_beta=cfg["anchor_smooth_l1_loss_beta"],
                                           proposal_smooth_l1_loss_beta=cfg["proposal_smooth_l1_loss_beta"])
    for b in model.modules():
        if isinstance(b, det_model.Bottleneck):
            b.bn3.weight.data.mul_(0.2)
    model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    return model.set_channels_last(args.layout == "nhwc")


# ------------------------------------------------------------------------------------ the loop
def _step_seed(seed, step):
    return (int(seed) * 1000003 + int(step)) % (1 << 62)


def train(model, loader, cfg, path_to_checkpoints_dir, log=None, path_to_resuming_checkpoint=None, loss_settings=1, seed=None, trainer=None):
    """train_aug_sat_muti_advt.py:45-211 around det_trainer.DetTrainer.step.  The learning rate of iteration t (t completed before it)
    is warmup_multistep_lr(t), written into optimizer.param_groups[0]["lr"] before the step.  The loss stays on the device until a
    `[Step s] Avg. Loss = ...` line needs the last 100.  A checkpoint every num_steps_to_snapshot steps and at the end; -r loads one
    and continues from its step, with the loader fast-forwarded to the epoch and batch that step stands at.  With a seed, the host
    and device generators are seeded from (seed, step) before every iteration, so a resumed run draws what the uninterrupted one
    drew (and DetTrainer draws no noise ahead of its iteration).  trainer: a det_trainer.DetTrainer on `model`, or a factory
    `trainer(model, cfg)` of one (train_aug_final.py and train_baseline.py: the same loop around another iteration); None: the
    multi-layer SAT iteration at `loss_settings`.  -> {"step", "lrs", "losses" (device tensors), "trainer"}."""
    log = log or Log()
    if trainer is None:
        trainer = det_trainer.DetTrainer(model, lr=cfg["learning_rate"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                                         loss_settings=loss_settings, noise_ahead=seed is None)
    elif not hasattr(trainer, "step"):
        trainer = trainer(model, cfg)
    optimizer = trainer.optimizer
    step = 0
    time_checkpoint = time.time()
    losses = deque(maxlen=100)
    should_stop = False
    num_steps_to_display = cfg["num_steps_to_display"]
    num_steps_to_snapshot = cfg["num_steps_to_snapshot"]
    num_steps_to_finish = cfg["num_steps_to_finish"]
    if len(loader) == 0:
        raise ValueError("the loader makes no batch: fewer tall and fewer fat images than the batch size")

    if path_to_resuming_checkpoint is not None:
        step = load_checkpoint(path_to_resuming_checkpoint, model, optimizer, trainer.arena)
        log.i(f'Model has been restored from file: {path_to_resuming_checkpoint}')
    log.i('Start training with {:d} GPUs ({:d} batches per GPU)'.format(trainer.world, loader.batch // max(loader.world, 1)))
    loader.epoch, skip = divmod(step, len(loader))
    lrs, all_losses = [], []

    while not should_stop:
        for image_batch, bboxes_batch, labels_batch, _ in loader.batches(skip):
            batch_size = image_batch.shape[0]
            lr = lr_at(step, cfg)
            optimizer.param_groups[0]["lr"] = lr
            lrs.append(lr)
            if seed is not None:
                torch.manual_seed(_step_seed(seed, step))
            r = trainer.step(image_batch, bboxes_batch, labels_batch)
            losses.append(r["loss"])
            all_losses.append(r["loss"])
            step += 1

            if step == num_steps_to_finish:
                should_stop = True

            if step % num_steps_to_display == 0:
                avg_loss = float(torch.stack([l.float().reshape(()) for l in losses]).sum()) / len(losses)     # the one read-back
                elapsed_time = time.time() - time_checkpoint
                time_checkpoint = time.time()
                steps_per_sec = num_steps_to_display / elapsed_time
                samples_per_sec = batch_size * steps_per_sec
                eta = (num_steps_to_finish - step) / steps_per_sec / 3600
                lr = lr_at(step, cfg)                                       # (scheduler.get_lr() after scheduler.step(): the next one)
                log.i(f'[Step {step}] Avg. Loss = {avg_loss:.6f}, LR = {lr:.8f} ({samples_per_sec:.2f} samples/sec; ETA {eta:.1f} hrs)')

            if step % num_steps_to_snapshot == 0 or should_stop:
                path_to_checkpoint = save_checkpoint(path_to_checkpoints_dir, step, model, optimizer, cfg)
                log.i(f'Model has been saved to {path_to_checkpoint}')

            if should_stop:
                break
        skip = 0

    log.i('Done')
    return {"step": step, "lrs": lrs, "losses": all_losses, "trainer": trainer}


def _run(program, args, cfg, path_to_checkpoints_dir, banner, trainer=None, loss_settings=1, first_line=None):
    """What the three programs do between their refusals and `FINISL!`: device, directory, train.log, banner, data, model, train()."""
    device = setup_device(program)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if not os.path.exists(path_to_checkpoints_dir):
        print("create dir:[{}]".format(path_to_checkpoints_dir))
        os.makedirs(path_to_checkpoints_dir)
    log = Log(os.path.join(path_to_checkpoints_dir, 'train.log'))
    log.i('Arguments:')
    for k, v in vars(args).items():
        log.i(f'\t{k} = {v}')
    log.i(describe(cfg))
    for line in banner:
        print(line)
    print(first_line if first_line is not None else "DATASET:[{}] DIR:[{}]".format(args.dataset, args.data_dir))
    images, boxes, classes, num_classes = build_split(args, cfg)
    loader = det_data.DetDeviceLoader(images, boxes, classes, cfg["batch_size"], device, True, cfg["image_min_side"], cfg["image_max_side"],
                                      seed=args.seed)
    log.i('Found {:d} samples'.format(len(images)))
    model = build_model(args, cfg, num_classes).to(device).train()
    out = train(model, loader, cfg, path_to_checkpoints_dir, log, args.resume_checkpoint, loss_settings, args.seed, trainer=trainer)
    print("=" * 100)
    print("FINISL!")
    print("=" * 100)
    return out


def trainer_factory(phases, final=None):
    return lambda model, cfg: det_trainer.DetTrainer(model, lr=cfg["learning_rate"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                                                     phases=phases, final=final)


def main(program, argv=None):
    args = get_full_argparser().parse_args(argv)
    print_args(args, 100)
    check_unbuilt(args)
    cfg = config(args)
    banner = ["-" * 100, "INFO: PID   : [{}]".format(os.getpid()), "-" * 100]
    return _run(program, args, cfg, checkpoints_dir(args), banner, loss_settings=args.loss_settings)


def final_banner(args, path_to_checkpoints_dir):
    """train_aug_final.py:273-283"""
    return ["-" * 100, "INFO: PID   : [{}]".format(os.getpid()),
            "EXP: [SE + SAT + MIX + SD] Dataset: [{}]".format(args.dataset),
            "SE : Layer:[{}]  MIX:[{}]  Gamma:[{}]  Eps:[{}]  Randinit:[{}] Clip:[{}]"
            .format(args.pertub_idx_se, args.mix_layer, args.gamma_se, args.eps, args.randinit, args.clip),
            "SD : Layer:[{}]  MIX:[{}]  Gamma:[{}]  AdvWeight:[{}] Noise:[{}] ROI:[{}]"
            .format(args.pertub_idx_sd, args.mix_sd, args.gamma_sd, args.sd_adv_loss_weight, args.noise_sd, args.only_roi_sd),
            "DIR:[{}]".format(path_to_checkpoints_dir), "-" * 100]


def main_final(program, argv=None):
    """train_aug_final.py:194-286"""
    args = get_full_argparser(get_final_argparser()).parse_args(argv)
    print_args(args, 100)
    check_unbuilt_final(args)
    cfg = config(args)
    d = final_checkpoints_dir(args)
    return _run(program, args, cfg, d, final_banner(args, d), trainer=trainer_factory("final", final_settings(args)))


def main_base(program, argv=None):
    """train_baseline.py:130-194"""
    args = get_full_argparser(get_base_argparser()).parse_args(argv)
    print_args(args, 100)
    print("INFO: PID   : [{}]".format(os.getpid()))
    check_unbuilt_model(args)
    cfg = config(args)
    return _run(program, args, cfg, base_checkpoints_dir(args), [], trainer=trainer_factory("base"),
                first_line="Training Baseline ! DATASET:[{}] DIR:[{}]".format(args.dataset, args.data_dir))


def adv_exp_name(args):
    """train_baseline_advtrain.py:167-169"""
    name = "s" + str(args.steps) + "g" + str(args.gamma) + "e" + str(args.eps)
    if args.randinit:
        name += "_rand"
    if args.clip:
        name += "_clip"
    return name


def adv_checkpoints_dir(args, create=False):
    """train_baseline_advtrain.py:175-179.  create: make the directory too, with the reference's `create dir:[...]` line only where it
    did not exist (main_adv leaves that to _run, behind the refusals)."""
    path = os.path.join(args.outputs_dir, 'ckpt-{:s}-{:s}-{:s}'.format(adv_exp_name(args), args.dataset, args.backbone))
    if create and not os.path.exists(path):
        print("create dir:[{}]".format(path))
        os.makedirs(path)
    return path


def check_unbuilt_adv(args):
    check_unbuilt_model(args)
    if args.steps < 0:
        raise ValueError(f"--steps {args.steps}: a number of PGD steps, 0 or more")


def adv_settings(args):
    """The keyword settings of det_attack_algo.det_adv_phases from the parsed flags."""
    return dict(steps=args.steps, eps=args.eps, gamma=args.gamma, randinit=args.randinit, clip=args.clip, noise=args.noise)


def adv_banner(args):
    """train_baseline_advtrain.py:195-199"""
    return ["-" * 100, "INFO: PID   : [{}]".format(os.getpid()),
            "EXP: Dataset:[{}] ADV Training Step:[{}] Gamma:[{}] Eps:[{}] Randinit:[{}] Clip:[{}]"
            .format(args.dataset, args.steps, args.gamma, args.eps, args.randinit, args.clip), "-" * 100]


def adv_trainer_factory(settings, noise_ahead=False):
    return lambda model, cfg: det_trainer.DetTrainer(model, lr=cfg["learning_rate"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                                                     phases="adv", adv=settings, noise_ahead=noise_ahead)


def main_adv(program, argv=None):
    """train_baseline_advtrain.py:126-202: PGD training on the image.  --noise host (the reference's draw) with --seed S: every
    iteration's host generator is seeded from (S, step), so a run resumed with -r draws what the uninterrupted run drew.  --noise
    device: the start comes from the device's own generator word, which is NOT one of the checkpoint's four keys (they are the
    reference's), so a resumed run draws other starts than the uninterrupted one.  Host noise is NOT drawn one iteration ahead
    (DetTrainer(noise_ahead=True) is there for it): on this iteration it gained less than the spread (profiles/det_adv_time.jsonl)."""
    args = get_full_adv_argparser().parse_args(argv)
    print_args(args, 100)
    check_unbuilt_adv(args)
    cfg = config(args)
    return _run(program, args, cfg, adv_checkpoints_dir(args), adv_banner(args), trainer=adv_trainer_factory(adv_settings(args)))
