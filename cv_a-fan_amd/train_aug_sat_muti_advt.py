"""Detection A-FAN training entry point — the flags, defaults, stdout lines, `train.log` and checkpoint layout of the reference's
Detection/train_aug_sat_muti_advt.py (multi-layer SAT feature perturbation + image-PGD adversarial training on Faster-RCNN /
ResNet-101), so `bash cmd/run_det.sh` works.  Additions (all optional): --synthetic N, --dtype, --layout, --seed.

What differs from the reference is execution only: the iteration body is det_trainer.DetTrainer.step (HIP kernels), the batch —
mirror, resize to min side 600 / max side 1000, padding, boxes — is built on the device by det_data.DetDeviceLoader in one launch
instead of eight DataLoader workers, the learning rate is WarmUpMultiStepLR's closed form (det_entry.warmup_multistep_lr), and the
loss stays on the device until a `[Step s] Avg. Loss = ...` line needs it.

Not built here: backbones other than resnet101 and datasets other than voc2007 / voc20072012 (they raise, each with its reason);
tensorboardX summaries (not installed: none are written); ImageNet weights (no download: see det_entry.build_model).  Evaluation is
eval.py."""
import os
import sys

if __package__ in (None, ""):  # executed as a script (cmd/run_det.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    det_entry = importlib.import_module("cv_a-fan_amd.det_entry")
else:
    from . import det_entry

get_argparser, get_full_argparser, print_args, ADDITIONS = (det_entry.get_argparser, det_entry.get_full_argparser, det_entry.print_args,
                                                            det_entry.ADDITIONS)
exp_name, checkpoints_dir = det_entry.exp_name, det_entry.checkpoints_dir


def main(argv=None):
    return det_entry.main("train_aug_sat_muti_advt.py", argv)


if __name__ == '__main__':
    main()
