"""Detection PGD training — the flags, defaults, stdout lines, `train.log` and checkpoint layout of the reference's
Detection/train_baseline_advtrain.py (an image-space sign-PGD on every batch, then one SGD step on the adversarial images, on
Faster-RCNN / ResNet-101): the model a robust mAP (eval_rob_ori.py) is normally compared against.  `bash cmd/run_det_adv.sh`.
Additions (all optional): --synthetic N, --dtype, --layout, --seed, --noise {host,device}.

The iteration body is det_attack_algo.det_adv_phases under det_trainer.DetTrainer(phases="adv"); loop, learning rate, log and
checkpoints are det_entry.train's, shared with the other Detection programs.  --noise says where --randinit's start is drawn: `host`
on torch's CPU generator as the reference does, `device` inside the start's own launch from a device-resident generator
(afan_pgd_rand_start).  With `--noise host --seed S` a run resumed with -r draws what the uninterrupted run drew; with `--noise device`
it does not: the checkpoint keeps the reference's four keys, and the device generator's word is not one of them.  Refused before any
work: backbones other than resnet101, datasets other than voc2007 / voc20072012, a negative --steps."""
import os
import sys

if __package__ in (None, ""):  # executed as a script (cmd/run_det_adv.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    det_entry = importlib.import_module("cv_a-fan_amd.det_entry")
else:
    from . import det_entry

get_argparser, print_args, ADDITIONS = det_entry.get_adv_argparser, det_entry.print_args, det_entry.ADV_ADDITIONS
get_full_argparser = det_entry.get_full_adv_argparser
exp_name, checkpoints_dir, check_unbuilt = det_entry.adv_exp_name, det_entry.adv_checkpoints_dir, det_entry.check_unbuilt_adv


def main(argv=None):
    return det_entry.main_adv("train_baseline_advtrain.py", argv)


if __name__ == '__main__':
    main()
