"""Detection baseline training — the flags, defaults, stdout lines, `train.log` and checkpoint layout of the reference's
Detection/train_baseline.py (one clean forward per iteration, the sum of the four losses' means, on Faster-RCNN / ResNet-101): what
an A-FAN mAP is compared against.  `bash cmd/run_det_base.sh`.  Additions (all optional): --synthetic N, --dtype, --layout, --seed.

The iteration body is det_attack_algo.det_base_phases under det_trainer.DetTrainer(phases="base"); loop, learning rate, log and
checkpoints are det_entry.train's, shared with the two A-FAN programs.  The reference's PGD flags are parsed and, as there, never
read.  Refused before any work: backbones other than resnet101 and datasets other than voc2007 / voc20072012."""
import os
import sys

if __package__ in (None, ""):  # executed as a script (cmd/run_det_base.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    det_entry = importlib.import_module("cv_a-fan_amd.det_entry")
else:
    from . import det_entry

get_argparser, print_args, ADDITIONS = det_entry.get_base_argparser, det_entry.print_args, det_entry.ADDITIONS
checkpoints_dir, check_unbuilt = det_entry.base_checkpoints_dir, det_entry.check_unbuilt_model


def get_full_argparser():
    return det_entry.get_full_argparser(get_argparser())


def main(argv=None):
    return det_entry.main_base("train_baseline.py", argv)


if __name__ == '__main__':
    main()
