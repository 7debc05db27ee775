"""Detection robust evaluation entry point — the flags, `results-...` directory, `eval.log`, `comp3_det_test_{category}.txt` files and
the `syd: pgd attack mean AP = ...` line of the reference's Detection/eval_rob_ori.py, so `bash cmd/run_det_rob.sh` works: VOC mAP of
the detections on images moved by an image-space PGD under the sum of the four training losses (attack_algo.eval_PGD: --steps 10,
--gamma 0.5 and --eps 2 in 1/255, --randinit, --clip; no clamp to [0, 1]).  --convert renames the keys of a checkpoint whose backbone
was an nn.Sequential before the overlap load (model.py:420-437, as written).  Additions (all optional): --synthetic N, --dtype, --layout.

Execution: det_eval.RobustEvaluator — det_attack_algo.eval_PGD on the sign-PGD core with input-gradient-only backward passes, then
eval.py's forward and metric.  An image without a non-difficult object has no loss; it is scored unattacked and counted in the log.

Not built: eval_rob.py (the reference's other robust evaluation is dead code: it calls attack_algo.untarget_PGD, which is commented
out), COCO; backbones other than resnet101 (they raise, each with its reason)."""
import os
import sys

if __package__ in (None, ""):  # executed as a script (cmd/run_det_rob.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    det_eval = importlib.import_module("cv_a-fan_amd.det_eval")
else:
    from . import det_eval

get_argparser, ADDITIONS = det_eval.get_rob_argparser, det_eval.ADDITIONS


def main(argv=None):
    return det_eval.main_rob("eval_rob_ori.py", argv)


if __name__ == '__main__':
    main()
