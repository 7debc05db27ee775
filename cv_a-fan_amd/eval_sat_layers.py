"""Detection layer-wise SAT evaluation entry point — the flags, `results-...` directory, `eval.log`, `comp3_det_test_{category}.txt`
files and the `SAT LAYER:[..] MIX:[..]` / `mean AP = ...` lines of the reference's Detection/eval_sat_layers.py, so
`bash cmd/run_det_sat.sh` works: VOC mAP of the detections when the backbone feature map behind layer --pertub_idx (1..3) is replaced
by sample point --sat_layer (0 = clean .. 4 = adversarial) of the line from its clean value to its feature-PGD value (attack_algo.PGD:
--steps 10, --gamma 0.5 and --eps 2 in 1/255, --randinit, --clip).  --mix re-normalises the point with mix_feature(point, clean map):
the argument order is REVERSED against the training scripts — the point is normalised, the clean map's per-pixel channel statistics
are the target.  Additions (all optional): --synthetic N, --dtype, --layout, and --table: all ten (sat_layer, mix) settings from one
attack per image and one launch for the ten points, one more log line per setting.

Execution: det_eval.SatLayerEvaluator.  --pertub_idx outside 1..3 (the reference's default 0 asserts in its backbone) and --sat_layer
outside 0..4 raise ValueError before any work.  An image without a non-difficult object has no loss; it is scored from its clean
feature and counted in the log.

Not built: eval_loss_vis.py, COCO; backbones other than resnet101 (they raise, each with its reason)."""
import os
import sys

if __package__ in (None, ""):  # executed as a script (cmd/run_det_sat.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    det_eval = importlib.import_module("cv_a-fan_amd.det_eval")
else:
    from . import det_eval

get_argparser, ADDITIONS = det_eval.get_sat_argparser, det_eval.SAT_ADDITIONS


def main(argv=None):
    return det_eval.main_sat("eval_sat_layers.py", argv)


if __name__ == '__main__':
    main()
