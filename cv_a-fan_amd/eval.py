"""Detection evaluation entry point — the flags, `results-...` directory, `eval.log`, `comp3_det_test_{category}.txt` files and the
`mean AP = ...` line of the reference's Detection/eval.py, so `bash cmd/run_det_eval.sh` works.  Additions (all optional):
--synthetic N, --dtype, --layout.

What differs from the reference is execution only: the forward is det_model's eval mode, whose tail (decode, clip, score filter, sort,
NMS for all 20 classes) is one launch (det_ops.class_nms); the batch is built on the device by det_data.DetDeviceLoader; the metric
is det_eval's restatement of voc_eval.py on in-memory arrays, with the reference's text round trip applied to the numbers.

Robust mAP is its own program, eval_rob_ori.py (the reference's working one).  Not built: eval_rob.py (the reference's dead one: it
calls attack_algo.untarget_PGD, which is commented out), COCO; backbones other than resnet101 (they raise,
each with its reason)."""
import os
import sys

if __package__ in (None, ""):  # executed as a script (cmd/run_det_eval.sh): import the hyphenated package by path
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    det_eval = importlib.import_module("cv_a-fan_amd.det_eval")
else:
    from . import det_eval

get_argparser, get_full_argparser, ADDITIONS = det_eval.get_argparser, det_eval.get_full_argparser, det_eval.ADDITIONS


def main(argv=None):
    return det_eval.main("eval.py", argv)


if __name__ == '__main__':
    main()
