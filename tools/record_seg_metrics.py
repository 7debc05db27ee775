"""Record tests/golden/seg_metrics.npz: what the reference's own StreamSegMetrics (Segmentation/metrics/stream_metrics.py) computes on
a handful of small (targets, predictions) sets.  Run on the CPU, with the reference checkout at hand (it needs scikit-learn to import):

    python tools/record_seg_metrics.py --reference /path/to/reference/Segmentation

The tool only CALLS the reference; the fixture holds data: per case the inputs of every update() call, the confusion matrix, the four
scalars, the class IoUs and the to_str() string.  tests/test_seg_metrics.py holds seg_eval.StreamSegMetrics to it."""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU")


def cases():
    """name -> (n_classes, [(targets [N,H,W] int64, preds [N,H,W] int64), ...]): one pair per update() call."""
    rng = np.random.default_rng(20240607)
    out = {}
    # 21 classes, three of them (5, 11, 20) in neither labels nor predictions: NaN IoUs that nanmean leaves out
    present = np.array([c for c in range(21) if c not in (5, 11, 20)])
    t = present[rng.integers(0, len(present), (2, 12, 16))]
    p = np.where(rng.random(t.shape) < 0.6, t, present[rng.integers(0, len(present), t.shape)])
    out["absent3"] = (21, [(t, p)])
    # class 3 is predicted but never labelled: IoU 0 (not NaN), accuracy of the class NaN
    t = rng.integers(0, 3, (1, 9, 7))
    p = np.where(rng.random(t.shape) < 0.3, 3, t)
    out["pred_only"] = (4, [(t, p)])
    # ignored pixels (255) and other out-of-range labels are masked out
    t = rng.integers(0, 21, (2, 10, 10))
    t[rng.random(t.shape) < 0.25] = 255
    t[0, 0, :3] = 21
    t[1, 5, 5] = 254
    p = rng.integers(0, 21, t.shape)
    out["ignore255"] = (21, [(t, p)])
    # one class only, predicted perfectly
    t = np.full((1, 6, 6), 7)
    out["single_class"] = (21, [(t, t.copy())])
    # two update() calls into one matrix
    a = rng.integers(0, 5, (2, 8, 8))
    b = rng.integers(0, 5, (3, 5, 9))
    b[rng.random(b.shape) < 0.1] = 255
    out["two_updates"] = (5, [(a, np.where(rng.random(a.shape) < 0.7, a, rng.integers(0, 5, a.shape))),
                              (b, rng.integers(0, 5, b.shape))])
    return {k: (n, [(t.astype(np.int64), p.astype(np.int64)) for t, p in calls]) for k, (n, calls) in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Segmentation directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "seg_metrics.npz"))
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.reference))
    from metrics.stream_metrics import StreamSegMetrics
    rec = {"names": np.array(sorted(cases()))}
    for name, (n, calls) in cases().items():
        m = StreamSegMetrics(n)
        for i, (t, p) in enumerate(calls):
            rec[f"{name}/targets_{i}"], rec[f"{name}/preds_{i}"] = t, p
            m.update(t, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # (the reference divides by zero for absent classes)
            r = m.get_results()
        assert list(r) == list(SCALARS) + ["Class IoU"]
        rec[f"{name}/n_classes"] = np.int64(n)
        rec[f"{name}/n_updates"] = np.int64(len(calls))
        rec[f"{name}/confusion"] = np.asarray(m.confusion_matrix, np.float64)
        rec[f"{name}/scalars"] = np.array([r[k] for k in SCALARS], np.float64)
        rec[f"{name}/class_iou"] = np.array([r["Class IoU"][c] for c in range(n)], np.float64)
        rec[f"{name}/to_str"] = np.array(m.to_str(r))
        print(name, rec[f"{name}/scalars"], int(np.isnan(rec[f"{name}/class_iou"]).sum()), "NaN IoUs")
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
