"""Record tests/golden/det_voc_eval.npz: what the reference's own VOC evaluation (Detection/voc_eval.py `voc_eval` / `voc_ap`, and
`VOC2007.evaluate` of Detection/dataset/voc2007.py around them) computes on a few small annotation trees and detection lists.  Run on
the CPU, with the reference checkout at hand:

    python tools/record_det_eval.py --reference /path/to/reference/Detection

The tool only CALLS the reference; the fixture holds data.  Per case it writes a VOCdevkit/VOC2007 tree (ImageSets/Main/test.txt and
one annotation file per image; no pictures: the evaluation reads none) into a temporary directory, hands the detection lists to
`VOC2007.evaluate` (which writes the results files and returns the mean AP and the detail string), then calls `voc_eval` on each
results file for the class's recall and precision curves.  Stored: the ground truth and the detections as arrays, per class rec, prec,
AP and whether the reference raised its IndexError (a class without a detection), the mean and the detail string.
tests/test_det_eval_metric.py holds det_eval to it.

Two things the reference needs to run today: `np.bool` (set to `bool` where numpy has dropped it), and `torchvision` to IMPORT
dataset/base.py (its `evaluate` never touches it; an empty stand-in module is registered when it is not installed)."""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CATEGORIES = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse',
              'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']            # labels 1..20


def _f32(v):
    """A Python float holding an fp32 value: what `tensor.tolist()` hands the evaluation."""
    return float(np.float32(v))


def cases():
    """name -> (image ids, gt rows (image, label, difficult, [xmin, ymin, xmax, ymax]), detection rows (image, label, prob, box))."""
    out = {}
    # ---- every special case by hand
    ids = ["000001", "000002", "000003", "000004"]
    gt = [(0, 7, 0, [48, 240, 195, 371]), (0, 7, 1, [8, 12, 352, 498]), (0, 15, 0, [100, 50, 200, 300]),
          (1, 12, 0, [10, 10, 100, 100]), (1, 15, 0, [20, 30, 120, 230]), (1, 15, 1, [200, 100, 260, 220]),
          (2, 3, 0, [30, 40, 130, 140]), (2, 18, 0, [5, 5, 300, 200]), (2, 15, 0, [150, 20, 290, 330]),
          (3, 9, 1, [60, 60, 160, 160])]
    det = [
        # car: a hit, its duplicate (false positive), one whose best match is the difficult car (neither), one in an image without a car
        (0, 7, 0.953125017, [47.12345678, 239.7654321, 194.3333333, 370.6666667]),
        (0, 7, 0.9011112, [50.5, 243.25, 199.0000004, 368.9999996]),
        (0, 7, 0.85, [9.1234567, 13.7654321, 350.0000001, 497.4999999]),
        (2, 7, 0.6, [10.0, 10.0, 90.0, 90.0]),
        # person: two of three found, a false positive in between, one on the difficult person: recall stops at 2 / 3
        (0, 15, 0.881, [99.4444444, 49.5555555, 201.1111111, 299.2222222]),
        (3, 15, 0.7500001, [0.0, 0.0, 50.0, 50.0]),
        (1, 15, 0.7, [22.0, 33.0, 118.0, 228.0]),
        (1, 15, 0.31, [201.0, 101.0, 259.0, 219.0]),
        # dog: misplaced (IoU below 0.5): recall stays 0, the 11-point metric finds `rec >= t` empty from t = 0.1 on
        (1, 12, 0.5, [60.0, 60.0, 160.0, 160.0]),
        # bird: found
        (2, 3, 0.99, [29.0, 39.0, 129.0, 139.0]),
        # chair: the only ground truth is difficult: npos = 0
        (3, 9, 0.4, [59.0, 59.0, 159.0, 159.0]),
        # bottle: detections, no ground truth anywhere
        (0, 5, 0.3, [1.0, 2.0, 30.0, 40.0]), (3, 5, 0.2, [5.0, 6.0, 70.0, 80.0]),
        # sofa (18): ground truth, no detection
    ]
    out["by_hand"] = (ids, gt, det)

    # ---- five detections of one class
    ids = ["000010", "000011"]
    gt = [(0, 1, 0, [10, 10, 110, 110]), (0, 1, 0, [200, 200, 300, 300]), (1, 1, 0, [50, 50, 150, 250])]
    det = [(0, 1, 0.9, [11.0, 11.0, 109.0, 111.0]), (1, 1, 0.8, [300.0, 300.0, 350.0, 350.0]), (0, 1, 0.7, [198.0, 202.0, 301.0, 297.0]),
           (1, 1, 0.6, [52.0, 48.0, 149.0, 251.0]), (0, 1, 0.55, [12.0, 12.0, 108.0, 108.0])]
    out["five"] = (ids, gt, det)

    # ---- seeded: jittered copies of the ground truth among random boxes, over eight classes
    rng = np.random.default_rng(20240911)
    ids = ["%06d" % (100 + i) for i in range(7)]
    gt, det = [], []
    for i in range(len(ids)):
        for _ in range(int(rng.integers(0, 5))):
            x0, y0 = int(rng.integers(1, 300)), int(rng.integers(1, 200))
            w, h = int(rng.integers(20, 180)), int(rng.integers(20, 160))
            label = int(rng.integers(1, 9))
            gt.append((i, label, int(rng.random() < 0.25), [x0, y0, x0 + w, y0 + h]))
            for _ in range(int(rng.integers(0, 3))):
                j = rng.normal(0, 0.07, 4) * np.array([w, h, w, h])
                b = np.array([x0 - 1, y0 - 1, x0 + w - 1, y0 + h - 1], np.float64) + j
                det.append((i, label, float(rng.random()), b.astype(np.float32).astype(np.float64)))
    for _ in range(25):
        i = int(rng.integers(0, len(ids)))
        x0, y0 = rng.random() * 300, rng.random() * 200
        det.append((i, int(rng.integers(1, 11)), float(rng.random()), [x0, y0, x0 + 10 + rng.random() * 150, y0 + 10 + rng.random() * 150]))
    out["seeded"] = (ids, gt, det)
    return {k: (ids, gt, [(i, c, _f32(p), [_f32(v) for v in b]) for i, c, p, b in det]) for k, (ids, gt, det) in out.items()}


def write_tree(root, ids, gt):
    voc = os.path.join(root, "VOCdevkit", "VOC2007")
    os.makedirs(os.path.join(voc, "ImageSets", "Main"))
    os.makedirs(os.path.join(voc, "Annotations"))
    with open(os.path.join(voc, "ImageSets", "Main", "test.txt"), "w") as f:
        f.write("".join(i + "\n" for i in ids))
    for k, image_id in enumerate(ids):
        objs = "".join(
            "<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
            "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>" % ((CATEGORIES[c - 1], d) + tuple(b))
            for i, c, d, b in gt if i == k)
        with open(os.path.join(voc, "Annotations", image_id + ".xml"), "w") as f:
            f.write("<annotation><folder>VOC2007</folder><filename>%s.jpg</filename><size><width>500</width><height>375</height>"
                    "<depth>3</depth></size>%s</annotation>" % (image_id, objs))
    return voc


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Detection directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "det_voc_eval.npz"))
    a = ap.parse_args(argv)
    if not hasattr(np, "bool"):
        np.bool = bool                                         # voc_eval.py:126
    try:
        import torchvision  # noqa: F401
    except ImportError:
        tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tr.transforms, tv.transforms = tr, tr
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    sys.path.insert(0, os.path.abspath(a.reference))
    import voc_eval as ref
    from dataset.voc2007 import VOC2007

    rec = {"names": np.array(sorted(cases()))}
    home = os.getcwd()
    for name, (ids, gt, det) in cases().items():
        for c in range(1, 21):                                 # the test's premise: numpy's sort is never asked to break a tie
            conf = [float('{:f}'.format(p)) for _, cc, p, _ in det if cc == c]
            assert len(set(conf)) == len(conf), (name, c)
        with tempfile.TemporaryDirectory() as tmp:
            voc = write_tree(tmp, ids, gt)
            results = os.path.join(tmp, "results")
            os.makedirs(results)
            os.chdir(tmp)                                      # the reference caches the parsed annotations under ./caches
            try:
                with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
                    warnings.simplefilter("ignore")            # (the reference divides by npos = 0)
                    dataset = VOC2007(tmp, VOC2007.Mode.EVAL, 600., 1000.)
                    mean_ap, detail = dataset.evaluate(results, [ids[i] for i, _, _, _ in det], [b for _, _, _, b in det],
                                                       [c for _, c, _, _ in det], [p for _, _, p, _ in det])
                    aps, raised = np.zeros(20), np.zeros(20, bool)
                    for c in range(1, 21):
                        try:
                            r, p, v = ref.voc_eval(os.path.join(results, "comp3_det_test_%s.txt" % CATEGORIES[c - 1]),
                                                   os.path.join(voc, "Annotations", "{:s}.xml"),
                                                   os.path.join(voc, "ImageSets", "Main", "test.txt"), CATEGORIES[c - 1],
                                                   os.path.join("caches", "voc2007"), ovthresh=0.5, use_07_metric=True)
                            rec[f"{name}/rec_{c}"], rec[f"{name}/prec_{c}"], aps[c - 1] = np.asarray(r, np.float64), np.asarray(p, np.float64), v
                            rec[f"{name}/ap_all_points_{c}"] = np.float64(ref.voc_ap(r, p, False))
                        except IndexError:
                            raised[c - 1] = True
                files = {c: open(os.path.join(results, "comp3_det_test_%s.txt" % CATEGORIES[c - 1])).read() for c in range(1, 21)}
            finally:
                os.chdir(home)
        rec[f"{name}/image_ids"] = np.array(ids)
        rec[f"{name}/gt_image"] = np.array([g[0] for g in gt], np.int64)
        rec[f"{name}/gt_class"] = np.array([g[1] for g in gt], np.int64)
        rec[f"{name}/gt_difficult"] = np.array([g[2] for g in gt], bool)
        rec[f"{name}/gt_box"] = np.array([g[3] for g in gt], np.int64).reshape(-1, 4)
        rec[f"{name}/det_image"] = np.array([d[0] for d in det], np.int64)
        rec[f"{name}/det_class"] = np.array([d[1] for d in det], np.int64)
        rec[f"{name}/det_prob"] = np.array([d[2] for d in det], np.float64)
        rec[f"{name}/det_box"] = np.array([d[3] for d in det], np.float64).reshape(-1, 4)
        rec[f"{name}/ap"], rec[f"{name}/raised"] = aps, raised
        rec[f"{name}/mean_ap"] = np.float64(mean_ap)
        rec[f"{name}/detail"] = np.array(detail)
        rec[f"{name}/results_files"] = np.array([files[c] for c in range(1, 21)])
        print(name, "mean AP", mean_ap, "raised", int(raised.sum()), "APs", np.round(aps, 4).tolist())
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
