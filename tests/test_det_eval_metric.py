"""det_eval's VOC metric against what the reference's own voc_eval / voc_ap / VOC2007.evaluate computed (tests/golden/det_voc_eval.npz,
recorded by tools/record_det_eval.py): recall and precision curves, APs and the mean to 1e-12 (the same float64 numpy operations in
the same order: slack for another numpy build only), the detail string and the results files exactly.  Between them the cases hold a
duplicate detection, a best match on a difficult object, a detection in an image without the class, a class with detections and no
ground truth, one with ground truth and no detection, coordinates the six-decimal round trip changes, and recall curves the 11-point
metric finds empty."""
import os

import numpy as np
import pytest

from conftest import golden


@pytest.fixture(scope="module")
def fx():
    return golden("det_voc_eval")


def _case(fx, name):
    ids = [str(s) for s in fx[f"{name}/image_ids"]]
    gi, gc, gd, gb = (fx[f"{name}/gt_{k}"] for k in ("image", "class", "difficult", "box"))
    gt = {image_id: (gc[gi == k], gd[gi == k], gb[gi == k]) for k, image_id in enumerate(ids)}
    di, dc, dp, db = (fx[f"{name}/det_{k}"] for k in ("image", "class", "prob", "box"))
    return gt, [ids[k] for k in di], db.tolist(), dc.tolist(), dp.tolist()


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= 1e-12) | (np.isnan(a) & np.isnan(b))))


def test_fixture_holds_the_cases_it_is_meant_to(fx, pkg):
    names = [str(n) for n in fx["names"]]
    assert names == ["by_hand", "five", "seeded"]
    gt, ids, boxes, classes, probs = _case(fx, "by_hand")
    raised = fx["by_hand/raised"]
    assert raised[18 - 1] and any(18 in c for c, _, _ in gt.values())                        # ground truth, no detection
    assert not raised[5 - 1] and not any(5 in c for c, _, _ in gt.values())                  # detections, no ground truth
    assert any(c == 7 and 7 not in gt[i][0] for i, c in zip(ids, classes))                    # a detection in an image without the class
    assert any(all(d for d in dd) and len(dd) for _, dd, _ in gt.values())                    # an image with difficult objects only
    rt = pkg.det_eval.round_trip
    assert any(rt(v) != v for b in boxes for v in b) and any(rt(p) != p for p in probs)       # the round trip changes numbers
    assert np.isnan(fx["by_hand/rec_9"]).all()                                               # npos = 0: the reference's 0 / 0
    assert (fx["by_hand/rec_12"] == 0).all() and fx["by_hand/ap"][12 - 1] == 0               # `rec >= t` empty from t = 0.1 on
    assert fx["by_hand/rec_15"].max() < 1                                                    # ... and above 2 / 3 here
    for name in names:                                                                       # no ties for numpy's sort to break
        _, _, _, classes, probs = _case(fx, name)
        for c in set(classes):
            conf = [rt(p) for p, cc in zip(probs, classes) if cc == c]
            assert len(set(conf)) == len(conf)


@pytest.mark.parametrize("name", ["by_hand", "five", "seeded"])
def test_metric_equals_the_reference(fx, pkg, name, tmp_path):
    de = pkg.det_eval
    gt, ids, boxes, classes, probs = _case(fx, name)
    mean_ap, detail, results = de.evaluate_detail(gt, ids, boxes, classes, probs, str(tmp_path))
    assert detail == str(fx[f"{name}/detail"])
    assert abs(mean_ap - float(fx[f"{name}/mean_ap"])) <= 1e-12
    assert (mean_ap, detail) == de.evaluate(gt, ids, boxes, classes, probs)
    for c in range(1, 21):
        rec, prec, ap = results[c]
        if fx[f"{name}/raised"][c - 1]:
            assert rec is None and prec is None and ap == 0
            continue
        assert _close(rec, fx[f"{name}/rec_{c}"]) and _close(prec, fx[f"{name}/prec_{c}"]), c
        assert abs(ap - fx[f"{name}/ap"][c - 1]) <= 1e-12, c
        assert abs(de.voc_ap(rec, prec, False) - float(fx[f"{name}/ap_all_points_{c}"])) <= 1e-12 or \
            (np.isnan(de.voc_ap(rec, prec, False)) and np.isnan(fx[f"{name}/ap_all_points_{c}"])), c
        cat = de.LABEL_TO_CATEGORY_DICT[c]
        assert open(os.path.join(str(tmp_path), f"comp3_det_test_{cat}.txt")).read() == str(fx[f"{name}/results_files"][c - 1])
    assert sorted(os.listdir(str(tmp_path))) == sorted(f"comp3_det_test_{de.LABEL_TO_CATEGORY_DICT[c]}.txt" for c in range(1, 21))


def test_duplicate_and_difficult_by_hand(pkg):
    """The two rules stated on their own: the second detection of one object is a false positive; a best match on a difficult object
    counts neither way and the object is nobody's positive."""
    de = pkg.det_eval
    gt = {"a": (np.array([1, 1]), np.array([False, True]), np.array([[10, 10, 60, 60], [100, 100, 180, 180]]))}
    rec, prec, ap = de.voc_eval(gt, 1, ["a", "a", "a"], [0.9, 0.8, 0.7], [[10, 10, 60, 60], [100, 100, 180, 180], [11, 11, 61, 61]], 0.5, True)
    assert rec.tolist() == [1.0, 1.0, 1.0] and prec.tolist() == [1.0, 1.0, 0.5] and abs(ap - 1.0) < 1e-12
    with pytest.raises(IndexError):
        de.voc_eval(gt, 2, [], [], [])
