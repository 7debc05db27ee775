"""eval.py without a GPU: its parser against the names and defaults recorded from the reference's own parser
(tests/golden/det_eval_args.json), the EvalConfig defaults, the refusals before any device work, load_voc_det_eval on a three-image
VOCdevkit tree, the results files' lines, and the argument errors of afan_det_class_nms / afan_det_pack."""
import ctypes
import importlib
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.eval")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


BASE = ["-s", "voc2007", "-b", "resnet101", "model-1.pth"]


def test_parser_equals_the_references(entry, pkg):
    ref = json.load(open(os.path.join(GOLDEN, "det_eval_args.json")))
    assert len(ref) == 11 and ref[-1] == {"dest": "checkpoint", "flags": [], "default": None}
    assert _table(entry.get_argparser()) == ref                   # same options, same order, same defaults
    full = _table(entry.get_full_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == entry.ADDITIONS == ("synthetic", "dtype", "layout")
    o = entry.get_full_argparser().parse_args(BASE)
    assert (o.synthetic, o.dtype, o.layout, o.checkpoint, o.data_dir) == (0, "bf16", "nhwc", "model-1.pth", "./data")
    with pytest.raises(SystemExit):
        entry.get_full_argparser().parse_args(["-s", "voc2007", "-b", "resnet101"])          # the checkpoint is required


def test_eval_config_defaults(entry, pkg):
    de = pkg.det_eval
    cfg = de.config(entry.get_full_argparser().parse_args(BASE))
    assert cfg == {"image_min_side": 600.0, "image_max_side": 1000.0, "anchor_ratios": [(1, 2), (1, 1), (2, 1)], "anchor_sizes": [128, 256, 512],
                   "pooler_mode": "align", "rpn_pre_nms_top_n": 6000, "rpn_post_nms_top_n": 300}
    cfg = de.config(entry.get_full_argparser().parse_args(BASE + ["--rpn_post_nms_top_n", "100", "--anchor_sizes", "[64]", "--image_min_side", "128"]))
    assert (cfg["rpn_post_nms_top_n"], cfg["rpn_pre_nms_top_n"], cfg["anchor_sizes"], cfg["image_min_side"]) == (100, 6000, [64], 128.0)
    assert pkg.det_entry.DEFAULTS["rpn_post_nms_top_n"] == 2000               # (the training configuration is not touched)
    assert de.MIN_PROB == 0.05


def test_results_directory_name(pkg):
    d = pkg.det_eval.results_dir(os.path.join("out", "ckpt-x", "model-90000.pth"))
    assert os.path.dirname(d) == os.path.join("out", "ckpt-x")
    assert re.fullmatch(r"results-\d{14}-model-90000-[0-9a-f]{8}", os.path.basename(d))


@pytest.mark.parametrize("argv, word", [(["-s", "voc2007", "-b", "resnet18"], "BasicBlock"), (["-s", "voc2007", "-b", "resnet50"], "ResNet-101 is pinned"),
                                        (["-s", "coco2017", "-b", "resnet101"], "pycocotools"),
                                        (["-s", "voc2007-cat-dog", "-b", "resnet101"], "cat / dog subset")])
def test_refusals_come_before_any_device_work(entry, argv, word, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for before the refusal"))
    with pytest.raises(NotImplementedError, match=word):
        entry.main(argv + [str(tmp_path / "model-1.pth")])
    assert os.listdir(tmp_path) == []                                          # no results directory either


def test_entry_fails_loudly_without_a_gpu(entry, monkeypatch, tmp_path):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        entry.main(["-s", "voc2007", "-b", "resnet101", "--synthetic", "4", str(tmp_path / "model-1.pth")])
    assert os.listdir(tmp_path) == []


def test_load_voc_det_eval_reads_a_tiny_tree(pkg, tmp_path):
    """Three images: one with an easy and a difficult object, one whose only object is difficult (it stays in the list, with no box
    for the loader), one plain.  The loader's boxes carry the `- 1`, the ground truth the XML's own integers."""
    Image = pytest.importorskip("PIL.Image")
    voc = tmp_path / "VOCdevkit" / "VOC2007"
    for d in ("ImageSets/Main", "Annotations", "JPEGImages"):
        os.makedirs(voc / d)
    (voc / "ImageSets/Main/test.txt").write_text("000001\n000002\n000003\n")
    obj = "<object><name>{}</name><difficult>{}</difficult><bndbox><xmin>{}</xmin><ymin>{}</ymin><xmax>{}</xmax><ymax>{}</ymax></bndbox></object>"
    xml = "<annotation><filename>{}.jpg</filename><size><width>12</width><height>10</height></size>{}</annotation>"
    (voc / "Annotations/000001.xml").write_text(xml.format("000001", obj.format("dog", 0, 2, 3, 9, 8) + obj.format("cat", 1, 1, 1, 5, 5)))
    (voc / "Annotations/000002.xml").write_text(xml.format("000002", obj.format("person", 1, 1, 1, 5, 5)))
    (voc / "Annotations/000003.xml").write_text(xml.format("000003", obj.format("tvmonitor", 0, 1, 1, 12, 10)))
    for n in ("000001", "000002", "000003"):
        Image.fromarray(np.full((10, 12, 3), 90, np.uint8)).save(voc / f"JPEGImages/{n}.jpg")
    images, boxes, classes, ids, gt = pkg.det_data.load_voc_det_eval(str(tmp_path), "voc20072012")
    assert ids == ["000001", "000002", "000003"] and len(images) == 3 and images[1].shape == (10, 12, 3)
    assert [b.tolist() for b in boxes] == [[[1., 2., 8., 7.]], [], [[0., 0., 11., 9.]]] and [b.dtype for b in boxes] == [np.float32] * 3
    assert [b.shape for b in boxes] == [(1, 4), (0, 4), (1, 4)] and [c.tolist() for c in classes] == [[12], [], [20]]
    assert list(gt) == ids
    assert gt["000001"][0].tolist() == [12, 8] and gt["000001"][1].tolist() == [False, True]
    assert gt["000001"][2].tolist() == [[2, 3, 9, 8], [1, 1, 5, 5]] and gt["000001"][2].dtype == np.int64
    assert gt["000002"][0].tolist() == [15] and gt["000002"][1].tolist() == [True] and gt["000002"][2].tolist() == [[1, 1, 5, 5]]
    # the split packs (an image without a box included) and scores: a detection on the easy dog, one on the difficult person
    pkg.det_data.pack_det_split(images, boxes, classes)
    mean_ap, detail = pkg.det_eval.evaluate(gt, ["000001", "000002"], [[1., 2., 8., 7.], [0., 0., 4., 4.]], [12, 15], [0.9, 0.8])
    assert mean_ap == pytest.approx(1 / 20) and "12: dog AP = 1.0000\n" in detail and "15: person AP = 0.0000\n" in detail
    with pytest.raises(FileNotFoundError, match="test.txt"):
        pkg.det_data.load_voc_det_eval(str(tmp_path / "nowhere"), "voc2007")
    with pytest.raises(ValueError, match="voc2007 and voc20072012"):
        pkg.det_data.load_voc_det_eval(str(tmp_path), "coco2017")


def test_synthetic_split_names_its_images_and_ground_truth(pkg):
    s = pkg.det_data.SyntheticDetSplit(3, seed=1)
    assert s.image_ids == ["000000", "000001", "000002"]
    gt = s.ground_truth()
    for i, b, c in zip(s.image_ids, s.boxes, s.classes):
        assert gt[i][0].tolist() == c.tolist() and not gt[i][1].any() and gt[i][2].dtype == np.int64
        assert gt[i][2].tolist() == (b + 1).tolist()


def test_results_lines_follow_the_format(pkg, tmp_path):
    de = pkg.det_eval
    assert de.result_line("000007", 0.9531250171, [47.12345678, 239.7, 194.0, 370.66666666]) == \
        "000007 0.953125 47.123457 239.700000 194.000000 370.666667\n"
    de.write_results(str(tmp_path), ["000001", "000002", "000001"], [[1.5, 2.0, 3.0, 4.0], [0.0, 0.0, 9.0, 9.0], [5.0, 6.0, 7.0, 8.25]], [7, 20, 7],
                     [0.75, 0.0612345678, 0.5])
    assert sorted(os.listdir(tmp_path)) == sorted(f"comp3_det_test_{de.LABEL_TO_CATEGORY_DICT[c]}.txt" for c in range(1, 21))
    assert open(tmp_path / "comp3_det_test_car.txt").read() == "000001 0.750000 1.500000 2.000000 3.000000 4.000000\n" \
                                                               "000001 0.500000 5.000000 6.000000 7.000000 8.250000\n"
    assert open(tmp_path / "comp3_det_test_tvmonitor.txt").read() == "000002 0.061235 0.000000 0.000000 9.000000 9.000000\n"
    assert open(tmp_path / "comp3_det_test_dog.txt").read() == ""
    assert de.round_trip(0.0612345678) == 0.061235


def test_class_nms_argument_errors_without_gpu(pkg):
    lib = pkg._lib.load()
    cap = 2048
    assert [lib.afan_det_class_nms_supported(n, 21) for n in (0, 1, cap, cap + 1)] == [0, 1, 1, 0]
    assert [lib.afan_det_class_nms_supported(300, c) for c in (1, 2, 64, 65)] == [0, 1, 1, 0]
    assert pkg.det_ops.class_nms_supported(300, 21) and not pkg.det_ops.class_nms_supported(cap + 1, 21)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)                              # float-aligned, not 16-byte aligned
    f = lib.afan_det_class_nms
    assert f(p, p, p, p, 1, 0, 21, 9., 9., .3, -1., p, p, p, None) == -3            # AFAN_ESHAPE: N = 0
    assert f(p, p, p, p, 1, cap + 1, 21, 9., 9., .3, -1., p, p, p, None) == -3      # beyond the cap
    assert f(p, p, p, p, 1, 4, 1, 9., 9., .3, -1., p, p, p, None) == -3             # no foreground class
    assert f(p, p, p, p, -1, 4, 21, 9., 9., .3, -1., p, p, p, None) == -3
    assert f(None, None, None, None, 0, 4, 21, 9., 9., .3, -1., None, None, None, None) == 0      # B = 0: no launch
    for k in (0, 1, 2, 3, 11, 12, 13):
        a = [p, p, p, p, 1, 4, 21, 9., 9., .3, -1., p, p, p, None]
        a[k] = None
        assert f(*a) == -4, k                                                        # AFAN_ENULL
    for k in (0, 1, 11):
        a = [p, p, p, p, 1, 4, 21, 9., 9., .3, -1., p, p, p, None]
        a[k] = odd
        assert f(*a) == -2, k                                                        # AFAN_EALIGN
    g = lib.afan_det_pack
    assert g(p, p, p, -1, 4, p, p, None) == -3 and g(p, p, p, 2, 0, p, p, None) == -3
    assert g(None, None, None, 0, 4, None, None, None) == 0
    assert g(p, p, None, 2, 4, p, p, None) == -4 and g(odd, p, p, 2, 4, p, p, None) == -2
