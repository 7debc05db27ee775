"""train_aug_sat_muti_advt.py without a GPU: its parser against the names and defaults recorded from the reference's own parser
(tests/golden/det_args.json), the configuration the flags fold into, the experiment string and the checkpoint directory, the refused
backbones and datasets by their sentence, the loud failure on a host, and load_voc_det naming what is missing."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.train_aug_sat_muti_advt")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


BASE = ["-s", "voc2007", "-b", "resnet101"]


def test_parser_equals_the_references(entry, pkg):
    ref = json.load(open(os.path.join(GOLDEN, "det_args.json")))
    assert len(ref) == 32
    assert _table(entry.get_argparser()) == ref                   # same options, same order, same defaults
    full = _table(entry.get_full_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == entry.ADDITIONS == ("synthetic", "dtype", "layout", "seed")
    o = entry.get_full_argparser().parse_args(BASE)
    assert (o.synthetic, o.dtype, o.layout, o.seed) == (0, "bf16", "nhwc", None)
    with pytest.raises(SystemExit):
        entry.get_full_argparser().parse_args(["-b", "resnet101"])            # -s is required
    cfg = pkg.det_entry.config(o)                                              # config.py and train_config.py, folded in
    assert (cfg["image_min_side"], cfg["image_max_side"], cfg["rpn_pre_nms_top_n"], cfg["rpn_post_nms_top_n"]) == (600.0, 1000.0, 12000, 2000)
    assert (cfg["batch_size"], cfg["learning_rate"], cfg["momentum"], cfg["weight_decay"]) == (1, 0.001, 0.9, 0.0005)
    assert (cfg["step_lr_sizes"], cfg["step_lr_gamma"], cfg["warm_up_factor"], cfg["warm_up_num_iters"]) == ([50000, 70000], 0.1, 0.3333, 500)
    assert (cfg["num_steps_to_display"], cfg["num_steps_to_snapshot"], cfg["num_steps_to_finish"]) == (20, 10000, 90000)
    assert cfg["anchor_sizes"] == [128, 256, 512] and cfg["pooler_mode"] == "align"
    o = entry.get_full_argparser().parse_args(BASE + ["--step_lr_sizes", "[10, 20]", "--anchor_sizes", "[64]", "--batch_size", "2",
                                                      "--image_min_side", "128"])
    cfg = pkg.det_entry.config(o)
    assert cfg["step_lr_sizes"] == [10, 20] and cfg["anchor_sizes"] == [64] and cfg["batch_size"] == 2 and cfg["image_min_side"] == 128.0


def test_exp_string_and_checkpoint_directory(entry):
    o = entry.get_full_argparser().parse_args(BASE)
    assert entry.exp_name(o) == "s1p3g0.5e2"
    assert entry.checkpoints_dir(o) == os.path.join("./outputs", "ckpt-s1p3g0.5e2-voc2007-resnet101")
    o = entry.get_full_argparser().parse_args(["-s", "voc20072012", "-b", "resnet101", "--steps", "3", "--gamma", "0.25", "--eps", "4.0",
                                               "--randinit", "--clip", "-o", "/tmp/x"])
    assert entry.exp_name(o) == "s3p3g0.25e4.0_rand_clip"
    assert entry.checkpoints_dir(o) == "/tmp/x/ckpt-s3p3g0.25e4.0_rand_clip-voc20072012-resnet101"


def test_scheduler_state_and_checkpoint_keys(pkg):
    o = importlib.import_module("cv_a-fan_amd.det_entry")
    cfg = dict(o.DEFAULTS)
    st = o.scheduler_state(7, cfg)
    assert st == {"last_epoch": 7, "base_lr": 0.001, "milestones": [50000, 70000], "gamma": 0.1, "factor": 0.3333, "num_iters": 500}
    assert o.lr_at(0, cfg) == o.warmup_multistep_lr(0, 0.001, [50000, 70000], 0.1, 0.3333, 500)


@pytest.mark.parametrize("name, word", [("resnet18", "BasicBlock"), ("resnet50", "ResNet-101 is pinned")])
def test_refused_backbones(entry, name, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match=word):
        entry.main(["-s", "voc2007", "-b", name, "--loss_settings", "1"])
    assert not os.path.exists(tmp_path / "outputs")


@pytest.mark.parametrize("name, word", [("coco2017", "pycocotools"), ("coco2017-person", "pycocotools"), ("coco2017-car", "pycocotools"),
                                        ("coco2017-animal", "pycocotools"), ("voc2007-cat-dog", "cat / dog subset")])
def test_refused_datasets(entry, name, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match=word):
        entry.main(["-s", name, "-b", "resnet101", "--loss_settings", "1"])
    assert not os.path.exists(tmp_path / "outputs")


def test_loss_settings_outside_the_iteration_are_refused(entry, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="settings 1 to 4"):
        entry.main(BASE)                                                       # the reference's default of 0 asserts in its first step


def test_entry_fails_loudly_without_a_gpu(entry, monkeypatch, tmp_path):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        entry.main(BASE + ["--loss_settings", "1", "--synthetic", "4"])
    assert not os.path.exists(tmp_path / "outputs")


def test_load_voc_det_names_what_is_missing(pkg, tmp_path):
    pytest.importorskip("PIL")
    dd = pkg.det_data
    with pytest.raises(FileNotFoundError, match="trainval.txt") as e:
        dd.load_voc_det(str(tmp_path), "voc2007", True)
    assert "no download" in str(e.value) and os.path.join("VOCdevkit", "VOC2007") in str(e.value)
    with pytest.raises(FileNotFoundError, match="test.txt"):
        dd.load_voc_det(str(tmp_path), "voc20072012", False)
    main = tmp_path / "VOCdevkit" / "VOC2007" / "ImageSets" / "Main"
    os.makedirs(main)
    (main / "trainval.txt").write_text("000005\n")
    with pytest.raises(FileNotFoundError, match="Annotations"):
        dd.load_voc_det(str(tmp_path), "voc2007", True)
    with pytest.raises(ValueError, match="voc2007 and voc20072012"):
        dd.load_voc_det(str(tmp_path), "coco2017", True)


def test_load_voc_det_reads_a_tiny_tree(pkg, tmp_path, capsys):
    """One annotated image, one whose only object is difficult: the `- 1`, the category table, the dropped image and its count."""
    Image = pytest.importorskip("PIL.Image")
    import numpy as np
    voc = tmp_path / "VOCdevkit" / "VOC2007"
    for d in ("ImageSets/Main", "Annotations", "JPEGImages"):
        os.makedirs(voc / d)
    (voc / "ImageSets/Main/trainval.txt").write_text("000001\n000002\n")
    obj = "<object><name>{}</name><difficult>{}</difficult><bndbox><xmin>{}</xmin><ymin>{}</ymin><xmax>{}</xmax><ymax>{}</ymax></bndbox></object>"
    xml = "<annotation><filename>{}.jpg</filename><size><width>12</width><height>10</height></size>{}</annotation>"
    (voc / "Annotations/000001.xml").write_text(xml.format("000001", obj.format("dog", 0, 2, 3, 9, 8) + obj.format("cat", 1, 1, 1, 5, 5)
                                                           + obj.format("tvmonitor", 0, 1, 1, 12, 10)))
    (voc / "Annotations/000002.xml").write_text(xml.format("000002", obj.format("person", 1, 1, 1, 5, 5)))
    for n in ("000001", "000002"):
        Image.fromarray(np.full((10, 12, 3), 90, np.uint8)).save(voc / f"JPEGImages/{n}.jpg")
    images, boxes, classes = pkg.det_data.load_voc_det(str(tmp_path), "voc2007", True)
    assert len(images) == 1 and images[0].shape == (10, 12, 3) and images[0].dtype == np.uint8
    assert boxes[0].tolist() == [[1., 2., 8., 7.], [0., 0., 11., 9.]] and classes[0].tolist() == [12, 20]
    assert "Dropped 1 images" in capsys.readouterr().out
