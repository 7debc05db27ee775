"""seg_data.load_cityscapes without a GPU: a tree of two cities written with Pillow, read back sorted with the label ids mapped to
train ids; the table against the ids recorded from the reference (tests/golden/cityscapes_train_ids.json); the refusals."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


def _write(root, split, city, name, img, ids):
    from PIL import Image
    for sub in ("leftImg8bit", "gtFine"):
        os.makedirs(os.path.join(root, sub, split, city), exist_ok=True)
    Image.fromarray(img, "RGB").save(os.path.join(root, "leftImg8bit", split, city, name + "_leftImg8bit.png"))
    Image.fromarray(ids, "L").save(os.path.join(root, "gtFine", split, city, name + "_gtFine_labelIds.png"))


def test_table_is_the_recorded_one(pkg):
    ref = json.load(open(os.path.join(GOLDEN, "cityscapes_train_ids.json")))
    sd = pkg.seg_data
    assert len(ref) == 35 and list(sd.CITYSCAPES_TRAIN_IDS) == ref
    assert sorted(set(ref) - {255}) == list(range(19))
    t = sd._train_id_table()
    assert t.shape == (256,) and t[:35].tolist() == ref and (t[35:] == -1).all()
    ids = np.arange(35, dtype=np.uint8).reshape(5, 7)
    assert sd.encode_cityscapes(ids).dtype == np.uint8 and sd.encode_cityscapes(ids).reshape(-1).tolist() == ref


def test_tree_is_read_sorted_and_mapped(pkg, tmp_path):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(0)
    root = str(tmp_path)
    files = [("zurich", "zurich_000002_000019"), ("aachen", "aachen_000010_000019"), ("zurich", "zurich_000001_000019"),
             ("aachen", "aachen_000003_000019")]
    written = {}
    for k, (city, name) in enumerate(files):
        h, w = 6 + k % 2, 8 - k % 2
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ids = rng.integers(0, 34, (h, w), dtype=np.uint8)
        ids[0, :4] = (0, 7, 33, 34)                                  # a void id, road, bicycle, and the table's last entry
        _write(root, "train", city, name, img, ids)
        written[name] = (img, ids)
    _write(root, "val", "aachen", "aachen_000099_000019", written[files[0][1]][0], written[files[0][1]][1])
    images, labels = pkg.seg_data.load_cityscapes(root, "train")
    order = sorted(n for _, n in files)                             # cities sorted, then files: aachen_03, aachen_10, zurich_01, zurich_02
    assert len(images) == len(labels) == 4
    table = np.array(pkg.seg_data.CITYSCAPES_TRAIN_IDS)
    for name, im, lb in zip(order, images, labels):
        img, ids = written[name]
        assert im.dtype == lb.dtype == np.uint8 and np.array_equal(im, img)
        assert np.array_equal(lb, table[ids]) and lb[0, :4].tolist() == [255, 0, 18, 255]
    assert len(pkg.seg_data.load_cityscapes(root, "val")[0]) == 1


def test_refusals(pkg, tmp_path):
    pytest.importorskip("PIL")
    with pytest.raises(FileNotFoundError, match="no download"):
        pkg.seg_data.load_cityscapes(str(tmp_path), "train")
    ids = np.zeros((6, 8), np.uint8)
    ids[2, 3] = 40
    _write(str(tmp_path), "train", "bonn", "bonn_000000_000019", np.zeros((6, 8, 3), np.uint8), ids)
    with pytest.raises(ValueError, match="40"):
        pkg.seg_data.load_cityscapes(str(tmp_path), "train")
    with pytest.raises(ValueError):
        pkg.seg_data.load_cityscapes(str(tmp_path), "train_extra")
