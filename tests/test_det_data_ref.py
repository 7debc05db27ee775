"""det_data._det_batch_numpy — the plain-numpy restatement of the detection batch kernel and the GPU tests' reference — against
Pillow's and torch's own output (tests/golden/det_data_pillow.npz, recorded by tools/gen_det_data_golden.py from ImageOps.mirror /
Image.resize and the fp32 box arithmetic of Detection/dataset/voc2007.py:102-114): bit-equal, no tolerance, no case left out.  Where
Pillow is importable the same cases are also checked live.  And the host-side rules: preprocess_size, ratio_batches and the closed
form of the learning-rate schedule against values worked out by hand."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

SRC, OH, OW, FLIP, SIDE = range(5)
SOURCES = [(37, 53), (64, 48), (9, 7), (5, 40), (50, 33)]
SIDES = [(60., 100.), (24., 40.), (20., 100.), (48., 56.), (30., 30.)]


def _expected(g):
    """[(case row, scale, Pillow's uint8 HWC image, torch's fp32 boxes)]: a mirrored case is stored with its columns reversed again
    (tools/gen_det_data_golden.py)."""
    out, pi, pb = [], 0, 0
    for r, sc in zip(g["cases"], g["scales"]):
        n, nb = int(r[OH] * r[OW]) * 3, g[f"box{r[SRC]}"].size
        img = g["out_img"][pi:pi + n].reshape(r[OH], r[OW], 3)
        out.append((r, sc, img[:, ::-1] if r[FLIP] else img, g["out_box"][pb:pb + nb].reshape(-1, 4)))
        pi, pb = pi + n, pb + nb
    assert pi == g["out_img"].size and pb == g["out_box"].size
    return out


def _to_tensor(u8_hwc):
    return torch.from_numpy(np.ascontiguousarray(u8_hwc.transpose(2, 0, 1))).float().div(255).numpy()


def test_fixture_covers_what_it_must(pkg):
    g = golden("det_data_pillow")
    rows = g["cases"]
    assert len(rows) == 50 and np.array_equal(g["sides"], np.array(SIDES))
    want = set()
    for s, (h, w) in enumerate(SOURCES):
        assert g[f"img{s}"].shape == (h, w, 3) and g[f"box{s}"].dtype == np.float32 and g[f"box{s}"].shape[1] == 4
        for k, (lo, hi) in enumerate(SIDES):
            oh, ow, _ = pkg.det_data.preprocess_size(h, w, lo, hi)
            want |= {(s, oh, ow, 0, k), (s, oh, ow, 1, k)}
    assert {tuple(int(v) for v in r) for r in rows} == want                  # 5 sources x 5 side pairs, each flipped and not
    ratio = np.array([[r[OH] / SOURCES[r[SRC]][0], r[OW] / SOURCES[r[SRC]][1]] for r in rows])
    assert ratio.max() >= 4 and ratio.min() < 0.7 and (ratio == 1.0).any()  # up-scaling, reductions, identity passes
    assert any(max(r[OH], r[OW]) == int(SIDES[r[SIDE]][1]) and min(r[OH], r[OW]) < int(SIDES[r[SIDE]][0]) for r in rows)   # the cap
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "det_data_pillow.npz")) < 186 * 1024


def test_det_batch_numpy_equals_the_fixture(pkg):
    g = golden("det_data_pillow")
    dd = pkg.det_data
    images = [g[f"img{s}"] for s in range(5)]
    boxes = [g[f"box{s}"] for s in range(5)]
    classes = [np.arange(1, len(b) + 1, dtype=np.int64) for b in boxes]
    for r, sc, img, box in _expected(g):
        s, oh, ow, fl = (int(v) for v in r[:4])
        gi, gb, gl = dd._det_batch_numpy(images, boxes, classes, [s], [oh], [ow], [fl], [np.float32(sc)], oh, ow, len(box))
        assert gi.dtype == np.float32 and gb.dtype == np.float32 and gl.dtype == np.int64
        assert np.array_equal(gi[0].view(np.uint32), _to_tensor(img).view(np.uint32)), f"image differs from Pillow: case {r.tolist()}"
        assert np.array_equal(gb[0].view(np.uint32), box.view(np.uint32)), f"boxes differ from torch: case {r.tolist()}"
        assert np.array_equal(gl[0], classes[s])


def test_det_batch_numpy_pads_right_and_below_and_truncates(pkg):
    g = golden("det_data_pillow")
    dd = pkg.det_data
    img, box = g["img0"], g["box1"]
    cls = np.array([3, 7], np.int64)
    assert len(box) == 2
    a, b, l = dd._det_sample_numpy(img, box, cls, 40, 50, 1, np.float32(1.5), 44, 57, 4)
    ref, rb, _ = dd._det_sample_numpy(img, box, cls, 40, 50, 1, np.float32(1.5), 40, 50, 2)
    assert a.shape == (3, 44, 57) and np.array_equal(a[:, :40, :50], ref) and not a[:, 40:].any() and not a[:, :, 50:].any()
    assert np.array_equal(b[:2], rb) and not b[2:].any() and l.tolist() == [3, 7, 0, 0]
    a, b, l = dd._det_sample_numpy(img, box, cls, 40, 50, 0, np.float32(1.5), 33, 20, 1)        # a window at the origin, one box kept
    ref0 = dd._det_sample_numpy(img, box, cls, 40, 50, 0, np.float32(1.5), 40, 50, 2)
    assert np.array_equal(a, ref0[0][:, :33, :20]) and np.array_equal(b, ref0[1][:1]) and l.tolist() == [3]


def test_det_batch_numpy_equals_pillow_live(pkg):
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("gen_det_data_golden", os.path.join(ROOT, "tools", "gen_det_data_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = golden("det_data_pillow")
    for r, sc, img, box in _expected(g):
        s, oh, ow, fl = (int(v) for v in r[:4])
        live = gen.pillow_resize(g[f"img{s}"], oh, ow, fl)
        assert np.array_equal(live, img), f"this Pillow differs from the recorded one: case {r.tolist()}"
        assert np.array_equal(gen.torch_boxes(g[f"box{s}"], SOURCES[s][1], fl, sc).view(np.uint32), box.view(np.uint32))
        got = pkg.det_data._det_sample_numpy(g[f"img{s}"], g[f"box{s}"], np.zeros(len(box), np.int64), oh, ow, fl, np.float32(sc), oh, ow,
                                             len(box))
        assert np.array_equal(got[0].view(np.uint32), _to_tensor(live).view(np.uint32))


def test_preprocess_size_by_hand(pkg):
    f = pkg.det_data.preprocess_size
    assert f(375, 500, 600., 1000.) == (600, 800, 1.6)                       # the shorter side to 600
    assert f(500, 375, 600., 1000.) == (800, 600, 1.6)
    oh, ow, s = f(200, 500, 600., 1000.)                                     # 3.0 would give 1500: capped, 3 * (1000 / 1500)
    assert (oh, ow) == (400, 1000) and s == 3.0 * (1000. / 1500.)
    assert f(3, 2, 3., 100.) == (4, 3, 1.5)                                  # 4.5: Python's round, half to even
    assert f(5, 2, 3., 100.) == (8, 3, 1.5)                                  # 7.5 -> 8
    assert f(40, 5, 24., 40.) == (40, 5, 4.8 * (40. / 192.))                 # 4.8 would give 192: capped back to the size it has


def test_ratio_batches(pkg):
    dd = pkg.det_data
    rng0 = np.random.default_rng([3, 0])
    ratios = np.where(np.arange(23) % 3 == 0, 0.75, 1.0 + np.arange(23) / 50)          # 8 tall (0, 3, .., 21), 15 fat; 1.0 counts as fat
    tall = set(np.nonzero(ratios < 1)[0].tolist())
    b = dd.ratio_batches(ratios, 4, rng0)
    assert b.shape == (2 + 3, 4) and b.dtype == np.int64                     # 8 // 4 tall groups, 15 // 4 fat ones: 3 fat indices dropped
    kinds = [set(row.tolist()) <= tall for row in b]
    assert all(set(row.tolist()) <= tall or not (set(row.tolist()) & tall) for row in b) and sum(kinds) == 2
    flat = b.reshape(-1).tolist()
    assert len(set(flat)) == len(flat) == 20 and tall <= set(flat)
    assert np.array_equal(b, dd.ratio_batches(ratios, 4, np.random.default_rng([3, 0])))       # the same seed: the same batches
    assert not np.array_equal(b, dd.ratio_batches(ratios, 4, np.random.default_rng([3, 1])))
    assert dd.ratio_batches(ratios[:3], 4, np.random.default_rng(0)).shape == (0, 4)           # fewer than a batch of either kind
    one = dd.ratio_batches(ratios, 1, np.random.default_rng(0))
    assert sorted(one.reshape(-1).tolist()) == list(range(23))               # batch 1 drops nothing


def test_warmup_multistep_lr_by_hand(pkg):
    f = lambda t: pkg.det_entry.warmup_multistep_lr(t, 0.001, [50000, 70000], 0.1, 0.3333, 500)
    want = {0: 0.001 * 0.3333,                                               # the first iteration: base * factor
            250: 0.001 * (0.3333 + 0.6667 * 0.5),
            499: 0.001 * (0.3333 + 0.6667 * 0.998),
            500: 0.001,                                                      # the warm-up is over
            49999: 0.001,
            50000: 0.001 * 0.1,                                              # bisect_right: the milestone itself has stepped
            70000: 0.001 * 0.1 * 0.1}
    for t, v in want.items():
        assert f(t) == pytest.approx(v, rel=1e-12), t
    assert f(0) == pytest.approx(3.333e-4, rel=1e-12) and f(250) == pytest.approx(6.6665e-4, rel=1e-12)
    assert f(499) == pytest.approx(9.986666e-4, rel=1e-12) and f(70000) == pytest.approx(1e-5, rel=1e-12)
