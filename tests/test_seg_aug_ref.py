"""seg_data._augment_numpy — the plain-numpy restatement of the segmentation batch kernel and the GPU tests' reference — against
Pillow's own output (tests/golden/seg_aug_pillow.npz, recorded by tools/gen_seg_aug_golden.py from Image.resize / expand / crop /
transpose): bit-equal, no tolerance.  Where Pillow is importable the same cases are also checked live.  And the 256 values of
ToTensor's /255 against torch's CPU division."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

SRC, OH, OW, TOP, LEFT, FLIP, OUT_H, OUT_W, KIND = range(9)
TRAIN, CROP_VAL, NATIVE = 0, 1, 2
SOURCES = [(37, 53), (64, 48), (9, 7), (5, 40)]
SCALES = [0.5, 0.61803, 0.73, 1.0, 1.37, 1.5, 1.999]
OUTS = [(33, 33), (32, 32), (24, 40)]


def _expected(g):
    """[(case row, Pillow's uint8 HWC image, Pillow's uint8 HW label)]"""
    out, pi, pl = [], 0, 0
    for r in g["cases"]:
        n = int(r[OUT_H] * r[OUT_W])
        out.append((r, g["out_img"][pi:pi + 3 * n].reshape(r[OUT_H], r[OUT_W], 3), g["out_lbl"][pl:pl + n].reshape(r[OUT_H], r[OUT_W])))
        pi, pl = pi + 3 * n, pl + n
    assert pi == g["out_img"].size and pl == g["out_lbl"].size
    return out


def _to_tensor(u8_hwc):
    """ExtToTensor as the reference's CPU worker runs it."""
    return torch.from_numpy(np.ascontiguousarray(u8_hwc.transpose(2, 0, 1))).float().div(255).numpy()


def _pads(r):
    p1 = (1 + r[OUT_W] - r[OW]) // 2 if r[OW] < r[OUT_W] else 0
    p2 = (1 + r[OUT_H] - (r[OH] + 2 * p1)) // 2 if r[OH] + 2 * p1 < r[OUT_H] else 0
    return int(p1), int(p2)


def test_fixture_covers_what_it_must():
    g = golden("seg_aug_pillow")
    rows = g["cases"]
    train = rows[rows[:, KIND] == TRAIN]
    want = {(s, max(int(h * sc), 1), max(int(w * sc), 1), oh, ow) for s, (h, w) in enumerate(SOURCES) for sc in SCALES for oh, ow in OUTS}
    assert {tuple(int(v) for v in (r[SRC], r[OH], r[OW], r[OUT_H], r[OUT_W])) for r in train} == want
    for s, (h, w) in enumerate(SOURCES):
        assert g[f"img{s}"].shape == (h, w, 3) and g[f"lbl{s}"].shape == (h, w)
    kinds = {(_pads(r)[0] > 0, _pads(r)[1] > 0) for r in train}
    assert kinds == {(True, False), (False, True), (True, True), (False, False)}, "width-only, height-only, both pads, no pad"
    assert set(train[:, FLIP]) == {0, 1}
    mt = np.array([r[OH] + 2 * sum(_pads(r)) - r[OUT_H] for r in train])
    ml = np.array([r[OW] + 2 * sum(_pads(r)) - r[OUT_W] for r in train])
    assert ((train[:, TOP] == 0) & (mt > 0)).any() and ((train[:, TOP] == mt) & (mt > 0)).any()
    assert ((train[:, LEFT] == 0) & (ml > 0)).any() and ((train[:, LEFT] == ml) & (ml > 0)).any()
    assert (rows[:, KIND] == CROP_VAL).any() and (rows[:, KIND] == NATIVE).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "seg_aug_pillow.npz")) < 512 * 1024


def test_augment_numpy_equals_pillow_fixture(pkg):
    g = golden("seg_aug_pillow")
    sd = pkg.seg_data
    for r, img, lbl in _expected(g):
        got_i, got_l = sd._augment_numpy(g[f"img{r[SRC]}"], g[f"lbl{r[SRC]}"], *[int(v) for v in r[OH:KIND]])
        assert got_i.dtype == np.float32 and got_l.dtype == np.int64
        assert np.array_equal(got_l, lbl.astype(np.int64)), f"label differs from Pillow: case {r.tolist()}"
        assert np.array_equal(got_i.view(np.uint32), _to_tensor(img).view(np.uint32)), f"image differs from Pillow: case {r.tolist()}"


def test_validation_parameters(pkg):
    """ExtResize(int) + ExtCenterCrop as the loader derives them, against the values recorded in the fixture."""
    g = golden("seg_aug_pillow")
    sd = pkg.seg_data
    for r in g["cases"]:
        h, w = SOURCES[r[SRC]]
        if r[KIND] == CROP_VAL:
            size = int(r[OUT_H])
            assert sd.val_resize_size(h, w, size) == (r[OH], r[OW]) and min(r[OH], r[OW]) == size
            assert sd.center_crop_origin(int(r[OH]), int(r[OW]), size, size) == (r[TOP], r[LEFT])
        elif r[KIND] == NATIVE:
            assert (r[OH], r[OW], r[OUT_H], r[OUT_W]) == (h, w, h, w)
    assert sd.center_crop_origin(36, 38, 33, 33) == (2, 2)            # 1.5 and 2.5: Python's round, half to even


def test_closed_form_nearest_is_not_pillows(pkg):
    """The trap the kernel avoids: int((x + 0.5) * a) is not the accumulated coordinate."""
    sd = pkg.seg_data
    differs = 0
    for n_in, n_out in ((64, 96), (48, 72), (37, 50), (53, 105)):
        tab = sd._nearest_table(n_in, n_out)
        a = n_in / n_out
        xo, ref = a * 0.5, []
        for _ in range(n_out):
            ref.append(int(xo))
            xo += a
        assert tab.tolist() == ref
        differs += int((tab != ((np.arange(n_out) + 0.5) * a).astype(np.int64)).sum())
    assert differs > 0


def test_augment_numpy_equals_pillow_live(pkg):
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("gen_seg_aug_golden", os.path.join(ROOT, "tools", "gen_seg_aug_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = golden("seg_aug_pillow")
    for r, img, lbl in _expected(g):
        args = [int(v) for v in r[OH:KIND]]
        pi, pl = gen.pillow_augment(g[f"img{r[SRC]}"], g[f"lbl{r[SRC]}"], *args)
        assert np.array_equal(pi, img) and np.array_equal(pl, lbl), f"this Pillow differs from the recorded one: case {r.tolist()}"
        got_i, got_l = pkg.seg_data._augment_numpy(g[f"img{r[SRC]}"], g[f"lbl{r[SRC]}"], *args)
        assert np.array_equal(got_l, pl.astype(np.int64)) and np.array_equal(got_i.view(np.uint32), _to_tensor(pi).view(np.uint32))


def test_div255_is_the_cpu_quotient(pkg):
    """All 256 values of ToTensor's scaling: torch.from_numpy(u8).float().div(255) on the CPU is the correctly rounded quotient, and
    differs from the device product fl(v * fl(1/255)) that afan_batch_crop_flip_u8 reproduces."""
    v = np.arange(256, dtype=np.uint8)
    ref = torch.from_numpy(v).float().div(255).numpy()
    assert np.array_equal(pkg.seg_data.QUOT255.view(np.uint32), ref.view(np.uint32))
    exact = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(ref.view(np.uint32), exact.view(np.uint32))
    prod = np.arange(256, dtype=np.float32) * (np.float32(1.0) / np.float32(255.0))
    assert (prod != ref).sum() > 0
