"""seg_data._jitter_numpy — the plain-numpy restatement of ExtColorJitter(brightness, contrast, saturation) and the GPU tests'
reference — against Pillow's own ImageEnhance output (tests/golden/seg_jitter_pillow.npz, recorded by tools/gen_seg_jitter_golden.py):
bit-equal, no tolerance.  Where Pillow is importable the same cases, and 300 seeded random ones, are also checked live."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, golden


def _cases(g):
    """[(name, source, order, factor triple, Pillow's uint8 HWC output)]"""
    names, out, p = [str(n) for n in g["names"]], [], 0
    for s, o, f in g["cases"]:
        src = g[f"img_{names[s]}"]
        out.append((names[s], src, int(o), tuple(float(v) for v in g["factors"][f]), g["out_img"][p:p + src.size].reshape(src.shape)))
        p += src.size
    assert p == g["out_img"].size
    return out


def _gen():
    spec = importlib.util.spec_from_file_location("gen_seg_jitter_golden", os.path.join(ROOT, "tools", "gen_seg_jitter_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_covers_what_it_must(pkg):
    g = golden("seg_jitter_pillow")
    cases = _cases(g)
    assert {c[2] for c in cases} == set(range(6))                                          # all six orders
    flat = {v for c in cases for v in c[3]}
    assert {0.5, 1.0, 1.5} <= flat and any(0.5 < v < 1.0 for v in flat) and any(1.0 < v < 1.5 for v in flat)
    by = {c[0]: c[1] for c in cases}
    assert (by["const"] == by["const"][0, 0]).all() and by["pixel"].shape == (1, 1, 3)
    for ch in range(3):
        assert (by["extremes"][..., ch] == 0).any() and (by["extremes"][..., ch] == 255).any()
    for name in ("half_even", "half_odd"):                                                 # a gray mean of exactly k + 0.5
        gr = pkg.seg_data._gray(by[name]).reshape(-1)
        assert gr.size == 2 and gr[1] == gr[0] + 1
        assert {c[2] for c in cases if c[0] == name} == set(range(6))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "seg_jitter_pillow.npz")) < 256 * 1024
    assert pkg.seg_data.JITTER_ORDERS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def test_jitter_numpy_equals_pillow_fixture(pkg):
    for name, src, order, fac, want in _cases(golden("seg_jitter_pillow")):
        got = pkg.seg_data._jitter_numpy(src, order, fac)
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"differs from Pillow: {name}, order {order}, factors {fac}"


def test_order_code_is_clamped(pkg):
    sd = pkg.seg_data
    src = golden("seg_jitter_pillow")["img_rand0"]
    fac = (0.73, 1.21, 0.88)
    assert np.array_equal(sd._jitter_numpy(src, -3, fac), sd._jitter_numpy(src, 0, fac))
    assert np.array_equal(sd._jitter_numpy(src, 9, fac), sd._jitter_numpy(src, 5, fac))
    assert not np.array_equal(sd._jitter_numpy(src, 0, fac), sd._jitter_numpy(src, 5, fac))


def test_jitter_numpy_equals_pillow_live(pkg):
    pytest.importorskip("PIL")
    gen = _gen()
    for name, src, order, fac, want in _cases(golden("seg_jitter_pillow")):
        assert np.array_equal(gen.pillow_jitter(src, order, fac), want), f"this Pillow differs from the recorded one: {name} {order} {fac}"
    rng = np.random.default_rng(5)
    for k in range(300):
        h, w = (int(v) for v in rng.integers(1, 12, 2))
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if k % 7 else np.full((h, w, 3), rng.integers(0, 256, 3), np.uint8)
        fac = tuple(float(np.float32(v)) for v in rng.uniform(0.5, 1.5, 3))
        if k % 5 == 0:
            fac = (1.0,) + fac[1:]
        order = int(rng.integers(0, 6))
        assert np.array_equal(pkg.seg_data._jitter_numpy(src, order, fac), gen.pillow_jitter(src, order, fac)), (k, order, fac)


def test_unit_factors_are_the_plain_augmentation(pkg):
    """All factors 1.0: every blend returns the pixel, so _augment_jitter_numpy is _augment_numpy (padding, resize and flip included)."""
    sd = pkg.seg_data
    g = golden("seg_aug_pillow")
    for s, (oh, ow, top, left, flip, out_h, out_w) in enumerate([(37, 53, 2, 9, 1, 33, 33), (40, 30, 0, 0, 0, 32, 32), (9, 7, 5, 1, 1, 24, 40)]):
        img, lbl = g[f"img{s}"], g[f"lbl{s}"]
        a = sd._augment_numpy(img, lbl, oh, ow, top, left, flip, out_h, out_w)
        for order in range(6):
            b = sd._augment_jitter_numpy(img, lbl, oh, ow, top, left, flip, order, (1.0, 1.0, 1.0), out_h, out_w)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
        c = sd._augment_jitter_numpy(img, lbl, oh, ow, top, left, flip, 3, (0.6, 1.4, 0.7), out_h, out_w)
        assert np.array_equal(a[1], c[1]) and not np.array_equal(a[0], c[0])               # the label is never jittered
