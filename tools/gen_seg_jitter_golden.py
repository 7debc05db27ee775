"""Records tests/golden/seg_jitter_pillow.npz: what Pillow's own ImageEnhance.Brightness / Contrast / Color give, chained in each of
the six orders, for the reference's ExtColorJitter(brightness=0.5, contrast=0.5, saturation=0.5) (Segmentation/args.py:146).  That is
what torchvision's PIL functional calls (adjust_brightness / adjust_contrast / adjust_saturation); torchvision itself is not needed.
Only arrays are stored: the sources, one row per case and Pillow's uint8 outputs.  tests/test_seg_jitter_ref.py holds
seg_data._jitter_numpy to them bit for bit (and to Pillow live, where it is installed, through `pillow_jitter` below).

    python tools/gen_seg_jitter_golden.py            # needs Pillow
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the order code: the permutations of (brightness, contrast, saturation) in lexicographic order (seg_data.JITTER_ORDERS)
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
# factor triples (brightness, contrast, saturation): the ends, exactly 1, and interior draws on both sides of 1
FACTORS = [(0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (1.5, 1.5, 1.5), (0.5, 1.5, 1.0), (1.5, 1.0, 0.5), (1.0, 0.5, 1.5),
           (0.73, 1.21, 0.88), (1.37, 0.61803, 1.4999), (0.9999, 1.0001, 1.25)]


def pillow_jitter(img, order, factors):
    """ImageEnhance chained in ORDERS[order] on an HWC uint8 array; factors by operation (brightness, contrast, saturation)."""
    from PIL import Image, ImageEnhance
    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    for op in ORDERS[order]:
        im = enh[op](im).enhance(float(factors[op]))
    return np.asarray(im, dtype=np.uint8)


def sources():
    """name -> HWC uint8: seeded random images, a constant one, a single pixel, one holding 0 and 255 in every channel, and two
    pixels whose gray values are k and k + 1 (a gray mean of exactly k + 0.5: the rounding of contrast's mean)."""
    rng = np.random.default_rng(23)
    src = {"rand0": rng.integers(0, 256, (13, 17, 3), dtype=np.uint8), "rand1": rng.integers(0, 256, (8, 5, 3), dtype=np.uint8),
           "dark": rng.integers(0, 40, (6, 7, 3), dtype=np.uint8), "bright": rng.integers(215, 256, (6, 7, 3), dtype=np.uint8),
           "const": np.full((5, 6, 3), (37, 140, 201), np.uint8), "pixel": np.array([[[200, 17, 99]]], np.uint8)}
    ext = rng.integers(0, 256, (4, 6, 3), dtype=np.uint8)
    ext[0, 0], ext[0, 1], ext[1, 0], ext[1, 1] = (0, 0, 0), (255, 255, 255), (0, 255, 0), (255, 0, 255)
    src["extremes"] = ext
    src["half_even"] = np.array([[[100, 100, 100], [101, 101, 101]]], np.uint8)      # gray 100 and 101: mean 100.5
    src["half_odd"] = np.array([[[77, 77, 77]], [[78, 78, 78]]], np.uint8)           # gray 77 and 78: mean 77.5
    return src


def cases(names):
    """[source, order, factor triple] rows: every source in every order, the factor triples cycling so that every triple meets every
    order; the small sources additionally with every triple in every order."""
    rows, c = [], 0
    for s, name in enumerate(names):
        every = name in ("pixel", "half_even", "half_odd", "const", "extremes")
        for o in range(6):
            for f in (range(len(FACTORS)) if every else [(c + k) % len(FACTORS) for k in range(3)]):
                rows.append([s, o, f])
            c += 1
    return np.array(rows, np.int64)


def main():
    src = sources()
    names = sorted(src)
    rows = cases(names)
    outs = [pillow_jitter(src[names[s]], o, FACTORS[f]).reshape(-1) for s, o, f in rows]
    import PIL
    store = {f"img_{n}": src[n] for n in names}
    store.update(names=np.array(names), cases=rows, factors=np.array(FACTORS, np.float64), out_img=np.concatenate(outs),
                 pillow_version=np.array([int(v) for v in PIL.__version__.split(".")[:3]], np.int64))
    path = os.path.join(ROOT, "tests", "golden", "seg_jitter_pillow.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes,", len(rows), "cases")


if __name__ == "__main__":
    sys.exit(main())
