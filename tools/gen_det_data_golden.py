"""Records tests/golden/det_data_pillow.npz: what Pillow's own ImageOps.mirror / Image.resize and torch's own fp32 box arithmetic give
for the Detection transforms (Detection/dataset/voc2007.py:95-116, dataset/base.py:75-91) on seeded random uint8 images.  Only arrays
are stored: the sources, their boxes, one parameter row per case, Pillow's uint8 outputs (`stored_output` below undoes the column
order a mirrored case is stored in) and torch's fp32 boxes.
tests/test_det_data_ref.py holds det_data._det_batch_numpy to them bit for bit (and to Pillow live, where it is installed, through
`pillow_resize` below).

    python tools/gen_det_data_golden.py            # needs Pillow and torch
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [(37, 53), (64, 48), (9, 7), (5, 40), (50, 33)]            # (h, w)
SIDES = [(60., 100.), (24., 40.), (20., 100.), (48., 56.), (30., 30.)]   # (min_side, max_side)
# columns of a case row (the fp32 scale sits in `scales`)
SRC, OH, OW, FLIP, SIDE = range(5)


def pillow_resize(img, oh, ow, flip):
    """ImageOps.mirror (where flip) -> Image.resize((ow, oh), BILINEAR): what transforms.Resize((oh, ow)) does to a PIL image."""
    from PIL import Image, ImageOps
    im = Image.fromarray(img, "RGB")
    if flip:
        im = ImageOps.mirror(im)
    return np.asarray(im.resize((ow, oh), Image.BILINEAR), dtype=np.uint8)


def stored_output(flat, oh, ow, flip):
    """Pillow's output of a case from its bytes in `out_img`."""
    a = flat.reshape(oh, ow, 3)
    return a[:, ::-1] if flip else a


def torch_boxes(boxes, width, flip, scale):
    """voc2007.py:102-114 on the boxes: the flip with the int image width, then `bboxes *= scale` with a float32 scalar tensor."""
    import torch
    bboxes = torch.tensor(boxes.tolist(), dtype=torch.float)
    if flip:
        bboxes[:, [0, 2]] = int(width) - bboxes[:, [2, 0]]
    bboxes *= torch.tensor(float(scale), dtype=torch.float)
    return bboxes.numpy()


def main():
    sys.path.insert(0, ROOT)
    dd = importlib.import_module("cv_a-fan_amd.det_data")
    rng = np.random.default_rng(17)
    store = {}
    for s, (h, w) in enumerate(SOURCES):
        store[f"img{s}"] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        g = 1 + s % 3
        x0, y0 = rng.integers(0, w - 2, g), rng.integers(0, h - 2, g)
        x1, y1 = x0 + 1 + rng.integers(0, w - 1 - x0), y0 + 1 + rng.integers(0, h - 1 - y0)
        store[f"box{s}"] = np.stack([x0, y0, x1, y1], axis=1).astype(np.float32)
    rows, scales, imgs, boxes = [], [], [], []
    for s, (h, w) in enumerate(SOURCES):
        for k, (lo, hi) in enumerate(SIDES):
            oh, ow, scale = dd.preprocess_size(h, w, lo, hi)
            for flip in (0, 1):
                rows.append([s, oh, ow, flip, k])
                scales.append(scale)
                a = pillow_resize(store[f"img{s}"], oh, ow, flip)
                assert a.shape == (oh, ow, 3)
                # a mirrored case is stored with its columns reversed AGAIN: next to the unmirrored case it then differs in the few
                # pixels where Pillow's coefficients are not mirror-symmetric, and the archive compresses to about half
                imgs.append((a[:, ::-1] if flip else a).reshape(-1))
                boxes.append(torch_boxes(store[f"box{s}"], w, flip, scale).reshape(-1))
    import PIL
    store.update(cases=np.array(rows, np.int64), scales=np.array(scales, np.float64), sides=np.array(SIDES, np.float64),
                 out_img=np.concatenate(imgs), out_box=np.concatenate(boxes).astype(np.float32),
                 pillow_version=np.array([int(v) for v in PIL.__version__.split(".")[:3]], np.int64))
    path = os.path.join(ROOT, "tests", "golden", "det_data_pillow.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes,", len(rows), "cases")


if __name__ == "__main__":
    main()
