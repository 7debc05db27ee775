"""afan_seg_batch_aug_u8 on the GPU against seg_data._augment_numpy (itself held to Pillow bit for bit by test_seg_aug_ref.py):
image and label bit-equal on vector (out_w % 4 == 0) and scalar widths, on one tile and on several tiles per sample (the tile is
16 rows x 128 columns), out-of-range parameters give the clamped result, and SegDeviceLoader's structure: every index once per
epoch, one launch per batch, no host synchronisation, the same seed gives the same batches, both validation forms."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

SRC, OH, OW, TOP, LEFT, FLIP, OUT_H, OUT_W, KIND = range(9)


class _Resident:
    def __init__(self, pkg, images, labels, dev):
        img, lab, off, hs, ws = pkg.seg_data.pack_split(images, labels)
        self.t = [torch.from_numpy(a).to(dev) for a in (img, off, lab, hs, ws)]
        self.images, self.labels = images, labels

    def run(self, pkg, rows, out_h, out_w, max_shrink=3.0):
        """rows: int64 [m, 6] (index, oh, ow, top, left, flip) -> (kernel output, numpy reference), both as numpy"""
        p = torch.from_numpy(np.ascontiguousarray(rows.T)).to(self.t[0].device)
        img, off, lab, hs, ws = self.t
        gi, gl = pkg.ops.seg_batch_aug(img, off, lab, hs, ws, p[0], p[1], p[2], p[3], p[4], p[5], out_h, out_w, max_shrink)
        ri, rl = pkg.seg_data._augment_numpy_batch(self.images, self.labels, *rows.T, out_h, out_w, max_shrink)
        assert gi.shape == (len(rows), 3, out_h, out_w) and gi.dtype == torch.float32 and gl.dtype == torch.int64
        return gi.cpu().numpy(), gl.cpu().numpy(), ri, rl


def _bit_equal(gi, gl, ri, rl, what):
    assert np.array_equal(gl, rl), f"{what}: {int((gl != rl).sum())} label pixels differ"
    bad = gi.view(np.uint32) != ri.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} image values differ, max |d| = {np.abs(gi - ri).max():.3e}"


@functools.lru_cache(maxsize=1)
def _fixture_split():
    g = golden("seg_aug_pillow")
    return [g[f"img{s}"] for s in range(4)], [g[f"lbl{s}"] for s in range(4)], g["cases"]


def test_fixture_cases_bit_equal(pkg, gpu):
    """Every case of the Pillow fixture (4 sources x 7 scales x 3 output sizes, both validation forms), one launch per output size:
    33 x 33, 9 x 7 and 37 x 53 take the scalar stores, 32 x 32, 24 x 40, 64 x 48 and 5 x 40 the 16-byte ones."""
    images, labels, cases = _fixture_split()
    res = _Resident(pkg, images, labels, gpu)
    sizes = sorted({(int(r[OUT_H]), int(r[OUT_W])) for r in cases})
    assert {w % 4 == 0 for _, w in sizes} == {True, False}
    before = pkg.ops.CALLS["seg_batch_aug"]
    for out_h, out_w in sizes:
        rows = cases[(cases[:, OUT_H] == out_h) & (cases[:, OUT_W] == out_w)][:, :6]
        _bit_equal(*res.run(pkg, rows, out_h, out_w), f"{out_h}x{out_w}")
    assert pkg.ops.CALLS["seg_batch_aug"] - before == len(sizes)


@pytest.mark.parametrize("out_h, out_w", [(41, 261), (40, 260)])
def test_several_tiles_bit_equal(pkg, gpu, out_h, out_w):
    """More than one workgroup per sample in both directions, sizes that are no multiple of the tile (3 x 3 tiles, the last 9 or 8 rows
    and 5 or 4 columns), every scale regime (0.5: 5 taps, 1.0: identity passes, 1.9: 2-3 taps), padding and interior crops, flips."""
    split = pkg.seg_data.SyntheticSegSplit(3, seed=2, min_side=120, max_side=170)
    res = _Resident(pkg, split.images, split.labels, gpu)
    rng = np.random.default_rng(out_w)
    rows = []
    for k, scale in enumerate((0.5, 0.77, 1.0, 1.9, 1.31, 0.5)):
        s = k % 3
        h, w = split.labels[s].shape
        oh, ow = int(h * scale), int(w * scale)
        _, _, pad, _, _ = pkg.seg_data._clamped(h, w, oh, ow, 0, 0, out_h, out_w)
        rows.append([s, oh, ow, rng.integers(0, oh + 2 * pad - out_h + 1), rng.integers(0, ow + 2 * pad - out_w + 1), k % 2])
    _bit_equal(*res.run(pkg, np.array(rows, np.int64), out_h, out_w), f"{out_h}x{out_w}")


def test_out_of_range_parameters_are_clamped(pkg, gpu):
    images, labels, _ = _fixture_split()
    res = _Resident(pkg, images, labels, gpu)
    big = 1 << 40
    rows = np.array([[-7, 30, 40, 3, 3, 0],            # index below the split -> 0
                     [99, 30, 40, 3, 3, 1],            # ... above -> the last image; flip is "non-zero"
                     [1, 50, 40, -5, -big, 7],         # origin below 0 -> 0
                     [1, 50, 40, big, big, 0],         # ... beyond the padded image -> its last window
                     [0, 0, -3, 0, 0, 0],              # a size below h / max_shrink -> ceil(h / 3), ceil(w / 3)
                     [2, big, 9, 5, 0, 0],             # a size beyond 32768 -> 32768 (9 x 7 source: the reference stays small)
                     [2, 9, big, 0, big, 1]], np.int64)
    gi, gl, ri, rl = res.run(pkg, rows, 33, 33)
    _bit_equal(gi, gl, ri, rl, "clamped")
    sd = pkg.seg_data
    assert np.array_equal(ri[0], sd._augment_numpy(images[0], labels[0], 30, 40, 3, 3, 0, 33, 33)[0])
    assert np.array_equal(ri[1], sd._augment_numpy(images[3], labels[3], 30, 40, 3, 3, 1, 33, 33)[0])
    assert np.array_equal(ri[4], sd._augment_numpy(images[0], labels[0], 13, 18, 0, 0, 0, 33, 33)[0])
    assert np.array_equal(ri[5], sd._augment_numpy(images[2], labels[2], 32768, 9, 5, 0, 0, 33, 33)[0])
    # a stricter bound from the caller clamps earlier: in/out <= 1.5
    gi, gl, ri, rl = res.run(pkg, np.array([[1, 10, 10, 0, 0, 0]], np.int64), 32, 32, max_shrink=1.5)
    _bit_equal(gi, gl, ri, rl, "max_shrink 1.5")
    assert np.array_equal(ri[0], sd._augment_numpy(images[1], labels[1], 43, 32, 0, 0, 0, 32, 32)[0])


def _marked_split(n, seed):
    """Image k is the constant k + 1 everywhere (image and label): a batch names the indices it was made from."""
    rng = np.random.default_rng(seed)
    images, labels = [], []
    for k in range(n):
        h, w = (int(v) for v in rng.integers(20, 61, 2))
        images.append(np.full((h, w, 3), k + 1, np.uint8))
        labels.append(np.full((h, w), k + 1, np.uint8))
    return images, labels


def test_loader_epoch_structure(pkg, gpu):
    sd = pkg.seg_data
    images, labels = _marked_split(11, 4)
    loader = sd.SegDeviceLoader(images, labels, 4, gpu, True, 33, seed=5)
    assert len(loader) == 2
    torch.cuda.synchronize()
    before = pkg.ops.CALLS["seg_batch_aug"]
    torch.cuda.set_sync_debug_mode("error")            # a host synchronisation inside the epoch raises
    try:
        batches = list(loader)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert pkg.ops.CALLS["seg_batch_aug"] - before == len(batches) == 2         # one launch per batch
    seen = []
    for x, y in batches:
        assert x.shape == (4, 3, 33, 33) and y.shape == (4, 33, 33) and x.dtype == torch.float32 and y.dtype == torch.int64
        ids = y.reshape(4, -1).max(dim=1).values
        assert torch.equal((x.reshape(4, -1).max(dim=1).values * 255).round().long(), ids)
        seen += ids.tolist()
    assert len(set(seen)) == 8 and set(seen) <= set(range(1, 12))                # drop_last: 8 of the 11, each once
    p = loader.last_params
    assert sorted(p[0] + 1) == sorted(seen) and set(p[5]) <= {0, 1}
    assert ((p[1] >= (loader.hs[p[0]] * 0.5).astype(np.int64)) & (p[1] <= loader.hs[p[0]] * 2)).all()
    ri, rl = sd._augment_numpy_batch(images, labels, *p, 33, 33, loader.max_shrink)
    got_i = torch.cat([b[0] for b in batches]).cpu().numpy()
    got_l = torch.cat([b[1] for b in batches]).cpu().numpy()
    _bit_equal(got_i, got_l, ri, rl, "loader epoch")
    # the same seed gives the same batches, epoch by epoch; the next epoch is another draw
    again = sd.SegDeviceLoader(images, labels, 4, gpu, True, 33, seed=5)
    for (x, y), (x2, y2) in zip(batches, again):
        assert torch.equal(x, x2) and torch.equal(y, y2)
    second, second2 = list(loader), list(again)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(second, second2))
    assert not all(torch.equal(a[1], b[1]) for a, b in zip(batches, second))
    # data parallel: the ranks slice the same draw
    halves = [list(sd.SegDeviceLoader(images, labels, 4, gpu, True, 33, seed=5, rank=r, world=2)) for r in (0, 1)]
    for b, (x, y) in enumerate(batches):
        assert torch.equal(torch.cat([halves[0][b][1], halves[1][b][1]]), y)
        assert torch.equal(torch.cat([halves[0][b][0], halves[1][b][0]]), x)


def test_loader_validation_forms(pkg, gpu):
    sd = pkg.seg_data
    images, labels, _ = _fixture_split()
    images, labels = images[:2], labels[:2]                 # 37 x 53 and 64 x 48
    native = sd.SegDeviceLoader(images, labels, 4, gpu, False, 33)
    out = list(native)
    assert len(native) == len(out) == 2                     # one image per batch at its own size, whatever the batch size asked for
    for (x, y), im, lb in zip(out, images, labels):
        assert x.shape == (1, 3) + lb.shape and y.shape == (1,) + lb.shape
        assert np.array_equal(y[0].cpu().numpy(), lb.astype(np.int64))
        assert np.array_equal(x[0].cpu().numpy(), torch.from_numpy(im.transpose(2, 0, 1).copy()).float().div(255).numpy())
    crop = sd.SegDeviceLoader(images, labels, 2, gpu, False, 32, crop_val=True)
    (x, y), = list(crop)
    assert x.shape == (2, 3, 32, 32)
    for k in range(2):
        h, w = labels[k].shape
        oh, ow = sd.val_resize_size(h, w, 32)
        top, left = sd.center_crop_origin(oh, ow, 32, 32)
        ri, rl = sd._augment_numpy(images[k], labels[k], oh, ow, top, left, 0, 32, 32)
        _bit_equal(x[k].cpu().numpy(), y[k].cpu().numpy(), ri, rl, f"crop_val {k}")
    with pytest.raises(ValueError, match="KMAX"):
        sd.SegDeviceLoader(images, labels, 2, gpu, False, 8, crop_val=True)        # 37 -> 8 is a reduction by more than 3
