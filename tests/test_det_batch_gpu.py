"""afan_det_batch_resize_u8 on the GPU against det_data._det_batch_numpy (itself held to Pillow and torch bit for bit by
test_det_data_ref.py): image (uint32 views), boxes (fp32 bits) and labels equal on vector (out_w % 4 == 0) and scalar widths, on one
tile and on several tiles per sample (the tile is 16 rows x 128 columns), padding exactly 0, out-of-range parameters give the clamped
result, a bad table entry gives a zero sample, and DetDeviceLoader's structure: one launch per batch, no host synchronisation, the
same seed gives the same epoch, rank slices partition the batch, evaluation mode in order and unflipped."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

SRC, OH, OW, FLIP, SIDE = range(5)


class _Resident:
    def __init__(self, pkg, images, boxes, classes, dev):
        self.packed = pkg.det_data.pack_det_split(images, boxes, classes)
        self.t = [torch.from_numpy(a).to(dev) for a in self.packed]
        self.images, self.boxes, self.classes = images, boxes, classes

    def run(self, pkg, rows, scale, out_h, out_w, g_max, max_shrink=3.0):
        """rows: int64 [m, 4] (index, oh, ow, flip), scale: fp32 [m] -> (kernel outputs, numpy references), all numpy"""
        dev = self.t[0].device
        p = torch.from_numpy(np.ascontiguousarray(rows.T)).to(dev)
        s = torch.from_numpy(np.asarray(scale, np.float32)).to(dev)
        got = pkg.ops.det_batch_resize(*self.t, p[0], p[1], p[2], p[3], s, out_h, out_w, g_max, max_shrink)
        ref = pkg.det_data._det_batch_numpy(self.images, self.boxes, self.classes, *rows.T, np.asarray(scale, np.float32), out_h, out_w,
                                            g_max, max_shrink)
        assert got[0].shape == (len(rows), 3, out_h, out_w) and got[1].shape == (len(rows), g_max, 4) and got[2].shape == (len(rows), g_max)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
        return tuple(t.cpu().numpy() for t in got), ref


def _bit_equal(got, ref, what):
    bad = got[0].view(np.uint32) != ref[0].view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} image values differ, max |d| = {np.abs(got[0] - ref[0]).max():.3e}"
    bad = got[1].view(np.uint32) != ref[1].view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} box coordinates differ"
    assert np.array_equal(got[2], ref[2]), f"{what}: labels differ"


@functools.lru_cache(maxsize=1)
def _fixture_split():
    g = golden("det_data_pillow")
    boxes = [g[f"box{s}"] for s in range(5)]
    return [g[f"img{s}"] for s in range(5)], boxes, [np.arange(3, 3 + len(b), dtype=np.int64) for b in boxes], g["cases"], g["scales"]


@functools.lru_cache(maxsize=1)
def _big_split(pkg):
    return pkg.det_data.SyntheticDetSplit(4, seed=2, min_side=120, max_side=170)


def test_fixture_cases_bit_equal(pkg, gpu):
    """Every case of the Pillow fixture (5 sources x 5 side pairs, flipped and not), one launch per output size with the mirrored and the
    unmirrored sample of the SAME source in it: both store paths occur."""
    images, boxes, classes, cases, scales = _fixture_split()
    res = _Resident(pkg, images, boxes, classes, gpu)
    sizes = sorted({(int(r[OH]), int(r[OW])) for r in cases})
    assert {w % 4 == 0 for _, w in sizes} == {True, False}
    before = pkg.ops.CALLS["det_batch_resize"]
    for out_h, out_w in sizes:
        sel = (cases[:, OH] == out_h) & (cases[:, OW] == out_w)
        rows = cases[sel][:, :4]
        assert set(rows[:, 3]) == {0, 1}
        got, ref = res.run(pkg, rows, scales[sel], out_h, out_w, 3)
        _bit_equal(got, ref, f"{out_h}x{out_w}")
        for b in range(0, len(rows), 2):                                       # the mirror is not a no-op
            assert not np.array_equal(got[0][b], got[0][b + 1]) and not np.array_equal(got[1][b], got[1][b + 1])
    assert pkg.ops.CALLS["det_batch_resize"] - before == len(sizes)


@pytest.mark.parametrize("out_h, out_w", [(48, 64), (47, 63)])
def test_padding_right_and_below_is_zero(pkg, gpu, out_h, out_w):
    """Samples smaller than the plane in width only, in height only, in both and in neither."""
    images, boxes, classes, _, _ = _fixture_split()
    res = _Resident(pkg, images, boxes, classes, gpu)
    rows = np.array([[0, out_h, out_w - 13, 1], [1, out_h - 9, out_w, 0], [4, out_h - 17, out_w - 30, 1], [0, out_h, out_w, 0]], np.int64)
    got, ref = res.run(pkg, rows, [1.25, 0.75, 1.0, 2.0], out_h, out_w, 5)
    _bit_equal(got, ref, f"padding {out_h}x{out_w}")
    for b, (_, oh, ow, _) in enumerate(rows):
        assert not got[0][b][:, oh:, :].any() and not got[0][b][:, :, ow:].any()
        assert got[0][b][:, :oh, :ow].any()
        n = len(boxes[rows[b, 0]])
        assert not got[1][b][n:].any() and not got[2][b][n:].any() and (got[2][b][:n] >= 3).all()


@pytest.mark.parametrize("out_h, out_w", [(41, 261), (40, 260), (150, 133)])
def test_several_tiles_bit_equal(pkg, gpu, out_h, out_w):
    """More than one workgroup per sample in both directions at sizes that are no multiple of the tile, every scale regime (0.6: 4-5
    taps, 1.0: identity passes, 1.6 and 2.0: 2-3 taps), windows at the origin of larger results and padding beside smaller ones."""
    split = _big_split(pkg)
    res = _Resident(pkg, split.images, split.boxes, split.classes, gpu)
    rows, scale = [], []
    for k, sc in enumerate((0.6, 1.0, 1.6, 2.0, 0.6, 1.0, 1.6, 2.0)):
        s = (k + k // 4) % 4
        h, w = split.images[s].shape[:2]
        rows.append([s, round(h * sc), round(w * sc), (k + k // 4) % 2])
        scale.append(sc)
    rows = np.array(rows, np.int64)
    assert (rows[:, 1] > out_h).any() and (rows[:, 2] < out_w).any() and (rows[:, 2] > out_w).any()
    _bit_equal(*res.run(pkg, rows, scale, out_h, out_w, 6), f"{out_h}x{out_w}")


def test_out_of_range_parameters_are_clamped(pkg, gpu):
    images, boxes, classes, _, _ = _fixture_split()
    res = _Resident(pkg, images, boxes, classes, gpu)
    dd = pkg.det_data
    big = 1 << 40
    rows = np.array([[-7, 30, 40, 0],                  # index below the split -> 0
                     [99, 30, 40, 5],                  # ... above -> the last image; flip is "non-zero"
                     [0, 0, -3, 0],                    # a size below h / max_shrink -> ceil(h / 3), ceil(w / 3)
                     [2, big, 9, 1],                   # a size beyond 32768 -> 32768 (9 x 7 source), of which the window is written
                     [2, 9, big, 0]], np.int64)
    scale = [1.0, 0.5, 2.0, 1.0, 3.0]
    got, ref = res.run(pkg, rows, scale, 33, 33, 3)
    _bit_equal(got, ref, "clamped")
    one = lambda k, oh, ow, fl, sc: dd._det_sample_numpy(images[k], boxes[k], classes[k], oh, ow, fl, np.float32(sc), 33, 33, 3)
    assert np.array_equal(ref[0][0], one(0, 30, 40, 0, 1.0)[0])
    assert np.array_equal(ref[0][1], one(4, 30, 40, 1, 0.5)[0]) and np.array_equal(ref[1][1], one(4, 30, 40, 1, 0.5)[1])
    assert np.array_equal(ref[0][2], one(0, 13, 18, 0, 2.0)[0])
    assert np.array_equal(ref[0][3], one(2, 32768, 9, 1, 1.0)[0])
    # a stricter bound from the caller clamps earlier: in/out <= 1.5
    got, ref = res.run(pkg, np.array([[1, 10, 10, 0]], np.int64), [1.0], 32, 32, 2, max_shrink=1.5)
    _bit_equal(got, ref, "max_shrink 1.5")
    assert np.array_equal(ref[0][0], dd._det_sample_numpy(images[1], boxes[1], classes[1], 43, 32, 0, np.float32(1.0), 32, 32, 2)[0])


def test_g_max_truncates_and_zero_boxes(pkg, gpu):
    images, boxes, classes, _, _ = _fixture_split()
    res = _Resident(pkg, images, boxes, classes, gpu)
    counts = [len(b) for b in boxes]
    assert max(counts) == 3 and min(counts) == 1
    rows = np.array([[s, 24, 24, s % 2] for s in range(5)], np.int64)
    for g_max in (1, 2, 0):
        got, ref = res.run(pkg, rows, [1.5] * 5, 24, 24, g_max)
        _bit_equal(got, ref, f"g_max {g_max}")
        for s in range(5):
            assert np.array_equal(got[2][s][:min(g_max, counts[s])], classes[s][:g_max])
    many = 300                                                                # more rows than the workgroup has threads
    got, ref = res.run(pkg, rows, [1.5] * 5, 24, 24, many)
    _bit_equal(got, ref, "g_max 300")
    assert not got[1][:, 3:].any() and not got[2][:, 3:].any()


def test_bad_table_entries_give_zero_samples(pkg, gpu):
    """An offset, a size or a box range that does not fit the split: the sample is all zero (image, boxes, labels), its neighbours are
    untouched, and nothing outside the buffers is read."""
    images, boxes, classes, _, _ = _fixture_split()
    res = _Resident(pkg, images, boxes, classes, gpu)
    img, off, hs, ws, bx, cl, box_off = res.packed
    rows = np.array([[0, 20, 28, 0], [1, 20, 28, 1], [2, 20, 28, 0], [3, 20, 28, 1], [4, 20, 28, 0]], np.int64)
    scale = [1.0, 2.0, 0.5, 1.5, 1.0]
    ref = pkg.det_data._det_batch_numpy(images, boxes, classes, *rows.T, np.asarray(scale, np.float32), 20, 28, 3)
    bad_off, bad_hs, bad_ws, bad_box = off.copy(), hs.copy(), ws.copy(), box_off.copy()
    bad_off[1] = 3 * (img.size // 3 - 5)               # 64 x 48 pixels from 5 pixels before the end
    bad_hs[2] = 40000                                  # beyond the largest side
    bad_ws[3] = 0
    bad_box[5] = len(bx) + 4                           # the last image's boxes run past the end
    bad_off2 = off.copy()
    bad_off2[0] = -3
    dev = res.t[0].device
    for tables, dead in (((img, bad_off, bad_hs, bad_ws, bx, cl, bad_box), {1, 2, 3, 4}), ((img, bad_off2, hs, ws, bx, cl, box_off), {0})):
        t = [torch.from_numpy(a).to(dev) for a in tables]
        p = torch.from_numpy(np.ascontiguousarray(rows.T)).to(dev)
        got = [x.cpu().numpy() for x in pkg.ops.det_batch_resize(*t, p[0], p[1], p[2], p[3], torch.tensor(scale, device=dev), 20, 28, 3)]
        for b in range(5):
            if b in dead:
                assert not got[0][b].any() and not got[1][b].any() and not got[2][b].any(), b
            else:
                _bit_equal([x[b] for x in got], [x[b] for x in ref], f"neighbour {b}")


def test_flipped_and_unflipped_of_one_source_in_one_batch(pkg, gpu):
    split = _big_split(pkg)
    res = _Resident(pkg, split.images, split.boxes, split.classes, gpu)
    h, w = split.images[1].shape[:2]
    oh, ow, sc = pkg.det_data.preprocess_size(h, w, 200., 300.)
    rows = np.array([[1, oh, ow, 1], [1, oh, ow, 0], [1, oh, ow, 1]], np.int64)
    got, ref = res.run(pkg, rows, [sc] * 3, oh, ow, 6)
    _bit_equal(got, ref, "flip pair")
    assert np.array_equal(got[0][0], got[0][2]) and not np.array_equal(got[0][0], got[0][1])
    n = len(split.boxes[1])
    assert np.array_equal(got[1][0][:n, [1, 3]], got[1][1][:n, [1, 3]]) and not np.array_equal(got[1][0][:n, [0, 2]], got[1][1][:n, [0, 2]])
    assert (got[1][0][:n, 2] > got[1][0][:n, 0]).all()


def _marked_split(n, seed):
    """Image k is the constant k + 1 everywhere, with k % 3 + 1 boxes of class k + 1: a batch names the indices it was made from."""
    rng = np.random.default_rng(seed)
    images, boxes, classes = [], [], []
    for k in range(n):
        a, b = sorted(int(v) for v in rng.integers(20, 61, 2))
        h, w = (b + 1, a) if k % 2 else (a, b + 1)
        images.append(np.full((h, w, 3), k + 1, np.uint8))
        g = k % 3 + 1
        boxes.append(np.array([[1 + j, 2, w - 2 - j, h - 3] for j in range(g)], np.float32))
        classes.append(np.full(g, k + 1, np.int64))
    return images, boxes, classes


def test_loader_epoch_structure(pkg, gpu):
    dd = pkg.det_data
    images, boxes, classes = _marked_split(13, 4)              # 7 fat, 6 tall
    loader = dd.DetDeviceLoader(images, boxes, classes, 2, gpu, True, 48., 64., seed=5)
    assert len(loader) == 3 + 3
    torch.cuda.synchronize()
    before = pkg.ops.CALLS["det_batch_resize"]
    torch.cuda.set_sync_debug_mode("error")            # a host synchronisation inside the epoch raises
    try:
        batches = list(loader)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert pkg.ops.CALLS["det_batch_resize"] - before == len(batches) == 6          # one launch per batch
    p, sc = loader.last_params, loader.last_scales
    seen = []
    for b, (x, bb, lb, s) in enumerate(batches):
        q = p[:, 2 * b:2 * b + 2]
        out_h, out_w, g_max = int(q[1].max()), int(q[2].max()), max(len(boxes[k]) for k in q[0])
        assert x.shape == (2, 3, out_h, out_w) and bb.shape == (2, g_max, 4) and lb.shape == (2, g_max) and s.shape == (2,)
        ids = lb.max(dim=1).values
        assert torch.equal((x.reshape(2, -1).max(dim=1).values * 255).round().long(), ids)
        assert len({images[k].shape[1] < images[k].shape[0] for k in q[0]}) == 1   # all tall or all fat
        ri, rb, rl = dd._det_batch_numpy(images, boxes, classes, *q, sc[2 * b:2 * b + 2], out_h, out_w, g_max, loader.max_shrink)
        _bit_equal([t.cpu().numpy() for t in (x, bb, lb)], (ri, rb, rl), f"loader batch {b}")
        assert np.array_equal(s.cpu().numpy(), sc[2 * b:2 * b + 2])
        seen += ids.tolist()
    assert len(set(seen)) == 12 and sorted(p[0] + 1) == sorted(seen) and set(p[3]) <= {0, 1}          # one fat image dropped
    for k, oh, ow, _ in p.T:
        assert (oh, ow) == dd.preprocess_size(*images[k].shape[:2], 48., 64.)[:2]
    # the same seed gives the same batches, epoch by epoch; the next epoch is another draw
    again = dd.DetDeviceLoader(images, boxes, classes, 2, gpu, True, 48., 64., seed=5)
    for a, b in zip(batches, again):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    second, second2 = list(loader), list(again)
    assert all(torch.equal(u, v) for a, b in zip(second, second2) for u, v in zip(a, b))
    assert not np.array_equal(p, loader.last_params)
    # a resumed run: the coming epoch from its fourth batch
    again.epoch = 1
    tail = list(again.batches(3))
    assert len(tail) == 3 and all(torch.equal(u, v) for a, b in zip(second[3:], tail) for u, v in zip(a, b))
    # data parallel: the ranks slice the same draw, padded alike
    halves = [list(dd.DetDeviceLoader(images, boxes, classes, 2, gpu, True, 48., 64., seed=5, rank=r, world=2)) for r in (0, 1)]
    for b, full in enumerate(batches):
        for i in range(4):
            assert torch.equal(torch.cat([halves[0][b][i], halves[1][b][i]]), full[i])
    with pytest.raises(RuntimeError, match="seed"):
        dd.DetDeviceLoader(images, boxes, classes, 2, gpu, True, 48., 64., rank=0, world=2)


def test_loader_evaluation_mode_and_refusals(pkg, gpu):
    dd = pkg.det_data
    images, boxes, classes = _marked_split(5, 9)
    loader = dd.DetDeviceLoader(images, boxes, classes, 2, gpu, False, 48., 64.)
    out = list(loader)
    assert len(loader) == len(out) == 3 and [o[0].shape[0] for o in out] == [2, 2, 1]
    assert torch.cat([o[2].max(dim=1).values for o in out]).tolist() == [1, 2, 3, 4, 5]         # in order
    assert not loader.last_params[3].any()                                                      # unflipped
    for k, (x, bb, lb, s) in enumerate((o[0][:1], o[1][:1], o[2][:1], o[3][:1]) for o in out[:2]):
        oh, ow, sc = dd.preprocess_size(*images[2 * k].shape[:2], 48., 64.)
        ri, rb, rl = dd._det_sample_numpy(images[2 * k], boxes[2 * k], classes[2 * k], oh, ow, 0, np.float32(sc), x.shape[2], x.shape[3],
                                          bb.shape[1])
        _bit_equal([t[0].cpu().numpy() for t in (x, bb, lb)], (ri, rb, rl), f"eval {k}")
        assert float(s[0]) == float(np.float32(sc))
    with pytest.raises(ValueError, match="KMAX"):
        dd.DetDeviceLoader(images, boxes, classes, 2, gpu, True, 5., 64.)                     # 20+ -> 5 is a reduction by more than 3
    with pytest.raises(ValueError, match="empty split"):
        dd.DetDeviceLoader([], [], [], 2, gpu, True)
