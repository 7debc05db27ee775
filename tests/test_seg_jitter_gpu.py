"""afan_seg_batch_aug_jitter_u8 on the GPU against seg_data._augment_jitter_numpy (itself held to Pillow's ImageEnhance bit for bit
by test_seg_jitter_ref.py): image and label bit-equal on scalar and vector widths, with a resize, with padding and at the identity
size, in all six orders, with the gray sum crossing workgroups on both axes; the workspace may be reused; a captured graph replays
with other parameters."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

FACTORS = [(0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (1.5, 1.5, 1.5), (0.73, 1.21, 0.88), (1.37, 0.61803, 1.4999), (0.5, 1.5, 1.0)]


def _tile():
    src = open(os.path.join(ROOT, "cv_a-fan_amd", "csrc", "afan_seg_data.hip")).read()
    return tuple(int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("TW", "TH"))


@functools.lru_cache(maxsize=1)
def _split():
    """The Pillow fixture's 37 x 53, 64 x 48 and 9 x 7 sources, one of 70 x 150, and a constant one."""
    g = golden("seg_aug_pillow")
    rng = np.random.default_rng(41)
    images, labels = [g[f"img{s}"] for s in range(3)], [g[f"lbl{s}"] for s in range(3)]
    images.append(rng.integers(0, 256, (70, 150, 3), dtype=np.uint8))
    labels.append(rng.integers(0, 19, (70, 150), dtype=np.uint8))
    images.append(np.full((40, 44, 3), (90, 200, 31), np.uint8))
    labels.append(np.full((40, 44), 7, np.uint8))
    return images, labels


class _Resident:
    def __init__(self, pkg, dev):
        self.images, self.labels = _split()
        img, lab, off, hs, ws = pkg.seg_data.pack_split(self.images, self.labels)
        self.t = [torch.from_numpy(a).to(dev) for a in (img, off, lab, hs, ws)]
        self.dev = dev

    def upload(self, rows, order, fac):
        p = torch.from_numpy(np.ascontiguousarray(rows.T)).to(self.dev)
        return [p[k] for k in range(6)] + [torch.from_numpy(order).to(self.dev)] + [torch.from_numpy(np.ascontiguousarray(fac[k])).to(self.dev)
                                                                                   for k in range(3)]

    def reference(self, pkg, rows, order, fac, out_h, out_w):
        return pkg.seg_data._augment_jitter_numpy_batch(self.images, self.labels, *rows.T, order, fac, out_h, out_w)


def _rows(pkg, specs, out_h, out_w, seed):
    """specs: (source, scale); the crop origin is a seeded draw inside the padded image, flips and orders cycle, factors cycle."""
    images, labels = _split()
    rng = np.random.default_rng(seed)
    rows, order, fac = [], [], []
    for k, (s, scale) in enumerate(specs):
        h, w = labels[s].shape
        oh, ow = max(int(h * scale), 1), max(int(w * scale), 1)
        _, _, pad, _, _ = pkg.seg_data._clamped(h, w, oh, ow, 0, 0, out_h, out_w)
        rows.append([s, oh, ow, rng.integers(0, oh + 2 * pad - out_h + 1), rng.integers(0, ow + 2 * pad - out_w + 1), (k // 2) % 2])
        order.append(k % 6)
        fac.append(FACTORS[(k + k // 6) % len(FACTORS)])
    return np.array(rows, np.int64), np.array(order, np.int64), np.ascontiguousarray(np.array(fac, np.float32).T)


def _bit_equal(gi, gl, ri, rl, what):
    gi, gl = gi.cpu().numpy(), gl.cpu().numpy()
    assert np.array_equal(gl, rl), f"{what}: {int((gl != rl).sum())} label pixels differ"
    bad = gi.view(np.uint32) != ri.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} image values differ, max |d| = {np.abs(gi - ri).max():.3e}"


# every source at the identity size, reduced, enlarged; 0.5 on 9 x 7 and 1.0 on the small ones pad on both axes
SPECS = [(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (0, 0.5), (1, 0.73), (2, 0.5), (3, 0.61803), (4, 1.37), (0, 1.5), (1, 1.999),
         (2, 1.5), (3, 0.4), (4, 0.6), (0, 0.61803), (1, 0.5), (3, 1.21)]


@pytest.mark.parametrize("out_h, out_w", [(33, 33), (32, 32), (24, 40)])
def test_bit_equal_with_the_restatement(pkg, gpu, out_h, out_w):
    """33 x 33 takes the scalar stores, 32 x 32 and 24 x 40 the 16-byte ones.  18 samples: three rounds of the six orders, each
    factor triple (0.5, 1.0, 1.5 and interior values on both sides of 1), sources resized, padded and at their own size, one constant."""
    res = _Resident(pkg, gpu)
    rows, order, fac = _rows(pkg, SPECS, out_h, out_w, seed=out_w)
    assert set(order) == set(range(6)) and any(r[1] == _split()[1][r[0]].shape[0] for r in rows)
    pads = [pkg.seg_data._clamped(*_split()[1][r[0]].shape, r[1], r[2], 0, 0, out_h, out_w)[2] for r in rows]
    assert any(p > 0 for p in pads) and any(p == 0 for p in pads)
    before = pkg.ops.CALLS["seg_batch_aug_jitter"]
    gi, gl = pkg.ops.seg_batch_aug_jitter(*res.t, *res.upload(rows, order, fac), out_h, out_w)
    assert pkg.ops.CALLS["seg_batch_aug_jitter"] - before == 1
    assert gi.shape == (len(rows), 3, out_h, out_w) and gi.dtype == torch.float32 and gl.dtype == torch.int64
    ri, rl = res.reference(pkg, rows, order, fac, out_h, out_w)
    _bit_equal(gi, gl, ri, rl, f"{out_h}x{out_w}")
    plain = pkg.seg_data._augment_numpy_batch(*_split(), *rows.T, out_h, out_w)
    assert not np.array_equal(plain[0], ri) and np.array_equal(plain[1], rl)              # the jitter did something; never to the label
    unit = [k for k in range(len(rows)) if tuple(fac[:, k]) == (1.0, 1.0, 1.0)]
    assert unit and all(np.array_equal(plain[0][k], ri[k]) for k in unit)


@pytest.mark.parametrize("vec", [True, False])
def test_gray_sum_crosses_workgroups(pkg, gpu, vec):
    """The 70 x 150 source on an output of more than one tile on both axes (3 x 2 tiles, the last ones partial): contrast's mean is a
    sum over six workgroups.  A batch of 5 with a repeated index, at the identity size, resized, and padded on both axes."""
    tw, th = _tile()
    out_h, out_w = 2 * th + 3, tw + (12 if vec else 13)
    assert out_h <= 70 and out_w <= 150 and (out_w % 4 == 0) == vec
    res = _Resident(pkg, gpu)
    rows, order, fac = _rows(pkg, [(3, 1.0), (3, 1.31), (3, 1.0), (3, 0.5), (1, 1.0)], out_h, out_w, seed=7)
    order[:] = (2, 3, 5, 1, 4)                                   # contrast first, second (twice), last
    pad = pkg.seg_data._clamped(64, 48, 64, 48, 0, 0, out_h, out_w)[2]
    assert pad > 0
    rows[4, 3] = pad + 10                                        # the 64 x 48 source: rows of the image, columns of image and padding
    ri, rl = res.reference(pkg, rows, order, fac, out_h, out_w)
    args = res.upload(rows, order, fac)
    ws = torch.full((8,), -1, dtype=torch.int64, device=gpu)      # a dirty workspace, longer than the batch
    gi, gl = pkg.ops.seg_batch_aug_jitter(*res.t, *args, out_h, out_w, workspace=ws)
    _bit_equal(gi, gl, ri, rl, "several tiles")
    sums = ws.cpu().numpy()
    assert (sums[:5] > 0).all() and (sums[5:] == -1).all()        # the call clears and fills one entry per sample, no more
    gi2, gl2 = pkg.ops.seg_batch_aug_jitter(*res.t, *args, out_h, out_w, workspace=ws)
    assert torch.equal(gi, gi2) and torch.equal(gl, gl2) and np.array_equal(ws.cpu().numpy(), sums)


def test_order_code_is_clamped(pkg, gpu):
    res = _Resident(pkg, gpu)
    rows, _, fac = _rows(pkg, [(0, 1.0), (1, 0.73)], 32, 32, seed=3)
    order = np.array([-4, 1 << 40], np.int64)
    gi, gl = pkg.ops.seg_batch_aug_jitter(*res.t, *res.upload(rows, order, fac), 32, 32)
    ri, rl = res.reference(pkg, rows, np.array([0, 5], np.int64), fac, 32, 32)
    _bit_equal(gi, gl, ri, rl, "clamped order")


def test_graph_replay_with_other_parameters(pkg, gpu):
    """Captured once (clear, statistics launch, batch launch), replayed twice after the parameter tensors were overwritten: each
    replay equals the eager call with those parameters."""
    ops = pkg.ops
    res = _Resident(pkg, gpu)
    out_h, out_w = 33, 40
    sets = [_rows(pkg, [(0, 1.0), (3, 0.61803), (2, 1.5)], out_h, out_w, seed=1), _rows(pkg, [(1, 0.73), (4, 1.0), (3, 1.0)], out_h, out_w, seed=2)]
    sets[1][1][:] = (4, 2, 3)
    eager = [ops.seg_batch_aug_jitter(*res.t, *res.upload(*s), out_h, out_w) for s in sets]
    for s, (gi, gl) in zip(sets, eager):
        _bit_equal(gi, gl, *res.reference(pkg, *s, out_h, out_w), "eager")
    static = [t.clone() for t in res.upload(*sets[0])]
    ws = torch.zeros(3, dtype=torch.int64, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with ops.no_gc_during_capture(), torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        out = ops.seg_batch_aug_jitter(*res.t, *static, out_h, out_w, workspace=ws)
    for k in (1, 0):
        for dst, src in zip(static, res.upload(*sets[k])):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(out[0], eager[k][0]) and torch.equal(out[1], eager[k][1]), f"replay with parameter set {k}"
