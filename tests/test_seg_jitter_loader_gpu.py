"""SegDeviceLoader with colour jitter (the Cityscapes training transform) on the GPU: its batches equal the numpy restatement at the
parameters it drew; without jitter it draws and builds exactly what it did before the option existed; scale_range=(1, 1) refuses a
source smaller than the crop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _legacy_draw(sd, hs, ws, n, batch, crop, seed, epoch, scale_range=(0.5, 2.0)):
    """SegDeviceLoader._draw's training branch as it was before the jitter option: the same generator calls in the same order."""
    rng = np.random.default_rng([int(seed), epoch])
    idx = rng.permutation(n)[:(n // batch) * batch]
    h, w = hs[idx], ws[idx]
    scale = rng.uniform(scale_range[0], scale_range[1], idx.shape[0])
    oh = np.maximum((h * scale).astype(np.int64), 1)
    ow = np.maximum((w * scale).astype(np.int64), 1)
    p1 = np.where(ow < crop, (1 + crop - ow) // 2, 0)
    p2 = np.where(oh + 2 * p1 < crop, (1 + crop - (oh + 2 * p1)) // 2, 0)
    pad = p1 + p2
    top = rng.integers(0, oh + 2 * pad - crop + 1)
    left = rng.integers(0, ow + 2 * pad - crop + 1)
    flip = (rng.random(idx.shape[0]) < 0.5).astype(np.int64)
    return np.stack([idx, oh, ow, top, left, flip]).astype(np.int64)


def _cat(batches):
    return torch.cat([b[0] for b in batches]).cpu().numpy(), torch.cat([b[1] for b in batches]).cpu().numpy()


def test_jitter_loader_equals_the_restatement(pkg, gpu):
    sd = pkg.seg_data
    split = sd.SyntheticSegSplit(7, seed=3, min_side=40, max_side=56, classes=19)
    loader = sd.SegDeviceLoader(split.images, split.labels, 3, gpu, True, 36, seed=9, jitter=(0.5, 0.5, 0.5), scale_range=(1, 1))
    assert len(loader) == 2
    before = pkg.ops.CALLS["seg_batch_aug_jitter"], pkg.ops.CALLS["seg_batch_aug"]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")            # a host synchronisation inside the epoch raises
    try:
        first = list(loader)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert (pkg.ops.CALLS["seg_batch_aug_jitter"] - before[0], pkg.ops.CALLS["seg_batch_aug"] - before[1]) == (2, 0)
    for epoch in range(2):
        batches = first if epoch == 0 else list(loader)
        p, (order, fac) = loader.last_params, loader.last_jitter
        assert p.shape == (6, 6) and order.shape == (6,) and fac.shape == (3, 6) and fac.dtype == np.float32 and order.dtype == np.int64
        assert np.array_equal(p, _legacy_draw(sd, loader.hs, loader.ws, 7, 3, 36, 9, epoch, (1.0, 1.0)))       # the jitter draws come after
        assert (p[1] == loader.hs[p[0]]).all() and (p[2] == loader.ws[p[0]]).all()                             # no random scale
        assert ((order >= 0) & (order <= 5)).all() and ((fac >= 0.5) & (fac <= 1.5)).all() and len(np.unique(fac)) == fac.size
        ri, rl = sd._augment_jitter_numpy_batch(split.images, split.labels, *p, order, fac, 36, 36, loader.max_shrink)
        gi, gl = _cat(batches)
        assert np.array_equal(gl, rl) and set(np.unique(gl).tolist()) <= set(range(19)) | {255}
        assert np.array_equal(gi.view(np.uint32), ri.view(np.uint32)), f"epoch {epoch}: {int((gi != ri).sum())} image values differ"
        assert not np.array_equal(ri, sd._augment_numpy_batch(split.images, split.labels, *p, 36, 36, loader.max_shrink)[0])
    assert not np.array_equal(_cat(first)[0], gi)                                                              # epochs differ
    # validation never jitters, whatever it is handed
    val = sd.SegDeviceLoader(split.images[:2], split.labels[:2], 2, gpu, False, 36, jitter=(0.5, 0.5, 0.5))
    x, y = next(iter(val))
    assert val.jitter is None and val.last_jitter is None
    assert np.array_equal(x[0].cpu().numpy(), sd.QUOT255[split.images[0]].transpose(2, 0, 1))


def test_loader_without_jitter_is_what_it_was(pkg, gpu):
    sd = pkg.seg_data
    split = sd.SyntheticSegSplit(9, seed=4, min_side=20, max_side=60)
    plain = sd.SegDeviceLoader(split.images, split.labels, 4, gpu, True, 33, seed=5)
    none = sd.SegDeviceLoader(split.images, split.labels, 4, gpu, True, 33, seed=5, jitter=None)
    before = pkg.ops.CALLS["seg_batch_aug_jitter"]
    for epoch in range(2):
        a, b = list(plain), list(none)
        want = _legacy_draw(sd, plain.hs, plain.ws, 9, 4, 33, 5, epoch)
        assert np.array_equal(plain.last_params, want) and np.array_equal(none.last_params, want)
        assert plain.last_jitter is None and none.last_jitter is None
        ri, rl = sd._augment_numpy_batch(split.images, split.labels, *want, 33, 33, plain.max_shrink)
        for got in (a, b):
            gi, gl = _cat(got)
            assert np.array_equal(gl, rl) and np.array_equal(gi.view(np.uint32), ri.view(np.uint32))
    assert pkg.ops.CALLS["seg_batch_aug_jitter"] == before


def test_unit_scale_refuses_a_source_smaller_than_the_crop(pkg, gpu):
    sd = pkg.seg_data
    split = sd.SyntheticSegSplit(3, seed=1, min_side=30, max_side=34, classes=19)
    with pytest.raises(ValueError, match="smaller than the crop"):
        sd.SegDeviceLoader(split.images, split.labels, 2, gpu, True, 35, seed=1, jitter=(0.5, 0.5, 0.5), scale_range=(1, 1))
    sd.SegDeviceLoader(split.images, split.labels, 2, gpu, True, 35, seed=1)                  # with the random scale it pads, as before
    sd.SegDeviceLoader(split.images, split.labels, 2, gpu, True, 30, seed=1, scale_range=(1, 1))
