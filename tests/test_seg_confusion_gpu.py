"""afan_seg_confusion_upsampled (bilinear resize + arg-max + confusion matrix in one launch, through ops.seg_confusion_upsampled)
against the route it replaces, EXACTLY: ops.upsample_bilinear (whose values the kernel must reproduce to the bit), torch.max(dim=1)[1]
and numpy's masked bincount (tests/seg_eval_refs.fast_hist, the reference's _fast_hist).  Integer counts: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import seg_eval_refs as E

pytestmark = pytest.mark.gpu

# (h, w) -> (H, W): one ragged 16 x 16 tile; ragged on both axes with h != w; the entry test's DeepLab shape; a ratio below 2, which
# afan_ce2d_upsampled declines; equal sizes; a single source pixel
SHAPES = [((3, 3), (9, 9)), ((5, 4), (17, 19)), ((9, 9), (33, 33)), ((33, 33), (65, 65)), ((7, 7), (7, 7)), ((1, 1), (5, 5))]


def _logits(kind, shape, gen):
    if kind == "gauss":
        return torch.randn(shape, generator=gen)
    return torch.randint(-1, 2, shape, generator=gen).float()          # {-1, 0, 1}: many pixels tie (the first maximum wins)


def _labels(c, shape, gen):
    t = torch.randint(0, c, shape, generator=gen)
    r = torch.rand(shape, generator=gen)
    t[r < 0.10] = 255
    t[(r >= 0.10) & (r < 0.15)] = torch.randint(c, 255, shape, generator=gen)[(r >= 0.10) & (r < 0.15)]      # [C, 254]: skipped too
    return t


def _expected(pkg, lo_dev, t_dev):
    """The replaced route on the same logits: the library's resize, torch's max, the host count."""
    c = lo_dev.shape[1]
    up = pkg.ops.upsample_bilinear(lo_dev.contiguous(memory_format=torch.channels_last), t_dev.shape[1:])
    return E.fast_hist(c, t_dev.cpu().numpy(), up.max(dim=1)[1].cpu().numpy())


def _got(pkg, lo_dev, t_dev, hist=None):
    c = lo_dev.shape[1]
    hist = torch.zeros(c * c, dtype=torch.int64, device=lo_dev.device) if hist is None else hist
    before = pkg.ops.CALLS["seg_confusion"]
    assert pkg.ops.seg_confusion_upsampled(lo_dev, t_dev, hist) is hist
    assert pkg.ops.CALLS["seg_confusion"] == before + 1
    return hist.cpu().numpy().reshape(c, c)


@pytest.mark.parametrize("kind", ["gauss", "ternary"])
@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [2, 21, 32])
def test_matrix_equals_resize_max_bincount(pkg, gpu, c, n, src, dst, kind):
    gen = torch.Generator().manual_seed(1000 * c + 10 * n + src[0])
    lo = _logits(kind, (n, c) + src, gen).to(gpu)
    t = _labels(c, (n,) + dst, gen).to(gpu)
    ref = _expected(pkg, lo, t)
    got = _got(pkg, lo.contiguous(memory_format=torch.channels_last), t)
    assert np.array_equal(got, ref)
    assert got.sum() == int(((t >= 0) & (t < c)).sum())
    if kind == "ternary" and c > 2 and src != dst:
        # the first-maximum rule was exercised: against the LAST maximum the matrix differs
        up = pkg.ops.upsample_bilinear(lo.contiguous(memory_format=torch.channels_last), dst)
        last = (c - 1) - up.flip(1).max(dim=1)[1]
        assert not np.array_equal(E.fast_hist(c, t.cpu().numpy(), last.cpu().numpy()), ref) or dst == (5, 5)
    assert np.array_equal(_got(pkg, lo, t), ref)                        # NCHW logits: made channels-last by ops


@pytest.mark.parametrize("kind", ["gauss", "ternary"])
def test_every_workgroup_walks_several_tiles(pkg, gpu, kind):
    """4 x 21 x 129 x 129 -> 513 x 513: 4 x 33 x 33 = 4356 tiles of 16 x 16 on a persistent grid of two workgroups per CU (512 on the
    256 CUs): every workgroup takes 8 or 9 tiles, stages a new source window for each and flushes once."""
    gen = torch.Generator().manual_seed(7)
    lo = _logits(kind, (4, 21, 129, 129), gen).to(gpu).contiguous(memory_format=torch.channels_last)
    t = _labels(21, (4, 513, 513), gen).to(gpu)
    assert 4 * 33 * 33 >= 2 * 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    assert np.array_equal(_got(pkg, lo, t), _expected(pkg, lo, t))


def test_labels_ignored_out_of_range_and_views(pkg, gpu):
    gen = torch.Generator().manual_seed(3)
    c = 21
    lo = torch.randn((3, c, 9, 9), generator=gen).to(gpu).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, c, (3, 33, 33), generator=gen)
    t[0] = 255                                                         # an image that is entirely ignored
    t[1, :, :7] = 255
    t[1, 5:9, 10:20] = torch.randint(c, 255, (4, 10), generator=gen)   # [C, 254]
    t[2, 0, 0], t[2, 1, 1], t[2, 2, 2] = -1, c, 254
    t = t.to(gpu)
    ref = _expected(pkg, lo, t)
    assert np.array_equal(_got(pkg, lo, t), ref) and ref.sum() == int(((t >= 0) & (t < c)).sum())
    # all ignored: the matrix is unchanged
    hist = torch.arange(c * c, dtype=torch.int64, device=gpu)
    assert np.array_equal(_got(pkg, lo[:1], t[:1], hist).reshape(-1), np.arange(c * c))
    # a target that is a non-contiguous view
    wide = torch.full((3, 33, 66), 255, dtype=torch.int64, device=gpu)
    wide[:, :, ::2] = t
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    assert np.array_equal(_got(pkg, lo, view), ref)
    tt = t.transpose(1, 2)
    assert not tt.is_contiguous()
    assert np.array_equal(_got(pkg, lo, tt), _expected(pkg, lo, tt.contiguous()))


def test_accumulates_with_64_bit_adds(pkg, gpu):
    gen = torch.Generator().manual_seed(4)
    c = 5
    a = (torch.randn((2, c, 5, 4), generator=gen).to(gpu), _labels(c, (2, 17, 19), gen).to(gpu))
    b = (torch.randn((1, c, 3, 3), generator=gen).to(gpu), _labels(c, (1, 9, 9), gen).to(gpu))
    ra, rb = _expected(pkg, *a), _expected(pkg, *b)
    assert (ra > 0).all()
    hist = torch.zeros(c * c, dtype=torch.int64, device=gpu)
    _got(pkg, *a, hist)
    assert np.array_equal(_got(pkg, *b, hist), ra + rb)                  # two calls into one matrix: the sum, never zeroed
    # high bits survive, and a carry out of the low 32 bits goes into them
    pre = np.full(c * c, (7 << 32) + 5, np.int64)
    pre[::2] = (1 << 32) - 1
    hist = torch.from_numpy(pre.copy()).to(gpu)
    assert np.array_equal(_got(pkg, *a, hist), pre.reshape(c, c) + ra)


def test_nan_is_the_maximum(pkg, gpu):
    gen = torch.Generator().manual_seed(5)
    c = 21
    lo = torch.randn((1, c, 9, 9), generator=gen)
    lo[0, 13, 4, 4] = float("nan")
    lo[0, 6, 0, 8], lo[0, 2, 0, 8] = float("nan"), float("nan")        # two NaNs in one pixel: the first (class 2) wins
    lo = lo.to(gpu).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, c, (1, 33, 33), generator=gen).to(gpu)
    up = pkg.ops.upsample_bilinear(lo, (33, 33))
    pred = up.max(dim=1)[1]
    nanpx = torch.isnan(up).any(1)
    assert int(nanpx.sum()) > 4 and set(pred[nanpx].tolist()) == {2, 13}
    got = _got(pkg, lo, t)
    assert np.array_equal(got, E.fast_hist(c, t.cpu().numpy(), pred.cpu().numpy()))
    assert got[:, 13].sum() >= int((pred == 13).sum()) > 0


def test_wrapper_rejects_what_the_kernel_does_not_take(pkg, gpu):
    lo = torch.zeros((1, 3, 4, 4), device=gpu)
    t = torch.zeros((1, 8, 8), dtype=torch.int64, device=gpu)
    h = torch.zeros(9, dtype=torch.int64, device=gpu)
    with pytest.raises(TypeError):
        pkg.ops.seg_confusion_upsampled(lo.bfloat16(), t, h)
    with pytest.raises(TypeError):
        pkg.ops.seg_confusion_upsampled(lo, t.int(), h)
    with pytest.raises(TypeError):
        pkg.ops.seg_confusion_upsampled(lo, t, h[:8])
    with pytest.raises(pkg.AfanLibraryError, match="AFAN_ESHAPE"):
        pkg.ops.seg_confusion_upsampled(lo, t[:, :3, :3].contiguous(), h)            # down-scaling
    assert not h.any()
