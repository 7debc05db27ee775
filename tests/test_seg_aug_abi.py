"""afan_seg_batch_aug_u8 at the C-ABI without a GPU: the argument errors, the KMAX refusal, the empty batch, and that the tensor
wrapper and its launch counter exist (no compute calls here)."""
import ctypes

import pytest
import torch

ESHAPE, EALIGN, ENULL = -3, -2, -4


def _call(lib, p, **kw):
    a = dict(images=p, img_off=p, labels=p, hs=p, ws=p, n_src=4, total_pixels=64, index=p, oh=p, ow=p, top=p, left=p, flip=p, out=p,
             labels_out=p, m=2, out_h=8, out_w=8, max_shrink=3.0, stream=None)
    a.update(kw)
    return lib.afan_seg_batch_aug_u8(*a.values())


@pytest.fixture(scope="module")
def lib_p(pkg):
    buf = (ctypes.c_double * 64)()
    return pkg._lib.load(), ctypes.cast(buf, ctypes.c_void_p), buf


def test_symbol_wrapper_and_counter(pkg):
    assert "afan_seg_batch_aug_u8" in pkg._lib.SIGNATURES
    assert callable(pkg.ops.seg_batch_aug)
    assert pkg.ops.CALLS["seg_batch_aug"] >= 0 and "seg_batch_aug" in pkg.ops.CALLS
    assert "seg_batch_aug" not in set(pkg.ops.CALLS)              # the enumerated table stays the convolution table
    assert pkg.seg_data.KMAX == 8 and pkg.seg_data.MAX_SHRINK == 3.0


def test_argument_errors(lib_p):
    lib, p, _ = lib_p
    odd = ctypes.c_void_p(p.value + 4)                            # 4-byte aligned only
    for k in ("m", "out_h", "out_w", "n_src", "total_pixels"):
        assert _call(lib, p, **{k: -1}) == ESHAPE, k
    assert _call(lib, p, out_h=(1 << 20) + 1) == ESHAPE
    assert _call(lib, p, out_h=1 << 16, out_w=1 << 16) == ESHAPE                          # a plane of more than INT_MAX pixels
    assert _call(lib, p, m=1 << 40, out_h=1 << 10, out_w=1 << 10) == ESHAPE               # 64-bit sizes would overflow
    assert _call(lib, p, n_src=0) == ESHAPE and _call(lib, p, total_pixels=0) == ESHAPE   # a batch from an empty split
    for k in ("images", "img_off", "labels", "hs", "ws", "index", "oh", "ow", "top", "left", "flip", "out", "labels_out"):
        assert _call(lib, p, **{k: None}) == ENULL, k
    for k in ("img_off", "index", "oh", "ow", "top", "left", "flip", "labels_out"):
        assert _call(lib, p, **{k: odd}) == EALIGN, k
    assert _call(lib, p, out=ctypes.c_void_p(p.value + 2)) == EALIGN
    assert _call(lib, p, hs=ctypes.c_void_p(p.value + 2)) == EALIGN


def test_kmax_refusal(lib_p):
    """8 taps per axis cover in/out <= 3: a larger reduction is refused by the host entry, as is a bound below 1 or a NaN."""
    lib, p, _ = lib_p
    for bad in (3.0000001, 4.0, 0.999, float("nan"), float("inf"), -1.0):
        assert _call(lib, p, max_shrink=bad) == ESHAPE, bad


def test_empty_batch_is_no_launch(lib_p):
    lib, p, _ = lib_p
    assert _call(lib, p, m=0) == 0
    assert _call(lib, None, m=0) == 0                             # nothing is dereferenced
    assert _call(lib, None, out_h=0) == 0 and _call(lib, None, out_w=0) == 0
    assert _call(lib, p, m=0, max_shrink=9.0) == ESHAPE           # (sizes are checked first, like afan_batch_crop_flip_u8)


def test_wrapper_and_loader_refuse_the_host(pkg):
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(pkg.AfanLibraryError):
        pkg.ops.seg_batch_aug(torch.zeros(12, dtype=torch.uint8), z, torch.zeros(4, dtype=torch.uint8), z.int(), z.int(), z, z, z, z, z,
                              z, 4, 4)
    s = pkg.seg_data.SyntheticSegSplit(2, seed=0, min_side=8, max_side=12)
    with pytest.raises(pkg.AfanLibraryError):
        pkg.seg_data.SegDeviceLoader(s.images, s.labels, 2, "cpu", True, 8)


def test_synthetic_split_and_packing(pkg):
    sd = pkg.seg_data
    s = sd.SyntheticSegSplit(5, seed=3, min_side=9, max_side=20, classes=21)
    assert len(s) == 5 and len({l.shape for l in s.labels}) > 1
    for im, lb in zip(s.images, s.labels):
        assert im.dtype == lb.dtype == "uint8" and im.shape == lb.shape + (3,) and 9 <= min(lb.shape) and max(lb.shape) <= 20
        assert set(lb.reshape(-1).tolist()) <= set(range(21)) | {255}
    assert any((lb == 255).any() for lb in s.labels)
    img, lab, off, hs, ws = sd.pack_split(s.images, s.labels)
    assert img.size == 3 * lab.size and off[0] == 0 and (off % 3 == 0).all()
    for k in range(5):
        n = int(hs[k]) * int(ws[k])
        assert (img[off[k]:off[k] + 3 * n].reshape(hs[k], ws[k], 3) == s.images[k]).all()
        assert (lab[off[k] // 3:off[k] // 3 + n].reshape(hs[k], ws[k]) == s.labels[k]).all()
    s2 = sd.SyntheticSegSplit(5, seed=3, min_side=9, max_side=20)
    assert all((a == b).all() for a, b in zip(s.images, s2.images))
