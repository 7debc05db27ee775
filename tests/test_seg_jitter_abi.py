"""afan_seg_batch_aug_jitter_u8 at the C-ABI without a GPU: the argument errors, the empty batch, and that the tensor wrapper, its
launch counter and its refusal of non-finite factors exist (no compute calls here)."""
import ctypes

import numpy as np
import pytest
import torch

ESHAPE, EALIGN, ENULL = -3, -2, -4
POINTERS = ("images", "img_off", "labels", "hs", "ws", "index", "oh", "ow", "top", "left", "flip", "order", "brightness", "contrast",
            "saturation", "gray_sum", "out", "labels_out")


def _call(lib, p, **kw):
    a = dict(images=p, img_off=p, labels=p, hs=p, ws=p, n_src=4, total_pixels=64, index=p, oh=p, ow=p, top=p, left=p, flip=p, order=p,
             brightness=p, contrast=p, saturation=p, gray_sum=p, out=p, labels_out=p, m=2, out_h=8, out_w=8, max_shrink=3.0, stream=None)
    a.update(kw)
    return lib.afan_seg_batch_aug_jitter_u8(*a.values())


@pytest.fixture(scope="module")
def lib_p(pkg):
    buf = (ctypes.c_double * 64)()
    return pkg._lib.load(), ctypes.cast(buf, ctypes.c_void_p), buf


def test_symbol_wrapper_and_counter(pkg):
    sig = pkg._lib.SIGNATURES
    assert "afan_seg_batch_aug_jitter_u8" in sig
    assert len(sig["afan_seg_batch_aug_jitter_u8"][1]) == len(sig["afan_seg_batch_aug_u8"][1]) + 5      # order, 3 factors, workspace
    assert callable(pkg.ops.seg_batch_aug_jitter)
    assert pkg.ops.CALLS["seg_batch_aug_jitter"] >= 0 and "seg_batch_aug_jitter" in pkg.ops.CALLS
    assert "seg_batch_aug_jitter" not in set(pkg.ops.CALLS)       # the enumerated table stays the convolution table


def test_argument_errors(lib_p):
    lib, p, _ = lib_p
    odd = ctypes.c_void_p(p.value + 4)                            # 4-byte aligned only
    for k in ("m", "out_h", "out_w", "n_src", "total_pixels"):
        assert _call(lib, p, **{k: -1}) == ESHAPE, k
    assert _call(lib, p, out_h=(1 << 20) + 1) == ESHAPE
    assert _call(lib, p, out_h=1 << 16, out_w=1 << 16) == ESHAPE
    assert _call(lib, p, m=1 << 40, out_h=1 << 10, out_w=1 << 10) == ESHAPE
    assert _call(lib, p, n_src=0) == ESHAPE and _call(lib, p, total_pixels=0) == ESHAPE
    for bad in (3.0000001, 0.999, float("nan")):
        assert _call(lib, p, max_shrink=bad) == ESHAPE, bad
    for k in POINTERS:
        assert _call(lib, p, **{k: None}) == ENULL, k
    for k in ("img_off", "index", "oh", "ow", "top", "left", "flip", "order", "gray_sum", "labels_out"):
        assert _call(lib, p, **{k: odd}) == EALIGN, k
    for k in ("out", "hs", "ws", "brightness", "contrast", "saturation"):
        assert _call(lib, p, **{k: ctypes.c_void_p(p.value + 2)}) == EALIGN, k


def test_empty_batch_is_no_launch(lib_p):
    lib, p, _ = lib_p
    assert _call(lib, p, m=0) == 0
    assert _call(lib, None, m=0) == 0                             # nothing is dereferenced
    assert _call(lib, None, out_h=0) == 0 and _call(lib, None, out_w=0) == 0
    assert _call(lib, p, m=0, max_shrink=9.0) == ESHAPE           # (sizes are checked first, like afan_seg_batch_aug_u8)


def test_ops_refuses_non_finite_factors(pkg):
    ops = pkg.ops
    f = ops.jitter_factors([[0.5, 1.0], [1.5, 0.75], [1.0, 1.25]])
    assert f.dtype == np.float32 and f.shape == (3, 2)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            ops.jitter_factors([1.0, bad, 1.0])
    z = torch.zeros(4, dtype=torch.int64)
    one = torch.ones(4)
    args = (torch.zeros(12, dtype=torch.uint8), z, torch.zeros(4, dtype=torch.uint8), z.int(), z.int(), z, z, z, z, z, z, z)
    with pytest.raises(ValueError, match="finite"):               # refused on the host, before any tensor is looked at
        ops.seg_batch_aug_jitter(*args, one, torch.tensor([1.0, float("nan"), 1.0, 1.0]), one, 4, 4)
    with pytest.raises(pkg.AfanLibraryError):                     # finite factors: the host tensors are refused as everywhere
        ops.seg_batch_aug_jitter(*args, one, one, one, 4, 4)


def test_loader_arguments_on_the_host(pkg):
    s = pkg.seg_data.SyntheticSegSplit(2, seed=0, min_side=8, max_side=12, classes=19)
    with pytest.raises(pkg.AfanLibraryError):
        pkg.seg_data.SegDeviceLoader(s.images, s.labels, 2, "cpu", True, 8, jitter=(0.5, 0.5, 0.5), scale_range=(1, 1))
