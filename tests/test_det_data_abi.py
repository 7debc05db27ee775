"""afan_det_batch_resize_u8 at the C-ABI without a GPU: the argument errors, the KMAX refusal, the empty batch, that the tensor
wrapper and its launch counter exist, that wrapper and loader refuse the host, and the synthetic split (no compute calls here)."""
import ctypes

import numpy as np
import pytest
import torch

ESHAPE, EALIGN, ENULL = -3, -2, -4


def _call(lib, p, **kw):
    a = dict(images=p, img_off=p, hs=p, ws=p, n_src=4, total_pixels=64, boxes_src=p, cls_src=p, box_off=p, total_boxes=8, index=p, oh=p,
             ow=p, flip=p, scale=p, out=p, boxes_out=p, labels_out=p, m=2, out_h=8, out_w=8, g_max=3, max_shrink=3.0, stream=None)
    a.update(kw)
    return lib.afan_det_batch_resize_u8(*a.values())


@pytest.fixture(scope="module")
def lib_p(pkg):
    buf = (ctypes.c_double * 64)()
    return pkg._lib.load(), ctypes.cast(buf, ctypes.c_void_p), buf


def test_symbol_wrapper_and_counter(pkg):
    sig = pkg._lib.SIGNATURES["afan_det_batch_resize_u8"]
    assert sig[0] is ctypes.c_int and len(sig[1]) == 24 and sig[1][22] is ctypes.c_double
    assert callable(pkg.ops.det_batch_resize)
    assert pkg.ops.CALLS["det_batch_resize"] >= 0 and "det_batch_resize" in pkg.ops.CALLS
    assert "det_batch_resize" not in set(pkg.ops.CALLS)            # the enumerated table stays the convolution table
    assert pkg.det_data.KMAX == 8 and pkg.det_data.MAX_SHRINK == 3.0


def test_argument_errors(lib_p):
    lib, p, _ = lib_p
    odd = ctypes.c_void_p(p.value + 4)                            # 4-byte aligned only
    for k in ("m", "out_h", "out_w", "n_src", "total_pixels", "total_boxes", "g_max"):
        assert _call(lib, p, **{k: -1}) == ESHAPE, k
    assert _call(lib, p, out_h=(1 << 20) + 1) == ESHAPE and _call(lib, p, g_max=(1 << 20) + 1) == ESHAPE
    assert _call(lib, p, out_h=1 << 16, out_w=1 << 16) == ESHAPE                          # a plane of more than INT_MAX pixels
    assert _call(lib, p, m=1 << 40, out_h=1 << 10, out_w=1 << 10) == ESHAPE               # 64-bit sizes would overflow
    assert _call(lib, p, n_src=0) == ESHAPE and _call(lib, p, total_pixels=0) == ESHAPE   # a batch from an empty split
    for k in ("images", "img_off", "hs", "ws", "boxes_src", "cls_src", "box_off", "index", "oh", "ow", "flip", "scale", "out", "boxes_out",
              "labels_out"):
        assert _call(lib, p, **{k: None}) == ENULL, k
    for k in ("img_off", "cls_src", "box_off", "index", "oh", "ow", "flip", "labels_out"):
        assert _call(lib, p, **{k: odd}) == EALIGN, k
    for k in ("out", "hs", "ws", "boxes_src", "scale", "boxes_out"):
        assert _call(lib, p, **{k: ctypes.c_void_p(p.value + 2)}) == EALIGN, k


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
    assert _call(lib, p, m=0, max_shrink=9.0) == ESHAPE           # (sizes are checked first, like afan_seg_batch_aug_u8)


def test_wrapper_and_loader_refuse_the_host(pkg):
    z = torch.zeros(4, dtype=torch.int64)
    before = pkg.ops.CALLS["det_batch_resize"]
    with pytest.raises(pkg.AfanLibraryError):
        pkg.ops.det_batch_resize(torch.zeros(12, dtype=torch.uint8), z, z.int(), z.int(), torch.zeros(2, 4), z[:2], torch.zeros(5, dtype=torch.int64),
                                 z, z, z, z, torch.zeros(4), 4, 4, 2)
    assert pkg.ops.CALLS["det_batch_resize"] == before
    s = pkg.det_data.SyntheticDetSplit(4, seed=0, min_side=8, max_side=12)
    with pytest.raises(pkg.AfanLibraryError):
        pkg.det_data.DetDeviceLoader(s.images, s.boxes, s.classes, 2, "cpu", True, 16., 24.)


def test_synthetic_split_and_packing(pkg):
    dd = pkg.det_data
    s = dd.SyntheticDetSplit(9, seed=3, min_side=9, max_side=20, classes=21, max_boxes=6)
    assert len(s) == 9
    ratios = [im.shape[1] / im.shape[0] for im in s.images]
    assert any(r < 1 for r in ratios) and any(r > 1 for r in ratios)         # both tall and fat
    for im, bx, cl in zip(s.images, s.boxes, s.classes):
        h, w = im.shape[:2]
        assert im.dtype == np.uint8 and im.shape[2] == 3 and 9 <= min(h, w) and max(h, w) <= 21
        assert bx.dtype == np.float32 and cl.dtype == np.int64 and 1 <= len(bx) == len(cl) <= 6
        assert (bx[:, 0] >= 0).all() and (bx[:, 1] >= 0).all() and (bx[:, 2] <= w - 1).all() and (bx[:, 3] <= h - 1).all()
        assert (bx[:, 2] > bx[:, 0]).all() and (bx[:, 3] > bx[:, 1]).all() and (cl >= 1).all() and (cl <= 20).all()
    s2 = dd.SyntheticDetSplit(9, seed=3, min_side=9, max_side=20)
    assert all((a == b).all() for a, b in zip(s.images, s2.images)) and all((a == b).all() for a, b in zip(s.boxes, s2.boxes))
    assert not all(a.shape == b.shape and (a == b).all() for a, b in zip(s.images, dd.SyntheticDetSplit(9, seed=4, min_side=9, max_side=20).images))
    img, off, hs, ws, bx, cl, box_off = dd.pack_det_split(s.images, s.boxes, s.classes)
    assert off[0] == 0 and (off % 3 == 0).all() and box_off[0] == 0 and box_off[-1] == len(bx) == len(cl) and len(box_off) == 10
    for k in range(9):
        n = int(hs[k]) * int(ws[k])
        assert (img[off[k]:off[k] + 3 * n].reshape(hs[k], ws[k], 3) == s.images[k]).all()
        assert (bx[box_off[k]:box_off[k + 1]] == s.boxes[k]).all() and (cl[box_off[k]:box_off[k + 1]] == s.classes[k]).all()
    with pytest.raises(ValueError, match="empty split"):
        dd.pack_det_split([], [], [])
