"""ops.batch_crop_flip (afan_batch_crop_flip_u8: gather + random crop + flip + /255 in one launch) against the torch chain it
replaces, cls_data._augment_torch, bit for bit, labels included."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu


def _mp():
    return importlib.import_module("cv_a-fan_amd.cls_data")


def _split(n, c, h, w, gpu, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, c, h, w), dtype=torch.uint8, generator=g).to(gpu),
            torch.randint(0, 10, (n,), generator=g).to(gpu))


def _check(pkg, src, labels, index, top, left, flip, pad):
    before = pkg.ops.CALLS["batch_crop_flip"]
    out, lab = pkg.ops.batch_crop_flip(src, index, top, left, flip, labels=labels, pad=pad)
    assert pkg.ops.CALLS["batch_crop_flip"] == before + 1
    want = _mp()._augment_torch(src[index], top, left, flip, pad)
    assert out.dtype == torch.float32 and out.shape == want.shape and out.is_contiguous()
    assert torch.equal(out, want)
    assert torch.equal(lab, labels[index])
    return out


def test_every_corner_both_flips_repeated_indices(pkg, gpu):
    src, labels = _split(5, 3, 32, 32, gpu)
    index = torch.tensor([4, 0, 4, 2, 2, 1, 0, 3, 4], device=gpu)
    # (top, left) over all of {0, 4, 8}^2: rows / columns entirely inside the padding on each side
    top = torch.tensor([0, 0, 0, 4, 4, 4, 8, 8, 8], device=gpu)
    left = torch.tensor([0, 4, 8, 0, 4, 8, 0, 4, 8], device=gpu)
    flip = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 1], device=gpu, dtype=torch.bool)
    out = _check(pkg, src, labels, index[:7], top[:7], left[:7], flip[:7], 4)        # the issue's m = 7
    assert float(out[0, :, :4].abs().max()) == 0.0 and float(out[6, :, -4:].abs().max()) == 0.0
    _check(pkg, src, labels, index, top, left, ~flip, 4)                             # ... and all nine corners, flips swapped


def test_non_square_scalar_width(pkg, gpu):
    src, labels = _split(1, 1, 5, 7, gpu)
    z = torch.zeros(1, dtype=torch.int64, device=gpu)
    for t, l, f in ((0, 4, True), (4, 0, False), (2, 2, True), (1, 3, False)):
        _check(pkg, src, labels, z, z + t, z + l, torch.tensor([f], device=gpu), 2)


def test_null_augmentation_across_workgroups(pkg, gpu):
    src, labels = _split(40, 3, 32, 32, gpu)
    index = torch.randint(0, 40, (130,), generator=torch.Generator().manual_seed(1)).to(gpu)
    out = _check(pkg, src, labels, index, None, None, None, 0)
    assert torch.equal(out, src[index].float() / 255)
    out2, lab2 = pkg.ops.batch_crop_flip(src, index)                                 # no labels either
    assert lab2 is None and torch.equal(out2, out)


def test_all_256_quotients(pkg, gpu):
    src = torch.arange(256, dtype=torch.uint8)[:, None, None, None].expand(256, 1, 4, 4).contiguous().to(gpu)
    labels = torch.arange(256, device=gpu)
    out = _check(pkg, src, labels, torch.arange(256, device=gpu), None, None, None, 0)
    # the device's own quotients: torch divides by a host scalar on the GPU as a multiplication by the fp32 reciprocal, so 126 of these
    # are one ulp off the host's torch.arange(256).float() / 255 — the loader has always produced the device's values
    want = torch.arange(256, device=gpu).float() / 255
    assert torch.equal(want, torch.arange(256, device=gpu).float().div_(255.0))
    assert torch.equal(out[:, 0, 0, 0], want) and torch.equal(out, want[:, None, None, None].expand_as(out))
    host = torch.arange(256).float()
    assert torch.equal(want.cpu(), host * (torch.tensor(1.0) / 255.0))               # = fl(v * fl(1 / 255)), all 256
    off = (want.cpu() != host / 255)
    print(f"byte values whose device quotient differs from the host's correctly rounded v / 255: {int(off.sum())} of 256, "
          f"max {float((want.cpu() - host / 255).abs().max()):.2e}")
    assert float((want.cpu() - host / 255).abs().max()) <= 2.0 ** -24                  # never more than one ulp below 1.0


def test_out_of_range_index_is_clamped(pkg, gpu):
    """A bounds check, not a fault provocation: the kernel clamps the index, so nothing reads outside the split."""
    src, labels = _split(6, 3, 8, 8, gpu)
    bad = torch.tensor([-1, 6, 2, 2 ** 40, -2 ** 40], device=gpu)
    z = torch.zeros(5, dtype=torch.int64, device=gpu)
    out, lab = pkg.ops.batch_crop_flip(src, bad, z + 1, z + 2, z.bool(), labels=labels, pad=1)
    clamped = bad.clamp(0, 5)
    want = _mp()._augment_torch(src[clamped], z + 1, z + 2, z.bool(), 1)
    assert torch.equal(out, want) and torch.equal(lab, labels[clamped])
