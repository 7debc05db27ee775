"""The definition of afan_seg_confusion_upsampled (csrc/afan_seg_eval.hip) restated in float64, from the definitions: bilinear resize
with align_corners=False (the per-axis matrices of tests/seg_pinned_refs.py), arg-max over the classes with torch.max(dim=1)'s rule
(the lowest class among equal maxima; a NaN is the maximum and the first NaN wins), and the masked count of
Segmentation/metrics/stream_metrics.py:49-55 (labels outside [0, C) are skipped).  tests/test_seg_metrics.py checks it against torch
on the CPU; the reference formulas of the scores are restated here too.  Nothing here reads the kernel or ops.py."""
import numpy as np
import torch

import seg_pinned_refs as R


def resize(logits, ho, wo):
    """logits [N, C, h, w] (numpy or torch, any float type) -> float64 numpy [N, C, ho, wo]."""
    x = torch.as_tensor(np.asarray(logits, dtype=np.float64))
    wy, wx = torch.from_numpy(R.axis_matrix(x.shape[2], ho)), torch.from_numpy(R.axis_matrix(x.shape[3], wo))
    return torch.einsum("oi,ncij,pj->ncop", wy, x, wx).numpy()


def argmax_first(x):
    """x [N, C, H, W] -> int64 [N, H, W]: classes scanned in increasing order; a value replaces the running maximum when it is
    greater or NaN, unless the running maximum is already NaN."""
    best, arg = x[:, 0].copy(), np.zeros(x[:, 0].shape, np.int64)
    for c in range(1, x.shape[1]):
        v = x[:, c]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(best) & ((v > best) | np.isnan(v))
        best, arg = np.where(take, v, best), np.where(take, c, arg)
    return arg


def fast_hist(n_classes, target, pred):
    """int64 [C, C]: rows = labels, columns = predictions, over the pixels with 0 <= label < C."""
    t, p = np.asarray(target).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    m = (t >= 0) & (t < n_classes)
    return np.bincount(n_classes * t[m] + p[m], minlength=n_classes ** 2).reshape(n_classes, n_classes)


def confusion_upsampled(logits, target):
    """The kernel's definition: logits [N, C, h, w], target [N, H, W] -> int64 [C, C]."""
    target = np.asarray(target)
    return fast_hist(logits.shape[1], target, argmax_first(resize(logits, target.shape[1], target.shape[2])))


def scores(hist):
    """stream_metrics.py:64-72 on a float64 matrix: (overall acc, mean acc, freq-weighted acc, mean IoU, class IoUs)."""
    hist = np.asarray(hist, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        mean_iu = np.nanmean(iu)
        freq = hist.sum(axis=1) / hist.sum()
        fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
    return acc, acc_cls, fwavacc, mean_iu, iu
