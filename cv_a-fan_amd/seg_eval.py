"""Segmentation validation: StreamSegMetrics (Segmentation/metrics/stream_metrics.py:25-83), validate (Segmentation/args.py:168-220)
and pgd_validate (args.py:223-255: the same pass on images attacked in image space) with the reference's interfaces.

What differs is where the counting happens.  The reference resizes the logits to the image size, takes max(dim=1), copies the
predictions and the labels to the host and counts there (np.bincount), once per batch.  Here `update_logits` hands the classifier's
LOW-resolution logits and the labels to one launch (ops.seg_confusion_upsampled: resize, arg-max and the confusion matrix, added into
an int64 matrix on the device) and nothing is read back before `get_results()`.  `update` (predictions as arrays or tensors, the
reference's signature) is kept for callers that have predictions; it is plain numpy.  The formulas of `get_results` are the
reference's, in numpy float64 on the same float64 matrix."""
import numpy as np
import torch

from . import deeplab, ops, seg_attack_algo


def _fast_hist(n_classes, label_true, label_pred):
    """stream_metrics.py:49-55 on flat integer arrays: labels outside [0, n_classes) are left out."""
    mask = (label_true >= 0) & (label_true < n_classes)
    return np.bincount(n_classes * label_true[mask].astype(int) + label_pred[mask],
                       minlength=n_classes ** 2).reshape(n_classes, n_classes)


def _numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class StreamSegMetrics:
    """Stream metrics for semantic segmentation.  The matrix is the sum of a host part (`update`) and a device part
    (`update_logits`; created on the first call, on `device` or the logits' own); `confusion_matrix` reads both."""

    def __init__(self, n_classes, device=None):
        self.n_classes = int(n_classes)
        self.device = None if device is None else torch.device(device)
        self._host = np.zeros((self.n_classes, self.n_classes), np.int64)
        self._dev = None

    # ---- the reference's update: predictions
    def update(self, label_trues, label_preds):
        for lt, lp in zip(label_trues, label_preds):
            self._host += _fast_hist(self.n_classes, _numpy(lt).flatten(), _numpy(lp).flatten())

    # ---- the hot path: logits
    def update_logits(self, out, targets):
        """`out`: what model(input_dict) returned — a deeplab.LowResLogits or a logits tensor [N,C,h,w]; targets [N,H,W] integer
        labels.  fp32 GPU logits of up to 32 classes (and n_classes of them) are scored in one launch, up-scaling included;
        other GPU logits are resized first (deeplab.interpolate) and scored by the same launch at equal sizes; anything the
        kernel does not take (CPU tensors, more than 32 classes, down-scaling) goes through torch's max(dim=1) and `update`."""
        if isinstance(out, deeplab.LowResLogits):
            logits, size = out.logits, out.size
        else:
            logits, size = out, tuple(int(v) for v in targets.shape[-2:])
        logits = logits.detach()
        if tuple(targets.shape[-2:]) != tuple(size) or targets.shape[0] != logits.shape[0]:
            raise ValueError(f"update_logits: labels {tuple(targets.shape)} do not match logits resized to {tuple(size)}")
        c = logits.shape[1]
        kernel = (logits.is_cuda and targets.is_cuda and c == self.n_classes and c <= ops.CE2D_MAX_CLASSES
                  and not torch.is_floating_point(targets))
        if kernel and (logits.dtype != torch.float32 or logits.shape[2] > size[0] or logits.shape[3] > size[1]):
            logits = deeplab.interpolate(logits, size).float()
        if not kernel:
            full = logits if tuple(logits.shape[2:]) == tuple(size) else deeplab.interpolate(logits, size)
            return self.update(targets.cpu().numpy(), full.max(dim=1)[1].cpu().numpy())
        if self._dev is None:
            self._dev = torch.zeros(c * c, dtype=torch.int64, device=self.device or logits.device)
        ops.seg_confusion_upsampled(logits, targets.to(torch.int64), self._dev)

    @property
    def confusion_matrix(self):
        """float64 [n_classes, n_classes], rows = labels, columns = predictions (one read-back when logits were scored)."""
        m = self._host
        if self._dev is not None:
            m = m + self._dev.cpu().numpy().reshape(self.n_classes, self.n_classes)
        return m.astype(np.float64)

    def get_results(self):
        """stream_metrics.py:57-80: overall accuracy, mean accuracy, frequency-weighted accuracy, mean IoU, per-class IoU.
        Classes absent from labels and predictions are NaN and left out of the means (nanmean); no warning is raised."""
        hist = self.confusion_matrix
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.diag(hist).sum() / hist.sum()
            acc_cls = np.diag(hist) / hist.sum(axis=1)
            acc_cls = np.nanmean(acc_cls)
            iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
            mean_iu = np.nanmean(iu)
            freq = hist.sum(axis=1) / hist.sum()
            fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
        cls_iu = dict(zip(range(self.n_classes), iu))
        return {"Overall Acc": acc, "Mean Acc": acc_cls, "FreqW Acc": fwavacc, "Mean IoU": mean_iu, "Class IoU": cls_iu}

    @staticmethod
    def to_str(results):
        string = "\n"
        for k, v in results.items():
            if k != "Class IoU":
                string += "%s: %f\n" % (k, v)
        return string

    def reset(self):
        self._host = np.zeros((self.n_classes, self.n_classes), np.int64)
        if self._dev is not None:
            self._dev.zero_()


def validate(opts, model, loader, device, metrics, ret_samples_ids=None):
    """args.py:168-220: one pass over `loader`, (score, ret_samples).  The caller sets model.eval() / model.train().  Per batch: one
    forward that stops at the classifier's low-resolution logits and one scoring launch; the only read-back is get_results()'s.
    ret_samples is [] (no visdom in this build: ret_samples_ids is accepted and ignored)."""
    if getattr(opts, "save_val_results", False):
        raise NotImplementedError("--save_val_results: writing the validation images is not built (validation itself is)")
    metrics.reset()
    ret_samples = []
    with torch.no_grad():
        for images, labels in loader:
            images, labels = images.to(device), labels.to(device)
            out = model({"x": images, "adv": None, "out_idx": 0, "flag": "clean", "low_res": True})
            metrics.update_logits(out, labels)
        score = metrics.get_results()
    return score, ret_samples


def pgd_validate(opts, model, loader, device, metrics, criterion, ret_samples_ids=None):
    """args.py:223-255: one pass over `loader` with every batch attacked by image-space sign-PGD first (seg_attack_algo.adv_input with
    opts.steps_pgd / eps_pgd / gamma_pgd / randinit_pgd / clip_pgd, eps and gamma in 1/255 units), (score, ret_samples).  The caller
    sets model.eval().  Per batch: steps_pgd forward + input-gradient passes (no parameter gradient is computed: adv_input runs them
    under dgrad_only), then one forward under no_grad on the adversarial images that stops at the classifier's low-resolution
    logits and one scoring launch, as validate().  Nothing is read back before get_results() — except that --randinit_pgd draws
    its start on the host, as the reference does.  steps_pgd = 0 scores what validate() scores.  ret_samples is []."""
    metrics.reset()
    ret_samples = []
    criterion = deeplab.seg_criterion(criterion)
    for images, labels in loader:
        images, labels = images.to(device), labels.to(device)
        adv_images = seg_attack_algo.adv_input(x=images, criterion=criterion, y=labels, model=model, steps=opts.steps_pgd,
                                               eps=(opts.eps_pgd / 255), gamma=(opts.gamma_pgd / 255), randinit=opts.randinit_pgd,
                                               clip=opts.clip_pgd)
        with torch.no_grad():
            out = model({"x": adv_images.detach(), "adv": None, "out_idx": 0, "flag": "clean", "low_res": True})
            metrics.update_logits(out, labels)
    score = metrics.get_results()
    return score, ret_samples
