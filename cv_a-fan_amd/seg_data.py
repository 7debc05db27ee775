"""The Segmentation data path: a split of variably sized images resident in HBM as uint8, and per batch ONE launch
(ops.seg_batch_aug) that does what the reference's DataLoader workers do per image on PIL (Segmentation/args.py:113-136):

    train:     ExtRandomScale((0.5, 2.0)) -> ExtRandomCrop(crop, pad_if_needed=True) -> ExtRandomHorizontalFlip -> ExtToTensor
    crop_val:  ExtResize(crop) -> ExtCenterCrop(crop) -> ExtToTensor
    otherwise: ExtToTensor, batch 1 at the image's own size

The kernel is a pure function of per-sample parameters (index, resized size, crop origin, flip); SegDeviceLoader draws them on the
host for a whole epoch at once from a seeded generator and uploads them in one pinned, non-blocking copy, so a batch costs one launch
and no host synchronisation.  `_augment_numpy` restates the kernel in plain numpy: it is what the GPU tests hold the kernel to, and
tests/golden/seg_aug_pillow.npz holds it to Pillow's own output, bit for bit.

Cityscapes (args.py:142-151) is ExtRandomCrop -> ExtColorJitter(0.5, 0.5, 0.5) -> flip -> ToTensor: the same loader with
scale_range=(1, 1) and jitter=(0.5, 0.5, 0.5), through ops.seg_batch_aug_jitter; `_jitter_numpy` / `_augment_jitter_numpy` restate it and
tests/golden/seg_jitter_pillow.npz holds the restatement to Pillow's ImageEnhance.
"""
import math
import os

import numpy as np
import torch

from . import ops

KMAX = 8                 # taps per axis the kernel holds: in/out <= MAX_SHRINK
MAX_SHRINK = 3.0
MAX_SIDE = 1 << 15
_PREC = 22               # Pillow's PRECISION_BITS

# ToTensor on the CPU, torch.from_numpy(u8).float().div(255): the correctly rounded fp32 quotient
QUOT255 = np.arange(256, dtype=np.float32) / np.float32(255.0)


# ------------------------------------------------------------------------------------ Pillow's resizes, restated
def _bilinear_coeffs(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter: (xmin [n_out], count [n_out], coef [n_out, KMAX])."""
    x = np.arange(n_out)
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    center = (x + 0.5) * scale
    ss = 1.0 / fs
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = np.clip(xmax - xmin, 0, KMAX)
    k = np.zeros((n_out, KMAX), np.float64)
    ww = np.zeros(n_out, np.float64)
    for u in range(KMAX):                                     # summed left to right
        t = np.abs(((u + xmin) - center + 0.5) * ss)
        w = np.where((u < n) & (t < 1.0), 1.0 - t, 0.0)
        k[:, u] = w
        ww = ww + w
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    kk = k * float(1 << _PREC)
    coef = np.where(k < 0, (-0.5 + kk).astype(np.int64), (0.5 + kk).astype(np.int64))
    coef[np.arange(KMAX)[None, :] >= n[:, None]] = 0
    return xmin, n, coef


def _resample_axis(a, n_out, axis):
    """One pass of Pillow's 8-bit resampler along `axis` of a uint8 array (skipped when the size does not change)."""
    n_in = a.shape[axis]
    if n_in == n_out:
        return a
    xmin, _, coef = _bilinear_coeffs(n_in, n_out)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    acc = np.full((n_out,) + a.shape[1:], 1 << (_PREC - 1), np.int64)
    tail = (1,) * (a.ndim - 1)
    for u in range(KMAX):
        acc += a[np.minimum(xmin + u, n_in - 1)] * coef[:, u].reshape((n_out,) + tail)      # (coef is 0 past the count)
    return np.moveaxis(np.clip(acc >> _PREC, 0, 255).astype(np.uint8), 0, axis)


def _resize_bilinear(img, oh, ow):
    """PIL.Image.resize((ow, oh), BILINEAR) of an HWC (or HW) uint8 array: the horizontal pass, rounded to uint8, then the vertical."""
    return _resample_axis(_resample_axis(img, ow, 1), oh, 0)


def _nearest_table(n_in, n_out):
    """Pillow's nearest source coordinates: the ACCUMULATED xo = a/2, a/2 + a, (a/2 + a) + a, ... truncated (not int((x + 0.5) * a))."""
    a = float(n_in) / float(n_out)
    steps = np.full(n_out, a, np.float64)
    steps[0] = a * 0.5
    return np.minimum(np.add.accumulate(steps).astype(np.int64), n_in - 1)       # (accumulate adds strictly left to right)


def _resize_nearest(lbl, oh, ow):
    return lbl[_nearest_table(lbl.shape[0], oh)][:, _nearest_table(lbl.shape[1], ow)]


# ------------------------------------------------------------------------------------ the kernel, restated
def _clamped(h, w, oh, ow, top, left, out_h, out_w, max_shrink=MAX_SHRINK):
    """The kernel's clamps and its padding: (oh, ow, P, top, left) for a source of h x w."""
    oh = int(min(max(int(oh), max(int(math.ceil(h / max_shrink)), 1)), MAX_SIDE))
    ow = int(min(max(int(ow), max(int(math.ceil(w / max_shrink)), 1)), MAX_SIDE))
    p1 = (1 + out_w - ow) // 2 if ow < out_w else 0           # ext_transforms.py:383-385: all four sides
    p2 = (1 + out_h - (oh + 2 * p1)) // 2 if oh + 2 * p1 < out_h else 0      # :388-390, on the already padded height
    pad = p1 + p2
    top = int(min(max(int(top), 0), oh + 2 * pad - out_h))
    left = int(min(max(int(left), 0), ow + 2 * pad - out_w))
    return oh, ow, pad, top, left


def _augment_numpy(img, lbl, oh, ow, top, left, flip, out_h, out_w, max_shrink=MAX_SHRINK):
    """One sample of ops.seg_batch_aug in numpy.  img: HWC uint8, lbl: HW uint8 -> (fp32 [3, out_h, out_w], int64 [out_h, out_w])."""
    h, w = lbl.shape
    oh, ow, pad, top, left = _clamped(h, w, oh, ow, top, left, out_h, out_w, max_shrink)
    ri = np.pad(_resize_bilinear(img, oh, ow), ((pad, pad), (pad, pad), (0, 0)))           # fill 0 ...
    rl = np.pad(_resize_nearest(lbl, oh, ow), ((pad, pad), (pad, pad)))                    # ... for the label too (background)
    ri, rl = ri[top:top + out_h, left:left + out_w], rl[top:top + out_h, left:left + out_w]
    if flip:
        ri, rl = ri[:, ::-1], rl[:, ::-1]
    return np.ascontiguousarray(QUOT255[ri].transpose(2, 0, 1)), np.ascontiguousarray(rl.astype(np.int64))


def _augment_numpy_batch(images, labels, index, oh, ow, top, left, flip, out_h, out_w, max_shrink=MAX_SHRINK):
    n = len(images)
    outs = [_augment_numpy(images[min(max(int(k), 0), n - 1)], labels[min(max(int(k), 0), n - 1)], a, b, t, l, f, out_h, out_w,
                           max_shrink) for k, a, b, t, l, f in zip(index, oh, ow, top, left, flip)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# ------------------------------------------------------------------------------------ ExtColorJitter, restated
# ExtColorJitter(brightness, contrast, saturation) is torchvision's PIL functional: PIL.ImageEnhance.{Brightness, Contrast, Color}
# (img).enhance(f) = Image.blend(degenerate, img, f), in a shuffled order, each on the uint8 output of the one before.
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
# the order code the kernel takes: the permutations of (brightness, contrast, saturation) in lexicographic order
JITTER_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def _gray(img):
    """Pillow's RGB -> L on an HWC uint8 array, in integers."""
    a = img.astype(np.int64)
    return (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16


def _blend(d, img, f):
    """Image.blend(degenerate, image, f) on uint8 values: fp32, the product and the sum rounded separately (numpy does not fuse)."""
    f32 = np.float32(f)
    d32 = np.asarray(d).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = d32 + f32 * (img.astype(np.float32) - d32)
        t = np.broadcast_to(t, img.shape)
        if np.float32(0) <= f32 <= np.float32(1):
            return t.astype(np.uint8)                                 # between d and the pixel: truncated
        out = np.where(t >= np.float32(255), np.float32(255), t)
        out = np.where(out > np.float32(0), out, np.float32(0))       # t <= 0 (and what is not a number) -> 0
        return out.astype(np.uint8)


def _jitter_numpy(img_u8, order, factors):
    """The three operations on an HWC uint8 image.  order: code into JITTER_ORDERS (clamped into 0..5, as the kernel clamps it);
    factors: (brightness, contrast, saturation), by operation — not by position in the order."""
    img = np.ascontiguousarray(img_u8)
    for op in JITTER_ORDERS[min(max(int(order), 0), 5)]:
        f = factors[op]
        if op == BRIGHTNESS:
            d = np.zeros((), np.int64)
        elif op == CONTRAST:
            g = _gray(img)                                            # ImageStat.Stat(img.convert("L")).mean[0], int(mean + 0.5)
            d = np.array(int(int(g.sum()) / g.size + 0.5), np.int64)
        else:
            d = _gray(img)[..., None]                                 # img.convert("L").convert("RGB")
        img = _blend(d, img, f)
    return img


def _augment_jitter_numpy(img, lbl, oh, ow, top, left, flip, order, factors, out_h, out_w, max_shrink=MAX_SHRINK):
    """One sample of ops.seg_batch_aug_jitter in numpy: _augment_numpy with the jitter between the crop and the flip (the padding's
    pixels count in contrast's mean and are jittered, as Pillow would do)."""
    h, w = lbl.shape
    oh, ow, pad, top, left = _clamped(h, w, oh, ow, top, left, out_h, out_w, max_shrink)
    ri = np.pad(_resize_bilinear(img, oh, ow), ((pad, pad), (pad, pad), (0, 0)))
    rl = np.pad(_resize_nearest(lbl, oh, ow), ((pad, pad), (pad, pad)))
    ri, rl = ri[top:top + out_h, left:left + out_w], rl[top:top + out_h, left:left + out_w]
    ri = _jitter_numpy(ri, order, factors)
    if flip:
        ri, rl = ri[:, ::-1], rl[:, ::-1]
    return np.ascontiguousarray(QUOT255[ri].transpose(2, 0, 1)), np.ascontiguousarray(rl.astype(np.int64))


def _augment_jitter_numpy_batch(images, labels, index, oh, ow, top, left, flip, order, factors, out_h, out_w, max_shrink=MAX_SHRINK):
    """factors: [3, m] (rows: brightness, contrast, saturation)."""
    n = len(images)
    fac = np.asarray(factors)
    outs = [_augment_jitter_numpy(images[min(max(int(k), 0), n - 1)], labels[min(max(int(k), 0), n - 1)], a, b, t, l, f, o, fac[:, i],
                                  out_h, out_w, max_shrink)
            for i, (k, a, b, t, l, f, o) in enumerate(zip(index, oh, ow, top, left, flip, order))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# ------------------------------------------------------------------------------------ parameters of the reference's transforms
def val_resize_size(h, w, size):
    """ExtResize(size) with an int: the shorter side becomes `size` (torchvision's F.resize)."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def center_crop_origin(h, w, th, tw):
    """ExtCenterCrop: F.center_crop's int(round((h - th) / 2.)) (Python's round: half to even)."""
    return int(round((h - th) / 2.)), int(round((w - tw) / 2.))


def pack_split(images, labels):
    """Lists of HWC uint8 images and HW uint8 labels -> (packed images, packed labels, byte offsets int64, hs int32, ws int32)."""
    if len(images) != len(labels) or not images:
        raise ValueError("a split needs as many labels as images, and at least one")
    hs = np.array([l.shape[0] for l in labels], np.int32)
    ws = np.array([l.shape[1] for l in labels], np.int32)
    for im, lb in zip(images, labels):
        if im.dtype != np.uint8 or lb.dtype != np.uint8 or im.shape != lb.shape + (3,):
            raise ValueError("images are HWC uint8 with 3 channels, labels HW uint8 of the same size")
    pix = hs.astype(np.int64) * ws.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(pix)[:-1]]).astype(np.int64) * 3
    return (np.concatenate([im.reshape(-1) for im in images]), np.concatenate([lb.reshape(-1) for lb in labels]), off, hs, ws)


class SegDeviceLoader:
    """The whole split resident in HBM as packed uint8 (VOC 2012 train-aug: about 6 GB of 288 GB), uploaded once.  Per epoch the
    permutation, scales, crop origins and flips are drawn on the host from one generator (seeded with (seed, epoch): every rank
    draws the same and takes its slice) and uploaded in one pinned non-blocking copy; per batch there is exactly one launch and no
    host synchronisation.  train=False gives the reference's validation transforms through the same kernel: crop_val (ExtResize +
    ExtCenterCrop at crop_size, in batches) or the images as they are, one per batch.

    jitter=(b, c, s) (training only) adds the reference's ExtColorJitter(brightness=b, contrast=c, saturation=s) between the crop and
    the flip (ops.seg_batch_aug_jitter): per sample and epoch an order of the three operations and three factors uniform in
    [max(0, 1 - v), 1 + v], drawn AFTER the other draws from the same generator, so a loader without jitter draws what it always drew.
    scale_range=(1, 1) is the Cityscapes transform: ExtRandomCrop without ExtRandomScale and without pad_if_needed — an image smaller
    than the crop is refused at construction (the reference's random.randint(0, h - th) raises there)."""

    def __init__(self, images, labels, batch, device, train, crop_size, crop_val=False, scale_range=(0.5, 2.0), seed=None, rank=0,
                 world=1, jitter=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ops.AfanLibraryError("SegDeviceLoader needs an MI355X: the batch is built by a HIP kernel and there is no CPU path")
        img, lab, off, hs, ws = pack_split(images, labels)
        self.n = len(hs)
        self.hs, self.ws = hs.astype(np.int64), ws.astype(np.int64)
        self.train, self.crop_val, self.crop = bool(train), bool(crop_val), int(crop_size)
        self.scale_range = (float(scale_range[0]), float(scale_range[1]))
        self.jitter = None
        if jitter is not None and self.train:
            self.jitter = tuple(float(v) for v in jitter)
            if len(self.jitter) != 3 or not all(math.isfinite(v) and v >= 0 for v in self.jitter):
                raise ValueError("jitter takes (brightness, contrast, saturation), three finite values >= 0")
        if self.train and self.scale_range == (1.0, 1.0) and (int(hs.min()) < self.crop or int(ws.min()) < self.crop):
            raise ValueError(f"scale_range=(1, 1) crops without padding: an image of {int(hs.min())} x {int(ws.min())} (smallest height x "
                             f"smallest width) is smaller than the crop of {self.crop}")
        self.rank, self.world, self.seed, self.epoch = int(rank), int(world), seed, 0
        if world > 1 and seed is None:
            raise RuntimeError("a data-parallel SegDeviceLoader needs a seed shared by all ranks")
        if self.train or self.crop_val:
            self.batch = int(batch)
        else:
            self.batch = 1                                    # native sizes differ: main_aug_final.py:50-51
        if self.batch % self.world:
            raise ValueError("the batch must divide among the ranks")
        self.n_batches = self.n // self.batch if self.train else (self.n + self.batch - 1) // self.batch
        # the bound on in/out the kernel is told (it clamps beyond): the smallest size a draw can ask for
        if self.train:
            lo_h = np.maximum((self.hs * self.scale_range[0]).astype(np.int64), 1)
            lo_w = np.maximum((self.ws * self.scale_range[0]).astype(np.int64), 1)
        elif self.crop_val:
            lo = np.array([val_resize_size(int(h), int(w), self.crop) for h, w in zip(self.hs, self.ws)], np.int64)
            lo_h, lo_w = lo[:, 0], lo[:, 1]
        else:
            lo_h, lo_w = self.hs, self.ws
        shrink = max(float((self.hs / lo_h).max()), float((self.ws / lo_w).max()), 1.0)
        if shrink > MAX_SHRINK:
            raise ValueError(f"the split asks for a reduction by {shrink:.3f} > {MAX_SHRINK}: more taps than the kernel holds (KMAX = {KMAX})")
        self.max_shrink = shrink
        dev = self.device
        self.images = torch.from_numpy(img).to(dev)
        self.labels = torch.from_numpy(lab).to(dev)
        self.offsets = torch.from_numpy(off).to(dev)
        self.d_hs = torch.from_numpy(hs).to(dev)
        self.d_ws = torch.from_numpy(ws).to(dev)
        self._gray_sums = self._jitter_draw = None

    def __len__(self):
        return self.n_batches

    def _draw(self):
        """The epoch's parameters, int64 [6, n_used]: index, oh, ow, top, left, flip — and the per-batch output sizes."""
        if self.train:
            rng = np.random.default_rng(None if self.seed is None else [int(self.seed), self.epoch])
            self.epoch += 1
            idx = rng.permutation(self.n)[:self.n_batches * self.batch]
            h, w = self.hs[idx], self.ws[idx]
            scale = rng.uniform(self.scale_range[0], self.scale_range[1], idx.shape[0])
            oh = np.maximum((h * scale).astype(np.int64), 1)          # ExtRandomScale: int(size * scale), in float64
            ow = np.maximum((w * scale).astype(np.int64), 1)
            p1 = np.where(ow < self.crop, (1 + self.crop - ow) // 2, 0)
            p2 = np.where(oh + 2 * p1 < self.crop, (1 + self.crop - (oh + 2 * p1)) // 2, 0)
            pad = p1 + p2
            top = rng.integers(0, oh + 2 * pad - self.crop + 1)         # ExtRandomCrop.get_params: randint(0, h - th), inclusive
            left = rng.integers(0, ow + 2 * pad - self.crop + 1)
            flip = (rng.random(idx.shape[0]) < 0.5).astype(np.int64)
            sizes = [(self.crop, self.crop)] * self.n_batches
            self._jitter_draw = None
            if self.jitter is not None:                               # ExtColorJitter.get_params: three factors, then the shuffle
                fac = np.stack([rng.uniform(max(0.0, 1.0 - v), 1.0 + v, idx.shape[0]) for v in self.jitter])
                self._jitter_draw = (rng.integers(0, 6, idx.shape[0]).astype(np.int64), ops.jitter_factors(fac))
        elif self.crop_val:
            idx = np.arange(self.n)
            s = np.array([val_resize_size(int(h), int(w), self.crop) for h, w in zip(self.hs, self.ws)], np.int64)
            oh, ow = s[:, 0], s[:, 1]
            o = np.array([center_crop_origin(int(a), int(b), self.crop, self.crop) for a, b in s], np.int64)
            top, left, flip = o[:, 0], o[:, 1], np.zeros(self.n, np.int64)
            sizes = [(self.crop, self.crop)] * self.n_batches
        else:
            idx = np.arange(self.n)
            oh, ow = self.hs, self.ws
            top = left = flip = np.zeros(self.n, np.int64)
            sizes = [(int(h), int(w)) for h, w in zip(self.hs, self.ws)]
        return np.stack([idx, oh, ow, top, left, flip]).astype(np.int64), sizes

    def __iter__(self):
        params, sizes = self._draw()
        self.last_params = params                                       # (host copy: what tests compare the batches against)
        dev_params = torch.from_numpy(params).pin_memory().to(self.device, non_blocking=True)       # one upload per epoch
        jit = self._jitter_draw if self.train else None
        self.last_jitter = jit                                          # (order int64 [n_used], factors fp32 [3, n_used]) or None
        if jit is not None:
            dev_order = torch.from_numpy(jit[0]).pin_memory().to(self.device, non_blocking=True)
            dev_fac = torch.from_numpy(jit[1]).pin_memory().to(self.device, non_blocking=True)
            if self._gray_sums is None:
                self._gray_sums = torch.empty(max(self.batch // self.world, 1), dtype=torch.int64, device=self.device)
        per = self.batch // self.world
        for b in range(self.n_batches):
            lo = b * self.batch + self.rank * per
            hi = min(lo + per, params.shape[1])
            if hi <= lo:
                continue
            p = dev_params[:, lo:hi]
            if jit is not None:
                f = dev_fac[:, lo:hi]
                yield ops.seg_batch_aug_jitter(self.images, self.offsets, self.labels, self.d_hs, self.d_ws, p[0], p[1], p[2], p[3], p[4],
                                               p[5], dev_order[lo:hi], f[0], f[1], f[2], sizes[b][0], sizes[b][1], self.max_shrink,
                                               workspace=self._gray_sums)
                continue
            yield ops.seg_batch_aug(self.images, self.offsets, self.labels, self.d_hs, self.d_ws, p[0], p[1], p[2], p[3], p[4], p[5],
                                    sizes[b][0], sizes[b][1], self.max_shrink)


# ------------------------------------------------------------------------------------ where a split comes from
_VOC_BASE = {"2012": "VOCdevkit/VOC2012", "2012_aug": "VOCdevkit/VOC2012", "2011": "TrainVal/VOCdevkit/VOC2011",
             "2009": "VOCdevkit/VOC2009", "2008": "VOCdevkit/VOC2008", "2007": "VOCdevkit/VOC2007"}


def load_voc(root, year="2012", image_set="train"):
    """datasets/voc.py:104-146: JPEGImages / SegmentationClass(Aug) of the image set, decoded ONCE on the host with Pillow into
    (list of HWC uint8, list of HW uint8).  There is no download here."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("load_voc decodes JPEG / PNG files with Pillow, which is not installed; --synthetic N needs no files") from e
    voc_root = os.path.join(root, _VOC_BASE[year])
    if year == "2012_aug" and image_set == "train":
        mask_dir, split_f = os.path.join(voc_root, "SegmentationClassAug"), os.path.join(root, "train_aug.txt")
    else:
        mask_dir = os.path.join(voc_root, "SegmentationClass")
        split_f = os.path.join(voc_root, "ImageSets", "Segmentation", image_set + ".txt")
    if not os.path.isdir(voc_root) or not os.path.exists(split_f) or not os.path.isdir(mask_dir):
        raise FileNotFoundError(f"VOC {year} '{image_set}' not found under {root} (expected {split_f} and {mask_dir}); "
                                "there is no download in this build")
    with open(split_f) as f:
        names = [x.strip() for x in f if x.strip()]
    images, labels = [], []
    for x in names:
        images.append(np.asarray(Image.open(os.path.join(voc_root, "JPEGImages", x + ".jpg")).convert("RGB"), dtype=np.uint8))
        labels.append(np.asarray(Image.open(os.path.join(mask_dir, x + ".png")), dtype=np.uint8))
    return images, labels


# datasets/cityscapes.py:25-66: id_to_train_id, the 35 entries (ids 0..33 and the license plate's -1, which numpy indexing puts last)
CITYSCAPES_TRAIN_IDS = (255, 255, 255, 255, 255, 255, 255, 0, 1, 255, 255, 2, 3, 4, 255, 255, 255, 5, 255, 6, 7, 8, 9, 10, 11, 12, 13, 14,
                        15, 255, 255, 16, 17, 18, 255)


def _train_id_table():
    """256 entries: label id -> train id; ids past the reference's 35 map to -1 here and are refused by load_cityscapes."""
    t = np.full(256, -1, np.int16)
    t[:len(CITYSCAPES_TRAIN_IDS)] = CITYSCAPES_TRAIN_IDS
    return t


def encode_cityscapes(label_ids):
    """Cityscapes.encode_target on an HW uint8 array of label ids -> HW uint8 train ids (0..18, 255 = ignore).  An id of 35 or more
    raises ValueError (the reference's table lookup raises IndexError there)."""
    out = _train_id_table()[np.asarray(label_ids, dtype=np.uint8)]
    if (out < 0).any():
        raise ValueError(f"a Cityscapes label id of {int(np.asarray(label_ids)[out < 0].max())}: the table has {len(CITYSCAPES_TRAIN_IDS)} ids")
    return out.astype(np.uint8)


def load_cityscapes(root, split="train"):
    """datasets/cityscapes.py:73-102: leftImg8bit/<split>/<city>/*_leftImg8bit.png with gtFine/<split>/<city>/*_gtFine_labelIds.png,
    decoded ONCE on the host with Pillow into (list of HWC uint8, list of HW uint8).  Cities and files are read in SORTED order (the
    reference takes os.listdir's, which is the file system's).  id_to_train_id is applied here, through a 256-entry table, so the
    resident labels are train ids: the mapping is pointwise and commutes with the crop and the flip, which the reference applies first.
    There is no download here."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("load_cityscapes decodes PNG files with Pillow, which is not installed; --synthetic N needs no files") from e
    if split not in ("train", "test", "val"):
        raise ValueError('Invalid split! Please use split="train", split="test" or split="val"')
    images_dir, targets_dir = os.path.join(root, "leftImg8bit", split), os.path.join(root, "gtFine", split)
    if not os.path.isdir(images_dir) or not os.path.isdir(targets_dir):
        raise FileNotFoundError(f"Cityscapes '{split}' not found under {root} (expected {images_dir} and {targets_dir}); "
                                "there is no download in this build")
    images, labels = [], []
    for city in sorted(os.listdir(images_dir)):
        img_dir = os.path.join(images_dir, city)
        if not os.path.isdir(img_dir):
            continue
        for name in sorted(os.listdir(img_dir)):
            if not name.endswith("_leftImg8bit.png"):
                continue
            target = os.path.join(targets_dir, city, name.split("_leftImg8bit")[0] + "_gtFine_labelIds.png")
            images.append(np.asarray(Image.open(os.path.join(img_dir, name)).convert("RGB"), dtype=np.uint8))
            labels.append(encode_cityscapes(np.asarray(Image.open(target), dtype=np.uint8)))
    if not images:
        raise FileNotFoundError(f"Cityscapes '{split}' under {root} holds no *_leftImg8bit.png; there is no download in this build")
    return images, labels


class SyntheticSegSplit:
    """A split for machines without the data: n images of random sizes in [min_side, max_side], labels in blocks of 8 x 8 pixels
    over `classes` classes with a sprinkling of 255 (the ignore index)."""

    def __init__(self, n, seed=0, min_side=96, max_side=160, classes=21):
        rng = np.random.default_rng(seed)
        self.num_classes = classes
        self.images, self.labels = [], []
        for _ in range(n):
            h, w = (int(v) for v in rng.integers(min_side, max_side + 1, 2))
            self.images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            blocks = rng.integers(0, classes, ((h + 7) // 8, (w + 7) // 8), dtype=np.uint8)
            lab = np.kron(blocks, np.ones((8, 8), np.uint8))[:h, :w].copy()
            lab[rng.random((h, w)) < 0.02] = 255
            self.labels.append(lab)

    def __len__(self):
        return len(self.images)
