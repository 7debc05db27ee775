"""The Detection data path: a split of variably sized images and their ground-truth boxes resident in HBM, and per batch ONE launch
(ops.det_batch_resize) that does what the reference's eight DataLoader workers do per image on PIL (Detection/dataset/voc2007.py:95-116,
dataset/base.py:75-124):

    ImageOps.mirror + `image.width - bboxes[:, [2, 0]]` (probability one half, training only)
    -> Base.preprocess: Resize((round(h * scale), round(w * scale))) with min side 600 / max side 1000 -> ToTensor, `bboxes *= scale`
    -> padding_collate_fn: F.pad right and below to the batch's largest image, zero rows up to its largest box count

The kernel is a pure function of per-sample parameters (index, resized size, flip, scale); DetDeviceLoader draws them on the host
for a whole epoch at once from a seeded generator and uploads them in one pinned, non-blocking copy, so a batch costs one launch and
no host synchronisation.  `_det_batch_numpy` restates the kernel in plain numpy on top of seg_data._resize_bilinear: it is what the
GPU tests hold the kernel to, and tests/golden/det_data_pillow.npz holds it to Pillow's and torch's own output, bit for bit.
"""
import math
import os

import numpy as np
import torch

from . import ops
from .seg_data import KMAX, MAX_SHRINK, MAX_SIDE, QUOT255, _resize_bilinear

# dataset/voc2007.py:35-41
CATEGORY_TO_LABEL_DICT = {
    'background': 0,
    'aeroplane': 1, 'bicycle': 2, 'bird': 3, 'boat': 4, 'bottle': 5,
    'bus': 6, 'car': 7, 'cat': 8, 'chair': 9, 'cow': 10,
    'diningtable': 11, 'dog': 12, 'horse': 13, 'motorbike': 14, 'person': 15,
    'pottedplant': 16, 'sheep': 17, 'sofa': 18, 'train': 19, 'tvmonitor': 20
}
DATASETS = ("voc2007", "voc20072012")


# ------------------------------------------------------------------------------------ the reference's parameters
def preprocess_size(h, w, min_side, max_side):
    """Base.preprocess (dataset/base.py:75-85) in double arithmetic with Python's round: the shorter side is scaled to min_side; if the
    longer side then exceeds max_side, it is scaled to max_side instead -> (oh, ow, scale)."""
    scale_for_shorter_side = min_side / min(w, h)
    longer_side_after_scaling = max(w, h) * scale_for_shorter_side
    scale_for_longer_side = (max_side / longer_side_after_scaling) if longer_side_after_scaling > max_side else 1
    scale = scale_for_shorter_side * scale_for_longer_side
    return round(h * scale), round(w * scale), scale


def ratio_batches(ratios, batch, rng):
    """The reference's NearestRatioRandomSampler (dataset/base.py:126-158) -> int64 [n_batches, batch]: tall (w / h < 1) and fat
    indices are shuffled separately, each group is cut to a multiple of `batch` (the remainders are dropped), formed into groups of
    `batch`, tall groups first, and the groups are shuffled.  The three permutations come from `rng`, a numpy generator, in that order
    (tall, fat, groups): the stream is the project's, not torch.randperm's, so an epoch's order differs from the reference's for the
    same seed while its distribution is the same."""
    ratios = np.asarray(ratios, dtype=np.float64)
    batch = int(batch)
    tall = np.nonzero(ratios < 1)[0]
    fat = np.nonzero(ratios >= 1)[0]
    tall = tall[rng.permutation(len(tall))]
    fat = fat[rng.permutation(len(fat))]
    tall = tall[:len(tall) - len(tall) % batch].reshape(-1, batch)
    fat = fat[:len(fat) - len(fat) % batch].reshape(-1, batch)
    merged = np.concatenate([tall, fat], axis=0)
    return merged[rng.permutation(len(merged))].astype(np.int64)


# ------------------------------------------------------------------------------------ the kernel, restated
def _det_sample_numpy(img, boxes, classes, oh, ow, flip, scale, out_h, out_w, g_max, max_shrink=MAX_SHRINK):
    """One sample of ops.det_batch_resize in numpy.  img: HWC uint8, boxes: fp32 [g, 4], classes: int64 [g] ->
    (fp32 [3, out_h, out_w], fp32 [g_max, 4], int64 [g_max])."""
    h, w = img.shape[:2]
    oh = int(min(max(int(oh), max(int(math.ceil(h / max_shrink)), 1)), MAX_SIDE))
    ow = int(min(max(int(ow), max(int(math.ceil(w / max_shrink)), 1)), MAX_SIDE))
    src = img[:, ::-1] if flip else img                       # ImageOps.mirror: BEFORE the horizontal pass
    r = _resize_bilinear(np.ascontiguousarray(src), oh, ow)[:out_h, :out_w]
    plane = np.zeros((out_h, out_w, 3), np.uint8)             # F.pad: to the right and below
    plane[:r.shape[0], :r.shape[1]] = r
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)[:g_max].copy()
    if flip:
        wf = np.float32(w)
        b[:, [0, 2]] = wf - b[:, [2, 0]]                      # image.width - bboxes[:, [2, 0]], in fp32
    b = b * np.float32(scale)                                 # bboxes *= scale (numpy does not fuse)
    bo = np.zeros((g_max, 4), np.float32)
    lo = np.zeros(g_max, np.int64)
    bo[:len(b)] = b
    lo[:len(b)] = np.asarray(classes, dtype=np.int64)[:g_max]
    return np.ascontiguousarray(QUOT255[plane].transpose(2, 0, 1)), bo, lo


def _det_batch_numpy(images, boxes, classes, index, oh, ow, flip, scale, out_h, out_w, g_max, max_shrink=MAX_SHRINK):
    """ops.det_batch_resize in numpy: images / boxes / classes are per-image lists, the rest one entry per sample."""
    n = len(images)
    ks = [min(max(int(k), 0), n - 1) for k in index]
    outs = [_det_sample_numpy(images[k], boxes[k], classes[k], a, b, f, s, out_h, out_w, g_max, max_shrink)
            for k, a, b, f, s in zip(ks, oh, ow, flip, scale)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs])


def pack_det_split(images, boxes, classes):
    """Lists of HWC uint8 images, fp32 [g, 4] boxes and int64 [g] classes -> (packed images, byte offsets int64, hs int32, ws int32,
    boxes fp32 [total, 4], classes int64 [total], box_off int64 [n + 1]); the image layout is seg_data.pack_split's."""
    if not images:
        raise ValueError("an empty split: there is nothing to build a batch from")
    if len(boxes) != len(images) or len(classes) != len(images):
        raise ValueError("a split needs one array of boxes and one of classes per image")
    for im in images:
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("images are HWC uint8 with 3 channels")
    bs = [np.asarray(b, dtype=np.float32).reshape(-1, 4) for b in boxes]
    cs = [np.asarray(c, dtype=np.int64).reshape(-1) for c in classes]
    if any(len(b) != len(c) for b, c in zip(bs, cs)):
        raise ValueError("every box needs a class")
    hs = np.array([im.shape[0] for im in images], np.int32)
    ws = np.array([im.shape[1] for im in images], np.int32)
    pix = hs.astype(np.int64) * ws.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(pix)[:-1]]).astype(np.int64) * 3
    box_off = np.concatenate([[0], np.cumsum([len(b) for b in bs])]).astype(np.int64)
    return (np.concatenate([im.reshape(-1) for im in images]), off, hs, ws, np.concatenate(bs).reshape(-1, 4),
            np.concatenate(cs), box_off)


class DetDeviceLoader:
    """The whole split resident in HBM as packed uint8 with its boxes (VOC 2007 trainval: about 2.7 GB of 288 GB), uploaded once.  Per
    epoch the batches (ratio_batches) and the flips (probability one half) are drawn on the host from one generator (seeded with
    (seed, epoch): every rank draws the same and takes its slice) and uploaded with the resized sizes and scales in one pinned
    non-blocking copy; per batch there is exactly one launch and no host synchronisation.  It yields (images fp32 [b, 3, out_h, out_w],
    bboxes fp32 [b, g_max, 4], labels int64 [b, g_max], scales fp32 [b]) with out_h / out_w / g_max the batch's maxima, as
    padding_collate_fn pads.  train=False is the reference's Mode.EVAL: no flip, no shuffle, batches in order (the last one may be
    short); the scales let an evaluation map detections back.  `batches(start)` iterates from batch `start` of the coming epoch
    without building the ones before it (a resumed run)."""

    def __init__(self, images, boxes, classes, batch, device, train, min_side=600., max_side=1000., seed=None, rank=0, world=1):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ops.AfanLibraryError("DetDeviceLoader needs an MI355X: the batch is built by a HIP kernel and there is no CPU path")
        img, off, hs, ws, bx, cl, box_off = pack_det_split(images, boxes, classes)
        self.n = len(hs)
        self.hs, self.ws = hs.astype(np.int64), ws.astype(np.int64)
        self.counts = np.diff(box_off)
        self.train, self.batch = bool(train), int(batch)
        self.min_side, self.max_side = float(min_side), float(max_side)
        self.rank, self.world, self.seed, self.epoch = int(rank), int(world), seed, 0
        if world > 1 and seed is None:
            raise RuntimeError("a data-parallel DetDeviceLoader needs a seed shared by all ranks")
        if self.batch < 1 or self.batch % self.world:
            raise ValueError("the batch must be positive and divide among the ranks")
        sizes = [preprocess_size(int(h), int(w), self.min_side, self.max_side) for h, w in zip(self.hs, self.ws)]
        self.oh = np.array([s[0] for s in sizes], np.int64)
        self.ow = np.array([s[1] for s in sizes], np.int64)
        self.scale = np.array([s[2] for s in sizes], np.float64).astype(np.float32)       # torch.tensor(scale, dtype=torch.float)
        if int(self.oh.min()) < 1 or int(self.ow.min()) < 1:
            raise ValueError("the split holds an image whose resized side rounds to 0")
        shrink = max(float((self.hs / self.oh).max()), float((self.ws / self.ow).max()), 1.0)
        if shrink > MAX_SHRINK:
            raise ValueError(f"the split asks for a reduction by {shrink:.3f} > {MAX_SHRINK}: more taps than the kernel holds (KMAX = {KMAX})")
        self.max_shrink = shrink
        self.ratios = self.ws / self.hs                                   # float(width / height), voc2007.py:88
        if self.train:
            self.n_batches = int((self.ratios < 1).sum()) // self.batch + int((self.ratios >= 1).sum()) // self.batch
        else:
            self.n_batches = (self.n + self.batch - 1) // self.batch
        dev = self.device
        self.images = torch.from_numpy(img).to(dev)
        self.offsets = torch.from_numpy(off).to(dev)
        self.d_hs = torch.from_numpy(hs).to(dev)
        self.d_ws = torch.from_numpy(ws).to(dev)
        self.boxes = torch.from_numpy(bx).to(dev)
        self.classes = torch.from_numpy(cl).to(dev)
        self.box_off = torch.from_numpy(box_off).to(dev)

    def __len__(self):
        return self.n_batches

    def _draw(self):
        """The epoch's parameters: int64 [4, n_used] (index, oh, ow, flip), fp32 [n_used] scales and the per-batch (lo, hi) ranges."""
        if self.train:
            rng = np.random.default_rng(None if self.seed is None else [int(self.seed), self.epoch])
            idx = ratio_batches(self.ratios, self.batch, rng).reshape(-1)
            flip = (rng.random(idx.shape[0]) < 0.5).astype(np.int64)
        else:
            idx = np.arange(self.n)
            flip = np.zeros(self.n, np.int64)
        self.epoch += 1
        bounds = [(b * self.batch, min((b + 1) * self.batch, idx.shape[0])) for b in range(self.n_batches)]
        return np.stack([idx, self.oh[idx], self.ow[idx], flip]).astype(np.int64), self.scale[idx], bounds

    def __iter__(self):
        return self.batches(0)

    def batches(self, start=0):
        params, scales, bounds = self._draw()
        self.last_params, self.last_scales = params, scales             # (host copies: what tests compare the batches against)
        if not bounds:
            return
        dev_params = torch.from_numpy(params).pin_memory().to(self.device, non_blocking=True)        # one upload per epoch ...
        dev_scales = torch.from_numpy(scales).pin_memory().to(self.device, non_blocking=True)        # (... of two arrays)
        per = self.batch // self.world
        for lo_b, hi_b in bounds[int(start):]:
            # the whole batch's maxima, whatever the rank's slice: every rank pads alike (padding_collate_fn runs before the scatter)
            out_h, out_w = int(params[1, lo_b:hi_b].max()), int(params[2, lo_b:hi_b].max())
            g_max = int(self.counts[params[0, lo_b:hi_b]].max())
            lo = lo_b + self.rank * per
            hi = min(lo + per, hi_b)
            if hi <= lo:
                continue
            p = dev_params[:, lo:hi]
            s = dev_scales[lo:hi]
            img, bb, lb = ops.det_batch_resize(self.images, self.offsets, self.d_hs, self.d_ws, self.boxes, self.classes, self.box_off,
                                               p[0], p[1], p[2], p[3], s, out_h, out_w, g_max, self.max_shrink)
            yield img, bb, lb, s


# ------------------------------------------------------------------------------------ where a split comes from
def _read_voc_year(voc_dir, image_set):
    import xml.etree.ElementTree as ET
    from PIL import Image
    ids_txt = os.path.join(voc_dir, 'ImageSets', 'Main', image_set + '.txt')
    ann_dir, jpg_dir = os.path.join(voc_dir, 'Annotations'), os.path.join(voc_dir, 'JPEGImages')
    for path in (ids_txt, ann_dir, jpg_dir):
        if not os.path.exists(path):
            raise FileNotFoundError(f"VOC detection data not found: {path} is missing; there is no download in this build")
    with open(ids_txt, 'r') as f:
        image_ids = [line.rstrip() for line in f.readlines()]
    images, boxes, classes, dropped = [], [], [], 0
    for image_id in image_ids:
        path = os.path.join(ann_dir, f'{image_id}.xml')
        if not os.path.exists(path):
            raise FileNotFoundError(f"VOC detection data not found: {path} is missing; there is no download in this build")
        root = ET.ElementTree(file=path).getroot()
        bb, cc = [], []
        for obj in root.iterfind('object'):
            if next(obj.iterfind('difficult')).text == '1':
                continue
            bb.append([float(next(obj.iterfind('bndbox/' + k)).text) - 1 for k in ('xmin', 'ymin', 'xmax', 'ymax')])   # 0-based
            cc.append(CATEGORY_TO_LABEL_DICT[next(obj.iterfind('name')).text])
        if not bb:
            dropped += 1
            continue
        path = os.path.join(jpg_dir, root.find('filename').text)
        if not os.path.exists(path):
            raise FileNotFoundError(f"VOC detection data not found: {path} is missing; there is no download in this build")
        images.append(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8))
        boxes.append(np.array(bb, np.float32))
        classes.append(np.array(cc, np.int64))
    return images, boxes, classes, dropped


def load_voc_det(root, name, train):
    """dataset/voc2007.py:45-89 / voc20072012.py: VOCdevkit/VOC2007 (training: trainval.txt, plus VOCdevkit/VOC2012's trainval.txt for
    voc20072012; evaluation: VOC2007's test.txt), the annotation XML parsed with the reference's `- 1` on every coordinate and its
    category table, `difficult` objects dropped, the JPEGs decoded ONCE on the host with Pillow in list order -> (list of HWC uint8,
    list of fp32 [g, 4], list of int64 [g]).  An image left with no object is dropped and the count printed (the reference's
    `bboxes[:, [0, 2]]` raises on it).  There is no download here."""
    if name not in DATASETS:
        raise ValueError(f"load_voc_det reads {' and '.join(DATASETS)}, not {name!r}")
    try:
        import PIL.Image  # noqa: F401
    except ImportError as e:
        raise ImportError("load_voc_det decodes JPEG files with Pillow, which is not installed; --synthetic N needs no files") from e
    image_set = 'trainval' if train else 'test'
    years = ['VOC2007'] + (['VOC2012'] if (name == 'voc20072012' and train) else [])
    images, boxes, classes, dropped = [], [], [], 0
    for year in years:
        im, bb, cc, d = _read_voc_year(os.path.join(root, 'VOCdevkit', year), image_set)
        images += im
        boxes += bb
        classes += cc
        dropped += d
    if dropped:
        print(f"Dropped {dropped} images without a non-difficult object")
    if not images:
        raise FileNotFoundError(f"VOC detection data not found: the '{image_set}' list under {root} names no image with an object")
    return images, boxes, classes


def load_voc_det_eval(root, name):
    """The evaluation split of dataset/voc2007.py (Mode.EVAL) together with what voc_eval.py reads from the same files: VOC2007's test.txt
    (voc20072012 evaluates on it too), EVERY image of the list kept.  -> (images, boxes, classes, image ids, ground truth): boxes /
    classes are what the loader yields for the image — its non-difficult objects with the `- 1` on every coordinate, fp32 [g, 4] /
    int64 [g], empty for an image that has none — and ground truth maps an image id to (classes int64 [k], difficult bool [k], boxes
    int64 [k, 4]) of ALL its objects with the XML's own integers, which is what the matching compares detections with."""
    import xml.etree.ElementTree as ET
    if name not in DATASETS:
        raise ValueError(f"load_voc_det_eval reads {' and '.join(DATASETS)}, not {name!r}")
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("load_voc_det_eval decodes JPEG files with Pillow, which is not installed; --synthetic N needs no files") from e
    voc_dir = os.path.join(root, 'VOCdevkit', 'VOC2007')
    ids_txt = os.path.join(voc_dir, 'ImageSets', 'Main', 'test.txt')
    ann_dir, jpg_dir = os.path.join(voc_dir, 'Annotations'), os.path.join(voc_dir, 'JPEGImages')
    for path in (ids_txt, ann_dir, jpg_dir):
        if not os.path.exists(path):
            raise FileNotFoundError(f"VOC detection data not found: {path} is missing; there is no download in this build")
    with open(ids_txt, 'r') as f:
        image_ids = [line.rstrip() for line in f.readlines()]
    images, boxes, classes, ground_truth = [], [], [], {}
    for image_id in image_ids:
        path = os.path.join(ann_dir, f'{image_id}.xml')
        if not os.path.exists(path):
            raise FileNotFoundError(f"VOC detection data not found: {path} is missing; there is no download in this build")
        root_tag = ET.ElementTree(file=path).getroot()
        cc, dd, raw = [], [], []
        for obj in root_tag.iterfind('object'):
            cc.append(CATEGORY_TO_LABEL_DICT[next(obj.iterfind('name')).text])
            dd.append(next(obj.iterfind('difficult')).text == '1')
            raw.append([next(obj.iterfind('bndbox/' + k)).text for k in ('xmin', 'ymin', 'xmax', 'ymax')])
        cc, dd = np.array(cc, np.int64), np.array(dd, bool)
        ground_truth[image_id] = (cc, dd, np.array([[int(v) for v in r] for r in raw], np.int64).reshape(-1, 4))
        easy = ~dd
        boxes.append((np.array([[float(v) for v in r] for r in raw], np.float64).reshape(-1, 4)[easy] - 1).astype(np.float32))
        classes.append(cc[easy])
        path = os.path.join(jpg_dir, root_tag.find('filename').text)
        if not os.path.exists(path):
            raise FileNotFoundError(f"VOC detection data not found: {path} is missing; there is no download in this build")
        images.append(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8))
    if not images:
        raise FileNotFoundError(f"VOC detection data not found: the 'test' list under {root} names no image")
    return images, boxes, classes, image_ids, ground_truth


class SyntheticDetSplit:
    """A split for machines without the data: n seeded uint8 images with sides in [min_side, max_side], alternately tall and fat,
    each with 1 to max_boxes boxes inside the image (at least 4 pixels on a side) and classes in 1..classes-1."""

    def __init__(self, n, seed=0, min_side=96, max_side=160, classes=21, max_boxes=6):
        rng = np.random.default_rng(seed)
        self.num_classes = classes
        self.images, self.boxes, self.classes = [], [], []
        for i in range(n):
            a, b = sorted(int(v) for v in rng.integers(min_side, max_side + 1, 2))
            if a == b:
                b = a + 1
            h, w = (b, a) if i % 2 == 0 else (a, b)               # tall, fat, tall, ...
            self.images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            g = int(rng.integers(1, max_boxes + 1))
            x0 = rng.integers(0, w - 4, g)
            y0 = rng.integers(0, h - 4, g)
            x1 = x0 + 4 + (rng.random(g) * (w - 1 - 4 - x0)).astype(np.int64)
            y1 = y0 + 4 + (rng.random(g) * (h - 1 - 4 - y0)).astype(np.int64)
            self.boxes.append(np.stack([x0, y0, x1, y1], axis=1).astype(np.float32))
            self.classes.append(rng.integers(1, classes, g).astype(np.int64))

    def __len__(self):
        return len(self.images)

    @property
    def image_ids(self):
        """"000000", "000001", ...: the names an evaluation files its detections under."""
        return ['{:06d}'.format(i) for i in range(len(self.images))]

    def ground_truth(self):
        """What load_voc_det_eval returns as ground truth: every object non-difficult, boxes as the 1-based integers an annotation
        file would hold (the split's own boxes are 0-based)."""
        return {i: (c.copy(), np.zeros(len(c), bool), b.astype(np.int64) + 1) for i, b, c in zip(self.image_ids, self.boxes, self.classes)}
