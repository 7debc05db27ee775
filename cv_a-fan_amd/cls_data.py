"""Classification data, resident on the device: the CIFAR-10 readers (cifar-10-batches-py pickles, the 45k/5k/10k splits of the
reference's dataset.py), DeviceLoader (shuffle, crop, flip and scaling in one launch per batch, ops.batch_crop_flip),
_augment_torch (the same batch as a chain of torch calls) and SyntheticLoader.  What seg_data.py is for Segmentation."""
import os
import pickle

import numpy as np
import torch

from . import ops


def _cifar10_dir(root):
    return root if os.path.basename(root.rstrip("/")) == "cifar-10-batches-py" else os.path.join(root, "cifar-10-batches-py")


def _read_cifar10_batch(path):
    with open(path, "rb") as f:
        b = pickle.load(f, encoding="latin1")
    return np.asarray(b["data"], dtype=np.uint8).reshape(-1, 3, 32, 32), np.asarray(b["labels"], dtype=np.int64)


def _load_cifar10_test(root):
    """The test split (cifar-10-batches-py/test_batch) as uint8 NCHW images and labels, in file order."""
    return _read_cifar10_batch(os.path.join(_cifar10_dir(root), "test_batch"))


def _load_cifar10(root):
    """cifar-10-batches-py pickles -> uint8 NCHW arrays; the 45k/5k train/val split of dataset.py:43-45."""
    d = _cifar10_dir(root)
    xs, ys = zip(*(_read_cifar10_batch(os.path.join(d, f"data_batch_{i}")) for i in range(1, 6)))
    x, y = np.concatenate(xs), np.concatenate(ys)
    return (x[:45000], y[:45000]), (x[45000:], y[45000:]), _load_cifar10_test(root)


def _augment_torch(x_u8, top=None, left=None, flip=None, pad=4):
    """dataset.py:36-39 on a gathered uint8 batch [m, c, h, w] as a chain of torch calls: RandomCrop(h, padding=pad) at offsets
    (top, left) in [0, 2*pad], RandomHorizontalFlip where flip, ToTensor's /255.  The draws are the caller's.  DeviceLoader's path on a
    device without the library's kernels, and what tests hold ops.batch_crop_flip to, bit for bit.  top is None: scale only."""
    x = x_u8
    if top is not None:
        m, _, h, w = x.shape
        dev = x.device
        xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))                     # [m, c, h + 2 pad, w + 2 pad]
        rows = top[:, None] + torch.arange(h, device=dev)[None, :]
        cols = left[:, None] + torch.arange(w, device=dev)[None, :]
        cols = torch.where(flip[:, None], cols.flip(1), cols)
        bi = torch.arange(m, device=dev)[:, None, None]
        x = xp[bi, :, rows[:, :, None], cols[:, None, :]].permute(0, 3, 1, 2).contiguous()
    return x.float().div_(255.0)


class DeviceLoader:
    """Whole split resident in HBM as uint8 (CIFAR-10 train = 138 MB of 288 GB); per batch: shuffle index, random
    crop (pad 4) + horizontal flip (dataset.py:36-39) and the /255 ToTensor scaling run on the device — on a GPU as ONE launch
    (ops.batch_crop_flip: gather, crop, flip, scale and the labels), fed by three draws on the device generator; the epoch's
    permutation is uploaded once."""

    def __init__(self, x_u8, y, batch, device, train, rank=0, world=1, drop_last=True, seed=None, pad=4):
        self.x = torch.as_tensor(x_u8).to(device).contiguous()
        self.y = torch.as_tensor(y).to(device).contiguous()
        self.batch, self.train, self.rank, self.world, self.device = batch, train, rank, world, device
        self.pad = int(pad)
        # data parallel: every rank must slice the SAME permutation (its own CPU generator would give overlapping shards):
        # a generator seeded with (seed + epoch), `seed` agreed on by all ranks (main() broadcasts rank 0's draw)
        self.seed, self.epoch = seed, 0
        n = self.x.shape[0]
        self.n_batches = n // batch if drop_last else (n + batch - 1) // batch

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        n = self.x.shape[0]
        if not self.train:
            perm = torch.arange(n)
        elif self.world > 1:
            if self.seed is None:
                raise RuntimeError("a data-parallel DeviceLoader needs a seed shared by all ranks")
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(self.seed) + self.epoch))
            self.epoch += 1
        else:
            perm = torch.randperm(n)                                  # CPU generator, like DataLoader's sampler
        per = self.batch // self.world
        idxs = []
        for b in range(self.n_batches):
            idx = perm[b * self.batch:(b + 1) * self.batch]
            idxs.append(idx[self.rank * per:(self.rank + 1) * per] if self.world > 1 else idx)
        on_gpu = torch.device(self.device).type == "cuda"
        if on_gpu and idxs:
            # one upload per epoch: this rank's index list of every batch, back to back
            every = torch.cat(idxs).to(self.device)
            ends = torch.tensor([i.shape[0] for i in idxs]).cumsum(0).tolist()
            idxs = [every[e - i.shape[0]:e] for i, e in zip(idxs, ends)]
        for idx in idxs:
            m = idx.shape[0]
            top = left = flip = None
            if self.train:
                top = torch.randint(0, 2 * self.pad + 1, (m,), device=self.device)
                left = torch.randint(0, 2 * self.pad + 1, (m,), device=self.device)
                flip = torch.rand(m, device=self.device) < 0.5
            if on_gpu:
                yield ops.batch_crop_flip(self.x, idx, top, left, flip, labels=self.y, pad=self.pad if self.train else 0)
            else:
                idx = idx.to(self.device)
                yield _augment_torch(self.x[idx], top, left, flip, self.pad), self.y[idx]


class SyntheticLoader:
    """U[0,1) images / uniform labels (SURVEY.md §8d synthetic inputs), generated once, resident in HBM."""

    def __init__(self, n, batch, device, rank=0, world=1, seed=3, side=32, classes=10):
        g = torch.Generator().manual_seed(seed + 1000 * rank)
        per = batch // world
        self.n_batches = max(n // batch, 1)
        self.x = [torch.rand(per, 3, side, side, generator=g).to(device) for _ in range(min(self.n_batches, 8))]
        self.y = [torch.randint(0, classes, (per,), generator=g).to(device) for _ in range(min(self.n_batches, 8))]

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        for b in range(self.n_batches):
            yield self.x[b % len(self.x)], self.y[b % len(self.y)]
