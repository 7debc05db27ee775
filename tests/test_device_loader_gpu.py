"""cls_data.DeviceLoader on the one-launch kernel: the same batches, bit for bit, as the torch chain (_augment_torch) fed with the
same seeds and the same permutation."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mp():
    return importlib.import_module("cv_a-fan_amd.cls_data")


def _fake(n):
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, (n, 3, 32, 32), dtype=np.uint8), rng.integers(0, 10, n).astype(np.int64)


def test_training_epoch_equals_the_torch_chain(pkg, gpu):
    mp = _mp()
    x, y = _fake(64)
    loader = mp.DeviceLoader(x, y, 16, gpu, True)
    assert len(loader) == 4
    torch.manual_seed(7)
    torch.cuda.manual_seed_all(7)
    before = pkg.ops.CALLS["batch_crop_flip"]
    got = []
    for k, (xb, yb) in enumerate(loader):
        assert pkg.ops.CALLS["batch_crop_flip"] == before + k + 1        # exactly one launch per batch
        got.append((xb.clone(), yb.clone()))
    assert len(got) == 4
    # the same seeds by hand: permutation on the CPU generator, then per batch rows, columns, flips on the device generator
    torch.manual_seed(7)
    torch.cuda.manual_seed_all(7)
    perm = torch.randperm(64)
    xd, yd = torch.as_tensor(x).to(gpu), torch.as_tensor(y).to(gpu)
    for b, (xb, yb) in enumerate(got):
        idx = perm[b * 16:(b + 1) * 16].to(gpu)
        top = torch.randint(0, 9, (16,), device=gpu)
        left = torch.randint(0, 9, (16,), device=gpu)
        flip = torch.rand(16, device=gpu) < 0.5
        assert torch.equal(xb, mp._augment_torch(xd[idx], top, left, flip)), b
        assert torch.equal(yb, yd[idx]), b
        assert xb.dtype == torch.float32 and xb.shape == (16, 3, 32, 32)


def test_evaluation_loader_with_a_ragged_last_batch(pkg, gpu):
    mp = _mp()
    x, y = _fake(70)
    loader = mp.DeviceLoader(x, y, 16, gpu, False, drop_last=False)
    assert len(loader) == 5
    xd, yd = torch.as_tensor(x).to(gpu), torch.as_tensor(y).to(gpu)
    before = pkg.ops.CALLS["batch_crop_flip"]
    sizes = []
    for b, (xb, yb) in enumerate(loader):
        order = torch.arange(b * 16, min((b + 1) * 16, 70), device=gpu)
        assert torch.equal(xb, xd[order].float() / 255) and torch.equal(yb, yd[order])
        sizes.append(xb.shape[0])
    assert sizes == [16, 16, 16, 16, 6]
    assert pkg.ops.CALLS["batch_crop_flip"] == before + 5


def test_two_ranks_split_the_world_one_batch(pkg, gpu):
    mp = _mp()
    x = np.zeros((64, 3, 32, 32), dtype=np.uint8)
    y = np.arange(64, dtype=np.int64)                                    # the label names the image: index sets are readable
    ranks = [[yb.cpu() for _, yb in mp.DeviceLoader(x, y, 16, gpu, True, rank=r, world=2, seed=123)] for r in (0, 1)]
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(123))
    assert len(ranks[0]) == len(ranks[1]) == 4
    for b in range(4):
        a0, a1 = ranks[0][b], ranks[1][b]
        assert a0.shape == a1.shape == (8,)
        assert not set(a0.tolist()) & set(a1.tolist())
        assert torch.equal(torch.cat([a0, a1]), perm[b * 16:(b + 1) * 16])           # together: the world-1 batch
