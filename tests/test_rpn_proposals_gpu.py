"""det_ops.rpn_proposals (afan_rpn_proposals: the proposal layer's NMS and row block for all images of a batch in three launches)
against the per-image path it replaces — det_ops.nms(max_keep, presorted, padded) on the gathered candidates + det_ops.proposal_rows —
on the same inputs: `padded` and `kept` bit for bit.

Shapes (A, pre_n, top_n), B = 3: one box; a ragged last 64-block with A > pre_n; A < pre_n and top_n beyond the survivors; lists
longer than the scan's band (12 blocks) plus ring (8), so that the worker waves have rows to OR, with an early stop; 47 blocks with
no early stop.  The three images differ: tightly clustered boxes (few survivors), boxes spread over a large canvas (many), and one
box repeated plus zero-extent boxes at one point (under the reference's +1 corners a zero-extent box has area 1: IoU 1 with its
copies, 1 / 1681 with the repeated box — the repeated box and one point box survive).  `order` is torch.sort's of random scores."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

THR = 0.7
CASES = [(1, 12000, 5), (65, 64, 10), (200, 200, 300), (1500, 1300, 100), (3000, 3000, 2000)]


def _images(A, seed):
    g = torch.Generator().manual_seed(seed)
    # clustered: six centres, jitter of a few pixels on boxes of ~100 pixels
    c = torch.rand(6, 2, generator=g) * 700
    which = torch.randint(0, 6, (A,), generator=g)
    xy = c[which] + torch.randn(A, 2, generator=g) * 3
    wh = 100 + torch.randn(A, 2, generator=g) * 4
    clustered = torch.cat([xy, xy + wh], dim=1)
    # spread: small boxes over a canvas that grows with A
    side = 3.0 * float(A) ** 0.5 + 50
    xy = torch.rand(A, 2, generator=g) * side
    wh = torch.rand(A, 2, generator=g) * 60 + 30
    spread = torch.cat([xy, xy + wh], dim=1)
    # one box repeated, every seventh a zero-extent box at one point
    same = torch.tensor([10.0, 10.0, 50.0, 50.0]).repeat(A, 1)
    same[3::7] = torch.tensor([200.0, 200.0, 200.0, 200.0])
    boxes = torch.stack([clustered, spread, same]).contiguous()
    scores = torch.rand(3, A, generator=g)
    return boxes, scores


def _greedy_count(boxes, thr, stop):
    """Survivors of plain greedy NMS over boxes in the given order (IoU with +1 corners, > thr), counted up to `stop`."""
    b = boxes.astype(np.float32)
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    dead = np.zeros(len(b), dtype=bool)
    kept = 0
    for i in range(len(b)):
        if dead[i]:
            continue
        kept += 1
        if kept >= stop:
            break
        w = np.maximum(np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]) + 1, 0)
        h = np.maximum(np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]) + 1, 0)
        inter = (w * h).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            dead[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > np.float32(thr)
    return kept


def _per_image(pkg, boxes, order, pre_n, top_n):
    cands, keeps = [], []
    for b in range(boxes.shape[0]):
        sb = boxes[b][order[b][:pre_n]]
        keeps.append(pkg.det_ops.nms(sb, None, THR, max_keep=top_n, presorted=True, padded=True))
        cands.append(sb)
    return pkg.det_ops.proposal_rows(cands, keeps, top_n)


@pytest.mark.parametrize("A,pre_n,top_n", CASES)
def test_batched_proposals_equal_the_per_image_path(pkg, gpu, A, pre_n, top_n):
    boxes, scores = _images(A, 1000 + A)
    order = torch.sort(scores, dim=-1, descending=True)[1]
    n = min(pre_n, A)
    if (A, pre_n, top_n) in ((1500, 1300, 100), (3000, 3000, 2000)):
        counts = [_greedy_count(boxes[b][order[b][:n]].numpy(), THR, top_n) for b in range(3)]
        print("survivors (counted up to top_n):", counts)
        if top_n == 100:
            assert any(c >= top_n for c in counts) and any(c < top_n for c in counts), counts
        else:
            assert all(c < top_n for c in counts), counts
    boxes, order = boxes.to(gpu), order.to(gpu)
    want_p, want_k = _per_image(pkg, boxes, order, pre_n, top_n)
    got_p, got_k = pkg.det_ops.rpn_proposals(boxes, order, pre_n, THR, top_n)
    assert got_p.shape == (3, top_n, 4) and got_p.dtype == torch.float32 and got_k.shape == (3,) and got_k.dtype == torch.int64
    assert torch.equal(got_k, want_k), (got_k.tolist(), want_k.tolist())
    assert torch.equal(got_p, want_p)
    k = got_k.tolist()
    assert all(1 <= c <= min(n, top_n) for c in k)
    for b, c in enumerate(k):
        assert not got_p[b, c:].any()                    # zero rows behind the survivors
    if A >= 200:
        assert k[2] == 2                                 # the repeated box and one point box


def test_reference_golden_list_as_one_image_of_a_batch(pkg, gpu):
    """The reference's own NMS test vector (9770 boxes -> 1934 at 0.7) as the middle image of three."""
    det = torch.from_numpy(np.load(os.path.join(GOLDEN, "det_nms_large_input.npy")))
    expect = torch.from_numpy(np.load(os.path.join(GOLDEN, "det_nms_large_output.npy")))
    A = det.shape[0]
    boxes, scores = _images(A, 7)
    boxes[1], scores[1] = det[:, :4], det[:, 4]
    order = torch.sort(scores, dim=-1, descending=True)[1]
    boxes, order = boxes.to(gpu), order.to(gpu)
    got_p, got_k = pkg.det_ops.rpn_proposals(boxes, order, A, THR, 2000)
    want_p, want_k = _per_image(pkg, boxes, order, A, 2000)
    assert torch.equal(got_k, want_k) and torch.equal(got_p, want_p)
    assert got_k[1].item() == 1934
    o1 = order[1].cpu()
    rows = det[:, :4][o1[torch.isin(o1, expect)]]        # the golden survivors in score order
    assert torch.equal(got_p[1, :1934].cpu(), rows)


def test_batch_sizes_and_workspace(pkg, gpu):
    lib = pkg._lib.load()
    boxes1, scores1 = _images(130, 3)
    for B in (1, 64, 65):
        boxes = boxes1[torch.arange(B) % 3].contiguous().to(gpu)
        order = torch.sort(scores1[torch.arange(B) % 3], dim=-1, descending=True)[1].to(gpu)
        if B == 65:
            with pytest.raises(pkg.AfanLibraryError, match="AFAN_ESHAPE"):
                pkg.det_ops.rpn_proposals(boxes, order, 100, THR, 20)
            continue
        got_p, got_k = pkg.det_ops.rpn_proposals(boxes, order, 100, THR, 20)
        want_p, want_k = _per_image(pkg, boxes, order, 100, 20)
        assert torch.equal(got_k, want_k) and torch.equal(got_p, want_p)
    ws = lib.afan_rpn_proposals_workspace_bytes
    assert ws(0, 100) == 0 and ws(3, 0) == 0
    sizes = [[ws(b, n) for n in (1, 63, 64, 65, 1000, 12000)] for b in (1, 2, 8, 64)]
    for row in sizes:
        assert all(x < y for x, y in zip(row, row[1:])), row
    for r0, r1 in zip(sizes, sizes[1:]):
        assert all(x < y for x, y in zip(r0, r1))
    assert ws(8, 12000) >= 8 * 12000 * 188 * 8
