"""det_ops.class_nms (afan_det_class_nms + afan_det_pack: decode, clip, score filter, sort and greedy NMS of every (image, class) list
in one launch) against the composition it replaces: F.softmax, det_ops.box_decode_clip on the denormalised transformers and
det_ops.nms(boxes, probs, 0.3) per class — boxes, probabilities and counts bit for bit.

torch.sort leaves the order of equal scores open, so ties are excluded by construction: the probabilities come from the softmax on the
device, and on the host every value that repeats within its (image, class) list is moved to the next free fp32 value before both
paths see them."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CAP = 2048
MEAN, STD = (0., 0., 0., 0.), (.1, .1, .2, .2)
W, H = 904., 600.


def _inputs(gpu, B, N, C, seed):
    """Proposals clustered round a few centres (so that suppression happens), raw transformers ~ N(0, 1), logits scaled so that the
    probabilities spread over (0, 1); probabilities pairwise distinct within every list."""
    g = torch.Generator().manual_seed(seed)
    k = max(1, min(6, N // 8))
    cxy = torch.rand(B, k, 2, generator=g) * torch.tensor([W - 200, H - 200]) + 100
    wh = torch.rand(B, k, 2, generator=g) * 150 + 40
    pick = torch.randint(0, k, (B, N), generator=g)
    c = torch.gather(cxy, 1, pick[..., None].expand(B, N, 2)) + torch.randn(B, N, 2, generator=g) * 10
    s = torch.gather(wh, 1, pick[..., None].expand(B, N, 2)) * (1 + torch.randn(B, N, 2, generator=g) * 0.1).clamp(0.5, 1.5)
    proposals = torch.cat([c - s / 2, c + s / 2], dim=-1).clamp(min=0)
    proposals[..., 2] = proposals[..., 2].clamp(max=W + 60)              # some reach past the right edge: the clip has work to do
    tr = torch.randn(B, N, C, 4, generator=g)
    logits = torch.randn(B, N, C, generator=g) * (3.0 if C > 4 else 1.0)          # (few classes: keep clear of fp32's crowding below 1)
    probs = F.softmax(logits.to(gpu), dim=-1).cpu().numpy()
    for b in range(B):
        for cc in range(C):
            col = probs[b, :, cc]
            seen = set()
            for n in range(N):
                v = col[n]
                while float(v) in seen:
                    v = np.nextafter(v, np.float32(2.0))
                seen.add(float(v))
                col[n] = v
            assert len(set(col.tolist())) == N                          # asserted on the host: no list holds a tie
    return proposals.to(gpu), tr.to(gpu), torch.from_numpy(probs).to(gpu)


def _yardstick(pkg, proposals, tr, probs, min_prob=None):
    """The loop of generate_detections on the operators the issue names -> (boxes, probs, counts [B, C - 1])."""
    B, N, C = probs.shape
    dev = probs.device
    t = tr * torch.tensor(STD, device=dev) + torch.tensor(MEAN, device=dev)
    boxes = pkg.det_ops.box_decode_clip(proposals.unsqueeze(2).repeat(1, 1, C, 1), t, W, H)
    ob, op, cnt = [], [], torch.zeros(B, C - 1, dtype=torch.int64)
    for b in range(B):
        for c in range(1, C):
            cb, cp = boxes[b, :, c, :], probs[b, :, c]
            keep = pkg.det_ops.nms(cb, cp, 0.3).to(dev)
            if min_prob is not None:
                keep = keep[cp[keep] > min_prob]
            ob.append(cb[keep])
            op.append(cp[keep])
            cnt[b, c - 1] = len(keep)
    return torch.cat(ob), torch.cat(op), cnt


def _compare(pkg, proposals, tr, probs, min_prob=None):
    want_b, want_p, want_c = _yardstick(pkg, proposals, tr, probs, min_prob)
    fb, fp, counts = pkg.det_ops.class_nms(proposals, tr, probs, MEAN + STD, W, H, 0.3, min_prob)
    torch.cuda.synchronize()
    counts = counts.cpu()
    total = int(counts.sum())
    assert torch.equal(counts, want_c)
    assert torch.equal(fb[:total], want_b) and torch.equal(fp[:total], want_p)
    return counts


@pytest.mark.parametrize("B,N,C", [(1, 1, 2), (1, 63, 21), (1, 64, 21), (1, 65, 21), (2, 300, 21), (1, 301, 3), (1, CAP, 2)])
def test_equals_the_per_class_composition(pkg, gpu, B, N, C):
    assert pkg.det_ops.class_nms_supported(N, C)
    proposals, tr, probs = _inputs(gpu, B, N, C, seed=1000 * B + N + C)
    counts = _compare(pkg, proposals, tr, probs)
    assert int(counts.min()) >= 1
    if N >= 63:
        assert int(counts.max()) > 1 and int(counts.min()) < N          # some list keeps more than one box, some list drops one


def test_min_prob_filters_like_the_evaluator(pkg, gpu):
    proposals, tr, probs = _inputs(gpu, 2, 300, 21, seed=77)
    probs[0, :, 3] = probs[0, :, 3] * 0.04                               # a list that ends up empty (every value <= 0.04, still distinct)
    assert len(set(probs[0, :, 3].cpu().tolist())) == 300
    counts = _compare(pkg, proposals, tr, probs, min_prob=0.05)
    assert counts[0, 2] == 0 and int(counts.sum()) > 0
    full = _compare(pkg, proposals, tr, probs)
    assert (counts <= full).all() and int(counts.sum()) < int(full.sum())
    neg = pkg.det_ops.class_nms(proposals, tr, probs, MEAN + STD, W, H, 0.3, -1.0)[2].cpu()     # min_prob < 0 keeps everything
    assert torch.equal(neg, full)


def test_identical_boxes_keep_one(pkg, gpu):
    N, C = 130, 4
    _, _, probs = _inputs(gpu, 1, N, C, seed=5)
    proposals = torch.tensor([100., 120., 300., 380.], device=gpu).repeat(1, N, 1)
    tr = torch.zeros(1, N, C, 4, device=gpu)
    counts = _compare(pkg, proposals, tr, probs)
    assert counts.tolist() == [[1, 1, 1]]
    fb, fp, _ = pkg.det_ops.class_nms(proposals, tr, probs, MEAN + STD, W, H, 0.3)
    assert torch.equal(fp[:3], probs[0, :, 1:].max(dim=0).values) and torch.equal(fb[:3], proposals[0, :3])


def test_zero_width_boxes_behave_as_in_nms(pkg, gpu):
    """Proposals right of the image clip to x1 = x2 = right: width 0, area (0 + 1) * (h + 1) by the + 1."""
    N, C = 90, 3
    proposals, tr, probs = _inputs(gpu, 1, N, C, seed=9)
    proposals[..., 0] += 2000.
    proposals[..., 2] += 2000.
    tr[..., 0] = 0
    want_b, _, _ = _yardstick(pkg, proposals, tr, probs)
    assert (want_b[:, 0] == W).all() and (want_b[:, 2] == W).all()
    counts = _compare(pkg, proposals, tr, probs)
    assert int(counts.max()) > 1 and int(counts.min()) < N


def _detection(pkg, gpu, C):
    return pkg.det_model.Model.Detection("align", nn.Sequential(), 8, C, 1.0).to(gpu).eval()


def _through_generate_detections(pkg, gpu, monkeypatch, N, C, on, compared=True):
    proposals, tr, probs = _inputs(gpu, 1, N, C, seed=N + C)
    logits = torch.log(probs)                                             # softmax(log p) is p up to rounding: only the route is under test
    again = F.softmax(logits, dim=-1).cpu().numpy()
    assert not compared or all(len(set(again[0, :, c].tolist())) == N for c in range(1, C))      # ... and still without a tie in any list
    calls = []
    real = pkg.det_model.nms
    monkeypatch.setattr(pkg.det_model, "nms", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(pkg.det_model.Model, "CLASS_NMS", on)
    out = _detection(pkg, gpu, C).generate_detections(proposals, logits, tr.reshape(1, N, C * 4), W, H)
    return out, len(calls)


def test_beyond_the_cap_the_loop_runs(pkg, gpu, monkeypatch):
    assert not pkg.det_ops.class_nms_supported(CAP + 1, 2)
    out, calls = _through_generate_detections(pkg, gpu, monkeypatch, CAP + 1, 2, True, compared=False)
    assert calls == 1 and out[0].shape[0] == out[1].shape[0] == out[2].shape[0] == out[3].shape[0] > 0


def test_supported_shapes_do_not_call_nms_and_return_the_loops_tensors(pkg, gpu, monkeypatch):
    on, calls_on = _through_generate_detections(pkg, gpu, monkeypatch, 300, 21, True)
    off, calls_off = _through_generate_detections(pkg, gpu, monkeypatch, 300, 21, False)
    assert calls_on == 0 and calls_off == 20
    for a, b in zip(on, off):
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    assert on[1].dtype == torch.int and on[3].dtype == torch.long and on[0].shape[0] > 20
    flt = _detection(pkg, gpu, 21)
    proposals, tr, probs = _inputs(gpu, 1, 300, 21, seed=321)
    a = flt.generate_detections(proposals, torch.log(probs), tr.reshape(1, 300, 84), W, H, min_prob=0.05)
    monkeypatch.setattr(pkg.det_model.Model, "CLASS_NMS", False)
    b = flt.generate_detections(proposals, torch.log(probs), tr.reshape(1, 300, 84), W, H, min_prob=0.05)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y)
    assert a[0].shape[0] > 0 and bool((a[2] > 0.05).all())
