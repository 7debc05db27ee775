"""References and case tables for the kernels of csrc/afan_det_targets.hip and csrc/afan_det_eval.hip (tests/test_det_targets_pinned_gpu.py
holds the kernels to them through the C ABI; tests/test_det_targets_pinned_ref.py checks them on the CPU).  Written in numpy from the
comments of include/afan_hip.h and the reference's formulas (Detection/bbox.py:41-92, rpn/region_proposal_network.py:66-90 and
:163-185, model.py:256-282, :343-407, extension/functional.py:6-10, support/src/cuda/nms.cu:36-49); nothing here imports the package.

Two kinds of reference.
  * BIT FOR BIT: every value that is a chain of single correctly rounded fp32 operations is restated in np.float32, one numpy operation
    per rounding (the library is built with -ffp-contract=off): both IoUs, the assignment, the labels, the lists, the linear target
    columns, decode + clip wherever expf's value is known without computing it (expf(0) = 1, overflow, underflow to 0), the whole of
    the per-class NMS on such inputs, the pack and the small entries.
  * WINDOWED against float64: |got - f64| <= C * 2^-24 * S elementwise, S the same expression on absolute values, C counted from the
    kernel's expression.  A correctly rounded operation costs one unit of 2^-24 (relative), an expf / logf call 2 ulp = 4 units (no
    document of the installed ROCm states a bound for the two, so the budget is the conventional 2 ulp); an error in the argument of expf
    scales its result by that error, which is why S carries |argument| terms.  Every counted C gets one unit more for the second-order
    terms.  The counts:
      decode              C = 7 + 1, S = |dx * sw| + |scx| + |w| / 2 with w = exp(dz) * sw.  sw, scx: 1 each; dx * sw: 2; cx: adds 1 |cx|;
                          w: 4 (expf) + 1 (sw) + 1 (product), halved exactly; the last subtraction 1 |out|: 4 A + 3 B + 7 W / 2 <= 7 S.
                          The clip is monotone and never increases a distance.
      log target columns  C = 4 + 1, S = 1 + |log|.  dw, sw, dw / sw: 1 each, each moving the logarithm by as much absolutely; logf: 4 |log|.
      ce row              -(x[lab] - m - lse): sum of C exponentials, each 4 + |x[c] - m| (its argument's rounding), C - 1 positive adds;
                          lse = logf(sum): that, absolutely, + 4 |lse|; the two subtractions 1 |x[lab] - m| and 1 |row|:
                          C_row = Cc + 3 on S_row = 1 + A + |x[lab] - m| + |lse|, A = max |x[c] - m| (Cc: the number of classes).
      ce[b]               a thread adds its L rows (L - 1 roundings: the first add, to 0, is exact), block_sum's tree adds 8 levels, the division 1:
                          C = Cc + 3 + (L - 1) + 8 + 1 = Cc + L + 11 (+ 1), S = sum of S_row / samples.
      sl1[b]              per coordinate: target (t - mean) / std 2, e = in - tg 1, |f'| <= 1; the branch's own operations 2 f; three adds
                          over the coordinates: C_row = 5 on S_row = sum(|in| + |tg|) + acc (3 |tg| + |in| <= 3 (|in| + |tg|)); chain, tree, denominator
                          (4 nfg + 1e-8: 1) and division: C = 5 + (L - 1) + 8 + 2 = L + 14 (+ 1).
      u_deltas            Lipschitz 1 / beta in e: C = 3 + 1 on S = (|in| + |tg|) / beta + |u|.
      d_deltas            u * (g / dn): dn 1, division 1, product 1: C = 6 + 1 on |g / dn| * S_u.
      u_logits            p = expf((x[c] - m) - lse) - onehot: the argument's error |x[c] - m| + |arg| + (Cc + 3 + A + 4 |lse|), expf 4, the
                          subtraction 1: C = Cc + 7 (+ 1) on S = p * (1 + |x[c] - m| + |arg| + A + |lse|) + |p - onehot|.
      d_logits            times g / samples: division 1, product 1: C = Cc + 9 (+ 1) on |g / samples| * S_u.
    Results below the normal range (an exponential that underflows) are held to 2^-126 absolutely: the underflow term of the rounding
    model; the build's denormal mode is not what this module pins.
"""
import collections
import re

import numpy as np

F = np.float32
I64 = np.int64
U = 2.0 ** -24
TINY = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)
NAN = F(np.nan)
TB = 256                      # workgroup width of every kernel here but sample_lists
SL_THREADS = 1024             # sample_lists_kernel's one workgroup
MAX_G_LDS = 1024              # box_assign_kernel<0>: the LDS merge up to this many ground truths
MAX_N, MAX_C = 2048, 64       # det_class_nms's caps
OK, ESHAPE, ENULL = 0, -3, -4            # AFAN_OK, AFAN_ESHAPE, AFAN_ENULL (include/afan_hip.h)

C_DECODE, C_LOG, C_U_DELTAS, C_D_DELTAS = 8, 5, 4, 7


def c_ce(n_cls, chain):
    return n_cls + chain + 11 + 1


def c_sl1(chain):
    return chain + 14 + 1


def c_u_logits(n_cls):
    return n_cls + 7 + 1


def c_d_logits(n_cls):
    return n_cls + 9 + 1


def same_f32(got, want):
    """None if the two fp32 arrays agree in every bit (any NaN equal to any NaN), else the flat index of the first difference."""
    g, w = np.ascontiguousarray(got, F).ravel(), np.ascontiguousarray(want, F).ravel()
    assert g.size == w.size, (g.size, w.size)
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


def window(got, ref, bound):
    """(every element inside, worst |got - ref| / bound): a NaN of the reference must be a NaN, an infinite bound holds anything finite."""
    got, ref, bound = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    with np.errstate(all="ignore"):
        nan = np.isnan(ref)
        err = np.abs(got - ref)
        ok = np.where(nan, np.isnan(got), err <= bound)
        fin = ~nan & np.isfinite(bound) & (bound > 0) & np.isfinite(err)
        ratio = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    return bool(ok.all()), ratio, (int(np.flatnonzero(~ok)[0]) if not ok.all() else None)


# ====================================================================================================================== decode, clip
def clip(o, right, bottom):
    """bbox.py:89-92: Tensor.clamp on each coordinate: a NaN stays a NaN (np.minimum / np.maximum propagate it, like clamp)."""
    o = o.copy()
    z, r, b = o.dtype.type(0), o.dtype.type(right), o.dtype.type(bottom)
    o[:, 0], o[:, 2] = np.minimum(np.maximum(o[:, 0], z), r), np.minimum(np.maximum(o[:, 2], z), r)
    o[:, 1], o[:, 3] = np.minimum(np.maximum(o[:, 1], z), b), np.minimum(np.maximum(o[:, 3], z), b)
    return o


def exp_known(d):
    """(expf(d), known) where the value is known without computing an exponential: expf(0) = 1, overflow, full underflow, NaN."""
    d = np.asarray(d, F)
    v = np.full(d.shape, NAN, F)
    known = np.zeros(d.shape, bool)
    for m, val in ((d == 0, 1.0), (d >= 89, np.inf), (d <= -104, 0.0), (np.isnan(d), np.nan)):
        v[m], known[m] = F(val), True
    return v, known


def decode_clip_f32(src, t, right, bottom):
    """bbox.py:54-64 + clip in fp32, one operation per rounding -> (boxes, rows whose every bit is known)."""
    s, d = np.asarray(src, F), np.asarray(t, F)
    ew, kw = exp_known(d[:, 2])
    eh, kh = exp_known(d[:, 3])
    two = F(2)
    with np.errstate(all="ignore"):
        scx, scy, sw, sh = (s[:, 0] + s[:, 2]) / two, (s[:, 1] + s[:, 3]) / two, s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
        cx, cy, w, h = d[:, 0] * sw + scx, d[:, 1] * sh + scy, ew * sw, eh * sh
        o = np.stack([cx - w / two, cy - h / two, cx + w / two, cy + h / two], axis=1).astype(F)
    return clip(o, F(right), F(bottom)), kw & kh


def decode_clip_f64(src, t, right, bottom):
    """-> (boxes, S) in float64; an exponential beyond fp32's range is the infinity fp32 gives (so inf * 0 is the NaN it is there)."""
    s, d = np.asarray(src, F).astype(np.float64), np.asarray(t, F).astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(d[:, 2:4])
        e[e > FLT_MAX] = np.inf
        scx, scy, sw, sh = (s[:, 0] + s[:, 2]) / 2, (s[:, 1] + s[:, 3]) / 2, s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
        ax, ay, w, h = d[:, 0] * sw, d[:, 1] * sh, e[:, 0] * sw, e[:, 1] * sh
        cx, cy = ax + scx, ay + scy
        o = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1)
        sx, sy = np.abs(ax) + np.abs(scx) + np.abs(w) / 2, np.abs(ay) + np.abs(scy) + np.abs(h) / 2
        S = np.stack([sx, sy, sx, sy], axis=1)
    return clip(o, right, bottom), S


RIGHT, BOTTOM = 600.0, 400.0
_B40 = (10, 10, 50, 50)
DECODE_SPECIALS = [  # (source box, transformer)
    (_B40, (np.nan, 0, 0, 0)), ((5, 5, 5, 5), (0, 0, 100, 0)), (_B40, (-2, 0, 0, 0)), (_B40, (20, 0, 0, 0)), (_B40, (0, -2, 0, 0)),
    (_B40, (0, 20, 0, 0)), ((5, 5, 5, 5), (1, 1, 0.5, 0.5)), ((7, 9, 7, 30), (0.5, 0.25, 100, -200)), (_B40, (0, 0, 0, np.nan)),
    (_B40, (0, 0, 100, 0)), (_B40, (0.5, 0.5, -200, 0)), (_B40, (0, 0, 0.5, -0.25)), ((590, 390, 640, 420), (0, 0, 0, 0))]
DECODE_N = (1, 255, 256, 257)
DECODE_KINDS = ("dyadic", "gauss", "specials")
DC = collections.namedtuple("DC", "n kind")
DECODE_CASES = [DC(n, k) for n in DECODE_N for k in DECODE_KINDS]


def decode_inputs(c):
    """dyadic: quarter-pixel boxes, transformers k / 4 with dw = dh = 0 (every operation exact or known); gauss: everything inexact;
    specials: the Gaussian table with DECODE_SPECIALS laid over its first rows and, where there is room, its last."""
    rng = np.random.default_rng(1000 + c.n + 7 * DECODE_KINDS.index(c.kind))
    if c.kind == "dyadic":
        xy = rng.integers(0, 2400, (c.n, 2)) / 4
        wh = rng.integers(0, 800, (c.n, 2)) / 4
        src = np.concatenate([xy, xy + wh], axis=1).astype(F)
        t = np.concatenate([rng.integers(-12, 13, (c.n, 2)) / 4, np.zeros((c.n, 2))], axis=1).astype(F)
        return src, t
    ctr = rng.uniform(0, (RIGHT, BOTTOM), (c.n, 2))
    ext = np.abs(rng.standard_normal((c.n, 2))) * 100
    src = np.concatenate([ctr - ext / 2, ctr + ext / 2], axis=1).astype(F)
    t = (rng.standard_normal((c.n, 4)) * 0.5).astype(F)
    if c.kind == "specials":
        k = min(len(DECODE_SPECIALS), c.n)
        for i in range(k):
            src[i], t[i] = DECODE_SPECIALS[i]
        if c.n >= 2 * len(DECODE_SPECIALS):
            for i, (a, b) in enumerate(DECODE_SPECIALS):
                src[c.n - len(DECODE_SPECIALS) + i], t[c.n - len(DECODE_SPECIALS) + i] = a, b
    return src, t


# ============================================================================================================================ IoUs
def iou_cont(a, b):
    """bbox.py:66-82 (no + 1), fp32, the tensor operations' order; a, b broadcastable [..., 4]."""
    with np.errstate(all="ignore"):
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), F(0))
        h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), F(0))
        inter = w * h
        return inter / (area_a + area_b - inter)


def iou_incl(a, b):
    """nms.cu:36-49 (+ 1 on every extent), fp32."""
    one = F(1)
    with np.errstate(all="ignore"):
        sa = (a[..., 2] - a[..., 0] + one) * (a[..., 3] - a[..., 1] + one)
        sb = (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one)
        w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + one, F(0))
        h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + one, F(0))
        inter = w * h
        return inter / (sa + sb - inter)


# ====================================================================================================================== assignment
def first_max(v):
    """torch.max along the last axis: the first maximum; a NaN takes over from anything that is not one (so: the first NaN)."""
    nan = np.isnan(v)
    arg = np.where(nan.any(-1), nan.argmax(-1), np.where(nan, -np.inf, v).argmax(-1))
    return np.take_along_axis(v, arg[..., None], -1)[..., 0], arg.astype(I64)


def box_assign(boxes, gt, mode, lo, hi, gt_classes=None):
    """boxes [B, N, 4], gt [B, G, 4] -> (labels [B, N], assign [B, N]) by the RPN's rule (mode 0, region_proposal_network.py:66-82)
    or the head's (mode 1, model.py:256-264).  No ground truth at all: every label -1, every assign 0."""
    boxes, gt = np.asarray(boxes, F), np.asarray(gt, F)
    B, N, G = boxes.shape[0], boxes.shape[1], gt.shape[1]
    labels, assign = np.full((B, N), -1, I64), np.zeros((B, N), I64)
    if G == 0 or B * N == 0:
        return labels, assign
    ious = iou_cont(boxes[:, :, None, :], gt[:, None, :, :])
    best, assign = first_max(ious)
    lo, hi = F(lo), F(hi)
    with np.errstate(invalid="ignore"):
        labels[best < lo] = 0
        if mode == 0:
            gt_max = ious.max(axis=1)                                  # (np.max propagates a NaN, like torch.max)
            tie = ((ious > 0) & (ious == gt_max[:, None, :])).any(-1)
            labels[tie] = 1
            labels[best >= hi] = 1
        else:
            m = best >= lo
            labels[m] = np.take_along_axis(np.asarray(gt_classes, I64), assign, 1)[m]
    return labels, assign


AC = collections.namedtuple("AC", "mode B N G kind")
ASSIGN_SHAPES = [(b, n, g) for b in (1, 3) for n in (1, 255, 257, 513) for g in (0, 1, 3)] + [(b, 300, g) for b in (1, 3) for g in (1024, 1025)]
ASSIGN_CASES = [AC(m, b, n, g, k) for m in (0, 1) for (b, n, g) in ASSIGN_SHAPES for k in ("exact", "gauss")]
LO, HI = 0.25, 0.75
_X = 64.0                     # the planted geometry lives at x >= 64, the random dyadic boxes inside [0, 24)^2
#            ground truth            boxes
PLANT_A = ((_X, 0, _X + 1, 1), [(_X, 0, _X + 4, 1), (_X, 0, _X + 2, 1), (_X, 0, _X + 1, 1)])        # IoU 1/4 (= lo), 1/2, 1
PLANT_B = ((_X, 8, _X + 4, 9), [(_X, 8, _X + 3, 9), (_X, 8, _X + 4, 9)])                            # IoU 3/4 (= hi), 1
PLANT_C = ((200, 200, 201, 201), [])                                                                # disjoint from every box: best IoU 0
PLANT_D = ((_X, 16, _X + 4, 17), [(_X, 16, _X + 2, 17), (_X, 16, _X + 2, 17)])                      # two boxes tie its best, 1/2
PLANT_E = ((_X, 24, _X + 2, 26), [(_X, 24, _X + 2, 26)])                                            # given twice: the first wins
PLANT_Z = ((0, 0, 0, 0), [(0, 0, 0, 0)])                                                            # 0 / 0


def assign_inputs(c):
    """-> boxes [B, N, 4], gt [B, G, 4], gt_classes [B, G], plan (what was planted: {name: (image, gt index, box indices)}).
    exact: quarter-unit boxes, with as much of the planted geometry as the shape holds laid over image 0 (G = 1: the tie pair;
    G = 3: lo / hi / the disjoint ground truth; G >= 8: everything) and, when B > 1, a box with a NaN coordinate in the last image.
    gauss: Gaussian centres and extents, one box in sixteen malformed (right < left)."""
    rng = np.random.default_rng(5000 + 97 * c.B + 13 * c.N + c.G + (0 if c.kind == "exact" else 1))
    B, N, G = c.B, c.N, c.G
    cls = rng.integers(1, 21, (B, G)).astype(I64)
    plan = {}
    if c.kind == "gauss":
        def rnd(n):
            ctr, ext = rng.standard_normal((B, n, 2)) * 8, np.abs(rng.standard_normal((B, n, 2))) * 12
            return np.concatenate([ctr - ext / 2, ctr + ext / 2], axis=2).astype(F)
        boxes, gt = rnd(N), rnd(G)
        bad = rng.random((B, N)) < 1 / 16
        boxes[bad] = boxes[bad][:, [2, 1, 0, 3]]
        return boxes, gt, cls, plan

    def rnd(n):
        xy, wh = rng.integers(0, 64, (B, n, 2)) / 4, rng.integers(1, 33, (B, n, 2)) / 4
        return np.concatenate([xy, xy + wh], axis=2).astype(F)
    boxes, gt = rnd(N), rnd(G)
    plants = {1: [("D", PLANT_D)], 3: [("A", PLANT_A), ("B", PLANT_B), ("C", PLANT_C)]}.get(
        G, [("A", PLANT_A), ("B", PLANT_B), ("C", PLANT_C), ("D", PLANT_D), ("E", PLANT_E), ("E2", (PLANT_E[0], [])), ("Z", PLANT_Z)] if G >= 8 else [])
    gi, bi = 0, 0
    for name, (g, bs) in plants:
        if bi + len(bs) > N:
            continue
        gt[0, gi] = g
        idx = list(range(bi, bi + len(bs)))
        if name == "D" and N - 1 - idx[0] > TB:                       # the second of the tying pair in another workgroup
            idx[1] = N - 1
            bi -= 1
        for i, b in zip(idx, bs):
            boxes[0, i] = b
        plan[name] = (0, gi, idx)
        gi, bi = gi + 1, bi + len(bs)
    if B > 1 and N > 2 and G > 0:
        boxes[B - 1, 1, 0] = NAN
        plan["nan"] = (B - 1, None, [1])
    return boxes, gt, cls, plan


# ========================================================================================================================= sampling
def sample_lists(labels):
    labels = np.asarray(labels, I64)
    return np.flatnonzero(labels > 0).astype(I64), np.flatnonzero(labels == 0).astype(I64)


LISTS_M = (0, 1, 1023, 1024, 1025, 5000)
LISTS_KINDS = ("mixed", "all_fg", "all_bg", "all_ignored")
LC = collections.namedtuple("LC", "M kind")
LISTS_CASES = [LC(m, k) for m in LISTS_M for k in LISTS_KINDS if m > 0 or k == "mixed"]


def lists_inputs(c):
    rng = np.random.default_rng(300 + c.M)
    if c.kind == "mixed":
        return rng.choice(np.array([-1, 0, 1, 7], I64), c.M, p=[0.3, 0.4, 0.2, 0.1])
    return np.full(c.M, {"all_fg": 3, "all_bg": 0, "all_ignored": -1}[c.kind], I64)


def sample_gather(fg, bg, pos, boxes, gt, assign, labels):
    """-> sel, out_boxes, out_labels, out_batch, the two linear target columns in fp32 (bit for bit), the two log columns in
    float64 with their S, and the mask of log entries whose two extents are equal (logf(1) = 0 exactly)."""
    boxes, gt = np.asarray(boxes, F), np.asarray(gt, F)
    B, N, G = boxes.shape[0], boxes.shape[1], gt.shape[1]
    pos = np.asarray(pos, I64)
    flat = np.where(pos >= 0, np.asarray(fg, I64)[np.maximum(pos, 0)], np.asarray(bg, I64)[np.maximum(-pos - 1, 0)])
    b = flat // N
    s = boxes.reshape(-1, 4)[flat]
    d = gt[b, np.asarray(assign, I64).reshape(-1)[flat]]
    two = F(2)
    with np.errstate(all="ignore"):
        scx, scy, sw, sh = (s[:, 0] + s[:, 2]) / two, (s[:, 1] + s[:, 3]) / two, s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
        dcx, dcy, dw, dh = (d[:, 0] + d[:, 2]) / two, (d[:, 1] + d[:, 3]) / two, d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
        lin = np.stack([(dcx - scx) / sw, (dcy - scy) / sh], axis=1).astype(F)
        s64, d64 = s.astype(np.float64), d.astype(np.float64)
        logs = np.log(np.stack([(d64[:, 2] - d64[:, 0]) / (s64[:, 2] - s64[:, 0]), (d64[:, 3] - d64[:, 1]) / (s64[:, 3] - s64[:, 1])], axis=1))
    equal = np.stack([dw == sw, dh == sh], axis=1)
    return flat, s, np.asarray(labels, I64).reshape(-1)[flat], b, lin, logs, 1 + np.abs(logs), equal


GC = collections.namedtuple("GC", "S B N G")
GATHER_CASES = [GC(1, 1, 40, 3), GC(1, 3, 40, 3), GC(257, 1, 300, 5), GC(257, 3, 130, 5)]


def gather_inputs(c):
    """Well-formed Gaussian boxes; every eighth box is a copy of a ground truth of its image, assigned to it (equal extents); the
    lists are the reference's own of labels drawn at random; the last positions sample the last image from both lists."""
    rng = np.random.default_rng(700 + c.S + c.B)
    B, N, G = c.B, c.N, c.G

    def rnd(n):
        ctr, ext = rng.standard_normal((B, n, 2)) * 40 + 100, np.abs(rng.standard_normal((B, n, 2))) * 30 + 1
        return np.concatenate([ctr - ext / 2, ctr + ext / 2], axis=2).astype(F)
    boxes, gt = rnd(N), rnd(G)
    assign = rng.integers(0, G, (B, N)).astype(I64)
    for b in range(B):
        for n in range(0, N, 8):
            boxes[b, n] = gt[b, assign[b, n]]
    labels = rng.choice(np.array([-1, 0, 2, 5], I64), (B, N), p=[0.2, 0.4, 0.2, 0.2])
    copy = (N - 1) // 8 * 8                                             # the last planted copy of a ground truth
    labels[B - 1, N - 1], labels[B - 1, N - 2], labels[B - 1, copy] = 4, 0, 6
    fg, bg = sample_lists(labels.reshape(-1))
    pos = np.where(rng.random(c.S) < 0.5, rng.integers(0, len(fg), c.S), -rng.integers(0, len(bg), c.S) - 1).astype(I64)
    pos[-1] = len(fg) - 1                                               # the last foreground entry: the last image's last box
    if c.S > 2:
        pos[0], pos[1] = -len(bg), int(np.searchsorted(fg, (B - 1) * N + copy))   # the last background entry, the last image's planted copy
    return boxes, gt, assign, labels, fg, bg, pos


# ============================================================================================================================ losses
def det_loss_f64(logits, deltas, rows, gt_labels, gt_deltas, batch, B, C, K, beta, norm):
    """The per-image losses of region_proposal_network.py:163-185 == model.py:343-367 in float64, with the saved unit gradients, the
    denominators and, for each, the S of this module's window.  beta and norm are the fp32 values the kernel is given."""
    S = len(gt_labels)
    r = np.arange(S) if rows is None else np.asarray(rows, I64)
    lab, batch = np.asarray(gt_labels, I64), np.asarray(batch, I64)
    beta = float(F(beta))
    ar = np.arange(S)
    out = {}
    with np.errstate(all="ignore"):
        x = np.asarray(logits, F).astype(np.float64).reshape(-1, C)[r]
        m = x.max(axis=1, keepdims=True) if S else np.zeros((0, 1))
        a = x - m
        fin = np.isfinite(a)
        absa = np.where(fin, np.abs(a), 0.0)
        A = absa.max(axis=1) if S else np.zeros(0)
        lse = np.log(np.exp(a).sum(axis=1))
        t1 = a[ar, lab]
        row = -(t1 - lse)
        s_row = 1 + A + np.abs(t1) + np.abs(lse)
        arg = a - lse[:, None]
        p = np.exp(arg)
        onehot = np.zeros((S, C))
        onehot[ar, lab] = 1
        ul = p - onehot
        s_ul = p * (1 + absa + np.where(fin, np.abs(arg), 0.0) + A[:, None] + np.abs(lse)[:, None]) + np.abs(ul)
        t = np.asarray(gt_deltas, F).astype(np.float64).reshape(S, 4)
        if norm is not None:
            nm = np.asarray(norm, F).astype(np.float64)
            t = (t - nm[:4]) / nm[4:]
        inp = np.asarray(deltas, F).astype(np.float64).reshape(-1, K, 4)[r, 0 if K == 1 else lab]
        e = inp - t
        d = np.abs(e)
        f = np.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
        acc = f.sum(axis=1)
        s_acc = (np.abs(inp) + np.abs(t)).sum(axis=1) + acc
        fg = lab != 0
        u = np.where(fg[:, None], np.where(d < beta, e / beta, np.sign(e)), 0.0)
        s_u = np.where(fg[:, None], (np.abs(inp) + np.abs(t)) / beta + np.abs(u), 0.0)
        ce, s_ce, sl, s_sl, chain, dn64 = (np.zeros(B) for _ in range(6))
        denom = np.zeros((B, 2), F)
        for b in range(B):
            idx = batch == b
            cnt, nfg = int(idx.sum()), int((idx & fg).sum())
            dn = dn64[b] = 4.0 * nfg + 1e-8
            ce[b], s_ce[b] = row[idx].sum() / cnt if cnt else np.nan, s_row[idx].sum() / cnt if cnt else np.nan
            sl[b], s_sl[b] = acc[idx & fg].sum() / dn, s_acc[idx & fg].sum() / dn
            chain[b] = np.bincount(np.flatnonzero(idx) % TB, minlength=1).max() if cnt else 1
            denom[b] = F(cnt), F(F(4) * F(nfg) + F(1e-8))
    out.update(ce=ce, s_ce=s_ce, sl=sl, s_sl=s_sl, chain=chain, ul=ul, s_ul=s_ul, u=u, s_u=s_u, denom=denom, dn=dn64, rows=r, fg=fg)
    return out


def det_loss_bwd_f64(fwd, g_ce, g_sl, gt_labels, batch, C, K, R):
    """-> d_logits [R, C], d_deltas [R, K, 4] with their S and the mask of the elements a sample owns (all others: exactly zero)."""
    lab, batch, r = np.asarray(gt_labels, I64), np.asarray(batch, I64), fwd["rows"]
    S = len(lab)
    dl, s_dl, dd, s_dd = np.zeros((R, C)), np.zeros((R, C)), np.zeros((R, K, 4)), np.zeros((R, K, 4))
    own_l, own_d = np.zeros((R, C), bool), np.zeros((R, K, 4), bool)
    if S == 0:
        return dl, s_dl, own_l, dd, s_dd, own_d, np.zeros(0)
    with np.errstate(all="ignore"):
        kc = np.asarray(g_ce, F).astype(np.float64)[batch] / fwd["denom"][batch, 0].astype(np.float64)
        ks = np.asarray(g_sl, F).astype(np.float64)[batch] / fwd["dn"][batch]
        dl[r], s_dl[r], own_l[r] = fwd["ul"] * kc[:, None], fwd["s_ul"] * np.abs(kc)[:, None], True
        k = np.zeros(S, I64) if K == 1 else lab
        dd[r, k], s_dd[r, k], own_d[r, k] = fwd["u"] * ks[:, None], fwd["s_u"] * np.abs(ks)[:, None], True
    return dl, s_dl, own_l, dd, s_dd, own_d, np.abs(kc)


def sl1_exact_f32(deltas, rows, gt_labels, gt_deltas, batch, B, K, beta, g_sl, R):
    """The smooth-L1 side of the exact table in fp32: every e is one of {0, +-beta / 2, +-beta, +-2 beta} with a dyadic beta, so each
    term and every partial sum is exact (asserted) and the only roundings are sl / dn, g / dn and u * (g / dn), one operation each."""
    S = len(gt_labels)
    r = np.arange(S) if rows is None else np.asarray(rows, I64)
    lab, batch, beta = np.asarray(gt_labels, I64), np.asarray(batch, I64), F(beta)
    inp = np.asarray(deltas, F).reshape(-1, K, 4)[r, 0 if K == 1 else lab]
    e = inp - np.asarray(gt_deltas, F).reshape(S, 4)
    d = np.abs(e)
    f = np.where(d < beta, F(0.5) * (d * d) / beta, d - F(0.5) * beta).astype(F)
    fg = lab != 0
    u = np.where(fg[:, None], np.where(d < beta, e / beta, np.sign(e)), F(0)).astype(F)
    sl, dd = np.zeros(B, F), np.zeros((R, K, 4), F)
    for b in range(B):
        idx = (batch == b) & fg
        tot = float(f[idx].astype(np.float64).sum())
        q = float(beta) / 8                                                # every term is a multiple of beta / 8: sums below 2^24 of them are exact in any order
        assert bool(((f[idx].astype(np.float64) / q) % 1 == 0).all()) and tot / q < 2 ** 24 and float(F(tot)) == tot
        dn = F(F(4) * F(idx.sum()) + F(1e-8))
        sl[b] = F(tot) / dn
        ks = F(np.asarray(g_sl, F)[b]) / dn
        dd[r[idx], 0 if K == 1 else lab[idx]] = u[idx] * ks
    return sl, u, dd


LSC = collections.namedtuple("LSC", "S B C K beta rows norm kind")
BETAS = (1.0, 0.5, 1.0 / 9)
LOSS_S = (0, 1, 255, 256, 257, 600)
LOSS_CASES = []
for _i, (_s, _b, (_c, _k)) in enumerate([(s, b, ck) for s in LOSS_S for b in (1, 3) for ck in ((2, 1), (21, 21))]):
    for _j, _beta in enumerate(BETAS):
        LOSS_CASES.append(LSC(_s, _b, _c, _k, _beta, ("null", "perm")[(_i + _j) % 2], ("null", "given")[((_i + _j) // 2) % 2], "gauss"))
LOSS_CASES += [LSC(s, b, c, k, beta, rows, "null", "exact") for s in (1, 257, 600) for b in (1, 3) for (c, k) in ((2, 1), (21, 21))
               for beta, rows in ((1.0, "perm"), (0.5, "null"))]
LOSS_NORM = np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.1, 0.2, 0.2], F)


def loss_inputs(c):
    """Gaussian logits x 3, with a row of magnitude 80 and a row holding -inf in a class that is not its target; with B = 3 image 1
    has no sample and image 2 no foreground.  rows = perm: R = S + 7 and rows a permutation's first S.  exact: deltas = targets + e,
    e drawn from {0, +-beta / 2, +-beta, +-2 beta}, targets and gradients dyadic."""
    rng = np.random.default_rng(900 + c.S * 7 + c.B * 3 + c.C + int(c.beta * 90) + (c.rows == "perm") + 2 * (c.norm == "given") + 4 * (c.kind == "exact"))
    S, B, C, K = c.S, c.B, c.C, c.K
    R = S + 7 if c.rows == "perm" else S
    rows = rng.permutation(R)[:S].astype(I64) if c.rows == "perm" else None
    r = np.arange(S) if rows is None else rows
    batch = (rng.integers(0, 2, S) * 2 if B == 3 else np.zeros(S)).astype(I64)
    lab = rng.integers(0, C, S).astype(I64)
    lab[batch == 2] = 0
    logits = (rng.standard_normal((R, C)) * 3).astype(F)
    if S >= 2:
        logits[r[0]] = np.where(rng.random(C) < 0.5, 80, -80).astype(F)
        logits[r[1], (lab[1] + 1) % C] = -np.inf
    beta = F(c.beta)
    if c.kind == "exact":
        gt_deltas = (rng.integers(-8, 9, (S, 4)) / 4).astype(F)
        deltas = (rng.integers(-8, 9, (R, K, 4)) / 4).astype(F)
        e = rng.choice(np.array([0, 0.5, -0.5, 1, -1, 2, -2], F), (S, 4)) * beta
        deltas[r, 0 if K == 1 else lab] = gt_deltas + e.astype(F)
        g_ce, g_sl = (rng.integers(1, 9, B) / 4).astype(F), (rng.integers(1, 9, B) / 4).astype(F)
    else:
        gt_deltas, deltas = rng.standard_normal((S, 4)).astype(F), rng.standard_normal((R, K, 4)).astype(F)
        if c.norm == "given":
            gt_deltas = (gt_deltas * 0.15).astype(F)
        if S >= 4:                                                        # |e| == beta and e == 0 exactly, on a foreground row
            lab[3] = max(int(lab[3]), 1) if batch[3] != 2 else 0
            k3 = 0 if K == 1 else lab[3]
            if c.norm == "null":
                deltas[r[3], k3] = gt_deltas[3] + np.array([beta, -beta, 0, 0], F)
        g_ce, g_sl = rng.uniform(0.5, 2, B).astype(F), rng.uniform(0.5, 2, B).astype(F)
    norm = LOSS_NORM if c.norm == "given" else None
    return dict(logits=logits, deltas=deltas, rows=rows, labels=lab, gt_deltas=gt_deltas, batch=batch, R=R, beta=beta, norm=norm, g_ce=g_ce, g_sl=g_sl)


# ================================================================================================================ class NMS and pack
def greedy_nms(boxes, order, thresh):
    """nms.cu: walk `order`; a row that is still alive strikes every later row whose inclusive IoU with it exceeds thresh.  -> kept
    original indices, ascending."""
    boxes = np.asarray(boxes, F)
    order = np.asarray(order, I64)
    alive = np.ones(len(order), bool)
    for i in range(len(order)):
        if not alive[i]:
            continue
        rest = order[i + 1:]
        with np.errstate(invalid="ignore"):
            alive[i + 1:] &= ~(iou_incl(boxes[order[i]][None, :], boxes[rest]) > F(thresh))
    return np.sort(order[alive])


def det_class_nms(proposals, transformers, probs, norm, right, bottom, thresh, min_prob):
    """model.py:369-407 per (image, class >= 1) list -> out_boxes [L, N, 4], out_probs [L, N], counts [L], written [L, N] and the mask
    `known` [L] of lists all of whose boxes are bit-for-bit known (see decode_clip_f32)."""
    proposals, transformers, probs, norm = np.asarray(proposals, F), np.asarray(transformers, F), np.asarray(probs, F), np.asarray(norm, F)
    B, N, C = probs.shape
    L = B * (C - 1)
    ob, op, counts = np.zeros((L, N, 4), F), np.zeros((L, N), F), np.zeros(L, I64)
    known = np.zeros(L, bool)
    for b in range(B):
        for c in range(1, C):
            l = b * (C - 1) + c - 1
            t = transformers[b, :, c] * norm[4:]
            t = t + norm[:4]
            box, kn = decode_clip_f32(proposals[b], t, right, bottom)
            p = probs[b, :, c]
            idx = np.arange(N) if min_prob < 0 else np.flatnonzero(p > F(min_prob))
            order = idx[np.lexsort((idx, -p[idx]))]                       # descending probability, ties by ascending proposal index
            keep = greedy_nms(box, order, thresh)
            known[l] = kn.all()
            counts[l] = len(keep)
            ob[l, :len(keep)], op[l, :len(keep)] = box[keep], p[keep]
    return ob, op, counts, known


def det_pack(boxes, probs, counts, total):
    """What det_pack_kernel does, out-of-range counts included: list l copies its first clamp(counts[l], 0, N) rows to
    sum(counts[:l]) — the offset adds the counts as they are.  -> flat_boxes [total, 4], flat_probs [total], written [total]."""
    boxes, probs, counts = np.asarray(boxes, F), np.asarray(probs, F), np.asarray(counts, I64)
    L, N = probs.shape
    fb, fp, wr = np.zeros((total, 4), F), np.zeros(total, F), np.zeros(total, bool)
    for l in range(L):
        off, n = int(counts[:l].sum()), int(min(max(counts[l], 0), N))
        assert n == 0 or (0 <= off and off + n <= total and not wr[off:off + n].any()), "the table keeps every write in range and disjoint"
        fb[off:off + n], fp[off:off + n], wr[off:off + n] = boxes[l, :n], probs[l, :n], True
    return fb, fp, wr


NC = collections.namedtuple("NC", "B N C kind")
NMS_SHAPES = [(1, 1, 2), (1, 2, 3), (1, 255, 3), (1, 256, 3), (1, 257, 3), (2, 300, 21), (1, 2048, 2), (5, 64, 64)]
NMS_CASES = [NC(b, n, c, k) for (b, n, c) in NMS_SHAPES for k in ("ties", "gauss")] + [NC(1, 1, 2, "nan"), NC(1, 300, 3, "all")]
NMS_NORM = np.array([0.25, -0.5, 0.0, 0.0, 0.1, 0.1, 0.2, 0.2], F)
NMS_THRESH, NMS_MIN_PROB = 0.3, 0.25


def nms_inputs(c):
    """The z / w transformers are 0 (decode exact).  ties: probabilities on the grid k / 8 with a block of exactly 1.0 and rows exactly on
    min_prob; class 1 of image 0 at or below min_prob when N > 2 and C > 2 (an empty list); identical boxes, boxes clipped to zero width.
    gauss: distinct Gaussian probabilities.  nan: one box with a NaN transformer.  all: min_prob < 0."""
    rng = np.random.default_rng(1100 + c.B + c.N * 3 + c.C * 5 + len(c.kind))
    B, N, C = c.B, c.N, c.C
    ctr = rng.uniform(0, (RIGHT, BOTTOM), (B, N, 2))
    ext = np.abs(rng.standard_normal((B, N, 2))) * 120 + 2
    prop = np.concatenate([ctr - ext / 2, ctr + ext / 2], axis=2).astype(F)
    for n in range(3, N, 5):
        prop[:, n] = prop[:, n - 2]                                        # identical proposals
    for n in range(4, N, 11):
        prop[:, n, [0, 2]] = (RIGHT + 50, RIGHT + 90)                      # beyond the right edge: clipped to zero width
    t = np.zeros((B, N, C, 4), F)
    t[..., :2] = (rng.standard_normal((B, N, C, 2)) * 0.8).astype(F)
    for n in range(3, N, 5):
        t[:, n] = t[:, n - 2]                                              # ... with identical transformers: identical boxes
    if c.kind in ("gauss", "all"):
        probs = rng.random((B, N, C)).astype(F)
    else:
        probs = (rng.integers(0, 9, (B, N, C)) / 8).astype(F)
        probs[:, N // 3: N // 3 + 40] = 1.0
        if N > 2 and C > 2:
            probs[0, :, 1] = np.minimum(probs[0, :, 1], F(NMS_MIN_PROB))
    if c.kind == "nan":
        t[0, 0, 1, 0], probs[0, 0, 1] = np.nan, 0.5
    return prop, t, probs, (-1.0 if c.kind == "all" else NMS_MIN_PROB)


PC = collections.namedtuple("PC", "L N kind")
PACK_CASES = [PC(1, 1, "full"), PC(5, 7, "zeros"), PC(5, 7, "full"), PC(300, 3, "mixed"), PC(6, 5, "out_of_range")]


def pack_inputs(c):
    rng = np.random.default_rng(1300 + c.L + c.N)
    boxes, probs = rng.standard_normal((c.L, c.N, 4)).astype(F), rng.random((c.L, c.N)).astype(F)
    counts = {"full": np.full(c.L, c.N), "zeros": np.zeros(c.L), "mixed": rng.integers(0, c.N + 1, c.L),
              # a count above N advances the offset by itself and copies N rows; a negative one copies nothing and moves the offset back
              "out_of_range": np.array([2, c.N + 4, -2, 1, 0, -7])}[c.kind].astype(I64)
    off, n = np.cumsum(np.concatenate([[0], counts[:-1]])), np.clip(counts, 0, c.N)
    total = int(((off + n) * (n > 0)).max())                               # the end of the last row any list copies
    return boxes, probs, counts, total


# ====================================================================================================================== small entries
def proposal_rows(cand, n_cand, keep, n_keep, count, P):
    """rows[j] = cand[clamp(keep[j], 0, n_cand - 1)] for j < min(max(count, 0), P, n_keep) (nothing to read with n_cand = 0), zero rows behind."""
    c = int(min(max(int(count), 0), P, n_keep))
    rows = np.zeros((P, 4), F)
    if n_cand > 0 and c > 0:
        rows[:c] = np.asarray(cand, F).reshape(-1, 4)[np.clip(np.asarray(keep, I64)[:c], 0, n_cand - 1)]
    return rows, c


PRC = collections.namedtuple("PRC", "P n_cand n_keep count")
PROPOSAL_ROWS_CASES = [PRC(p, 50, 40, cnt) for p in (1, 255, 257) for cnt in (-3, 0, 1, 30)] + \
                      [PRC(255, 400, 300, 1000), PRC(257, 400, 300, 280), PRC(257, 400, 300, 300), PRC(257, 400, 300, 301),
                       PRC(257, 400, 256, 999), PRC(255, 0, 40, 30), PRC(1, 50, 0, 5)]


def proposal_rows_inputs(c):
    rng = np.random.default_rng(1500 + c.P + c.n_cand + c.n_keep)
    cand = rng.standard_normal((max(c.n_cand, 1), 4)).astype(F)
    keep = rng.integers(0, max(c.n_cand, 1), max(c.n_keep, 1)).astype(I64)
    keep[:3] = (-5, c.n_cand + 9, max(c.n_cand - 1, 0))[:len(keep[:3])]
    return cand, keep


def labels_limit(labels, kept):
    labels = np.array(labels, I64)
    labels[:, int(np.max(kept)):] = -1
    return labels


LLC = collections.namedtuple("LLC", "B N kept")
LABELS_LIMIT_CASES = [LLC(1, 300, (120,)), LLC(3, 300, (7, 256, 40)), LLC(3, 257, (0, 0, 0)), LLC(1, 5, (0,)), LLC(1, 5, (5,)),
                      LLC(3, 257, (257, 1, 2)), LLC(3, 90, (3, 2, 89))]


def sum_scalars(a, b, c=None, d=None):
    s = F(a) + F(b)
    if c is not None:
        s = s + F(c)
    if d is not None:
        s = s + F(d)
    return F(s)


SUM_CASES = [(2, "gauss"), (3, "gauss"), (4, "gauss"), (4, "order"), (3, "nan")]


def sum_inputs(n, kind):
    if kind == "order":                                                    # ((a + b) + c) + d differs from every other association
        return [F(1.0), F(2.0 ** -24), F(2.0 ** -24), F(-1.0)][:n]
    v = list(np.random.default_rng(n).standard_normal(4).astype(F) * F(3))[:n]
    if kind == "nan":
        v[1] = NAN
    return v


# =========================================================================================================================== coverage
SOURCES = ("cv_a-fan_amd/csrc/afan_det_targets.hip", "cv_a-fan_amd/csrc/afan_det_eval.hip")
TABLES = {
    "afan_box_decode_clip": DECODE_CASES, "afan_box_assign": ASSIGN_CASES, "afan_sample_lists": LISTS_CASES,
    "afan_sample_gather": GATHER_CASES, "afan_det_loss_fwd": LOSS_CASES, "afan_det_loss_bwd": LOSS_CASES,
    "afan_sum_scalars_f32": SUM_CASES, "afan_proposal_rows": PROPOSAL_ROWS_CASES, "afan_labels_limit": LABELS_LIMIT_CASES,
    "afan_det_class_nms_supported": [(1, 2), (2048, 64), (0, 2), (2049, 2), (1, 1), (1, 65)], "afan_det_class_nms": NMS_CASES,
    "afan_det_pack": PACK_CASES,
}


def exports_of(text):
    """The names the extern "C" blocks of a source file define."""
    return re.findall(r"^(?:int|int64_t)\s+(afan_\w+)\(", text, flags=re.M)
