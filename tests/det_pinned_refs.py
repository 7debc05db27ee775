"""Float64 references of the Faster-RCNN kernels with no elementwise pin of their own: ROIAlign (csrc/afan_det.hip) forward and
backward as dense per-axis matrices, and the two-layers-on-one-input linear product (csrc/afan_linear.hip), with the operand
tables of the exact and the rounding-aware checks.  tests/test_det_pinned_gpu.py holds the kernels to these;
tests/test_det_pinned_ref.py checks them on the CPU against the fp32 C oracle and the torch restatement.  Nothing here reads the
kernels or ops.py.

ROIAlign (legacy, un-aligned: Detection/support/src/cuda/ROIAlign_cuda.cu).  The GEOMETRY is evaluated in np.float32, operation by
operation, in the order the definition states it (the library is built without contraction, so this is reproducible):
    start = roi * scale;  r = max(end - start, 1);  bin = r / P;  grid = sampling_ratio > 0 ? sampling_ratio : ceil(r / P)
    t = start + p * bin + (i + .5f) * bin / grid            sample i of bin p
    valid = !(t < -1 || t > size);  t <= 0 -> 0;  lo = int(t);  lo >= size - 1 -> lo = hi = size - 1, t = lo;  l = t - lo;  h = 1 - l
Everything after it is float64: validity and the clamps act per axis, so one ROI is two dense matrices Ay [PH, H], Ax [PW, W]
(A[p, lo] += h, A[p, hi] += l over the bin's valid samples, fp32 values held in float64) and
    y = Ay x[b] Ax^T / count,        dx[b] += Ay^T dy Ax / count,        count = grid_h * grid_w."""
import collections

import numpy as np
import torch

U = 2.0 ** -24                      # half an ulp of 1.0f: the unit of one fp32 rounding
F = np.float32

Axis = collections.namedtuple("Axis", "A N grid t valid")


def roi_axis(start_px, end_px, scale, P, size, sampling_ratio):
    """One axis of every ROI.  A [R, P, size] float64 weights; N [R, P, size] the number of non-zero contributions behind each entry;
    grid [R]; t [R, P, G] the fp32 sample coordinates (before the clamps) and valid [R, P, G] (False past a ROI's own grid)."""
    start_px, end_px = np.asarray(start_px, F), np.asarray(end_px, F)
    n = len(start_px)
    s = start_px * F(scale)
    e = end_px * F(scale)
    r = np.maximum(e - s, F(1))
    b = r / F(P)
    grid = np.full(n, sampling_ratio, np.int64) if sampling_ratio > 0 else np.ceil(r / F(P)).astype(np.int64)
    G = int(grid.max()) if n else 1
    p = np.arange(P, dtype=F)[None, :, None]
    i = np.arange(G, dtype=F)[None, None, :]
    s3, b3, g3 = s[:, None, None], b[:, None, None], grid.astype(F)[:, None, None]
    t = (s3 + p * b3) + ((i + F(.5)) * b3) / g3
    assert t.dtype == F
    live = np.broadcast_to(np.arange(G)[None, None, :] < grid[:, None, None], t.shape)
    valid = live & ~((t < F(-1)) | (t > F(size)))
    tc = np.where(valid, t, F(0))
    tc = np.where(tc <= 0, F(0), tc)
    lo = tc.astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    tc = np.where(top, lo.astype(F), tc)
    l = (tc - lo.astype(F)).astype(F)
    h = (F(1) - l).astype(F)
    A = np.zeros((n, P, size), np.float64)
    N = np.zeros((n, P, size), np.int64)
    ri = np.broadcast_to(np.arange(n)[:, None, None], t.shape)
    pi = np.broadcast_to(np.arange(P)[None, :, None], t.shape)
    for idx, w in ((lo, h), (hi, l)):
        w = np.where(valid, w, F(0)).astype(np.float64)
        np.add.at(A, (ri, pi, idx), w)
        np.add.at(N, (ri, pi, idx), (w != 0).astype(np.int64))
    return Axis(A, N, grid, t, valid)


Geom = collections.namedtuple("Geom", "batch y x count")


def roi_geom(rois, scale, ph, pw, h, w, sampling_ratio):
    rois = np.asarray(rois, F)
    ay = roi_axis(rois[:, 2], rois[:, 4], scale, ph, h, sampling_ratio)
    ax = roi_axis(rois[:, 1], rois[:, 3], scale, pw, w, sampling_ratio)
    return Geom(rois[:, 0].astype(np.int64), ay, ax, (ay.grid * ax.grid).astype(np.float64))


def roi_align_fwd(x, g):
    """x [N, C, H, W] float64 (torch) -> (y [R, C, PH, PW], S = the same map of |x|, K [R, PH, PW] = the number of samples with a
    non-zero tap that each output sums)."""
    ay, ax, cnt = torch.from_numpy(g.y.A), torch.from_numpy(g.x.A), torch.from_numpy(g.count)
    r, c = len(g.batch), x.shape[1]
    y = torch.zeros((r, c, ay.shape[1], ax.shape[1]), dtype=torch.float64)
    s = torch.zeros_like(y)
    for b in np.unique(g.batch):
        m = torch.from_numpy(g.batch == b)
        f = lambda v: torch.einsum("rcpw,rqw->rcpq", torch.einsum("rph,chw->rcpw", ay[m], v), ax[m]) / cnt[m].view(-1, 1, 1, 1)
        y[m], s[m] = f(x[b]), f(x[b].abs())
    ny, nx = g.y.valid.sum(2), g.x.valid.sum(2)               # [R, P]: a valid sample has a non-zero tap (h + l = 1)
    return y, s, torch.from_numpy(ny[:, :, None] * nx[:, None, :])


def roi_align_bwd(dy, g, n):
    """dy [R, C, PH, PW] float64 (torch) -> (dx [n, C, H, W], S = the same map of |dy|, K_scatter [n, H, W] = the number of non-zero
    (sample, corner) terms arriving at a cell, K_gather [n, H, W] = the number of non-zero (ROI, ph, pw) terms of the separable form)."""
    ay, ax, cnt = torch.from_numpy(g.y.A), torch.from_numpy(g.x.A), torch.from_numpy(g.count)
    c, h, w = dy.shape[1], ay.shape[2], ax.shape[2]
    dx = torch.zeros((n, c, h, w), dtype=torch.float64)
    s = torch.zeros_like(dx)
    ks, kg = np.zeros((n, h, w), np.int64), np.zeros((n, h, w), np.int64)
    for b in np.unique(g.batch):
        m = torch.from_numpy(g.batch == b)
        f = lambda v: torch.einsum("rph,rcpw->chw", ay[m], torch.einsum("rcpq,rqw->rcpw", v / cnt[m].view(-1, 1, 1, 1), ax[m]))
        dx[b], s[b] = f(dy[m]), f(dy[m].abs())
        mm = g.batch == b
        ks[b] = np.einsum("rh,rw->hw", g.y.N[mm].sum(1), g.x.N[mm].sum(1))
        kg[b] = np.einsum("rh,rw->hw", (g.y.A[mm] != 0).sum(1), (g.x.A[mm] != 0).sum(1))
    return dx, s, torch.from_numpy(ks), torch.from_numpy(kg)


def axis_terms(a):
    """The largest number of non-zero sample contributions summed into one entry of an axis matrix."""
    return int(a.N.max()) if a.N.size else 0


def overlaps(g):
    """[R] bool: the ROI has at least one sample that is valid on both axes."""
    return (g.y.A != 0).any((1, 2)) & (g.x.A != 0).any((1, 2))


def edge_samples(a, size):
    """(samples exactly at -1, samples exactly at size) among the valid samples of an axis."""
    return int((a.valid & (a.t == F(-1))).sum()), int((a.valid & (a.t == F(size))).sum())


def gather_paths(g, tile_w=4):
    """How a gather by (ROI, map row, tile of `tile_w` columns) meets the bins, from the non-zero ranges of Ay / Ax alone: (number of
    such triples whose bin ranges span fewer than 3 bins on the row and on every column of the tile, number of the others)."""
    def span(a):                                        # [R, size]: last - first non-zero bin, -1 where none
        nz = a.A != 0
        p = np.arange(a.A.shape[1])[None, :, None]
        first = np.where(nz, p, 10 ** 6).min(1)
        last = np.where(nz, p, -1).max(1)
        return np.where(last >= 0, last - first, -1)
    sy, sx = span(g.y), span(g.x)
    w = sx.shape[1]
    pad = (-w) % tile_w
    sxt = np.pad(sx, ((0, 0), (0, pad)), constant_values=-1).reshape(len(sx), -1, tile_w).max(2)      # [R, tiles]
    rows, tiles = sy[:, :, None], sxt[:, None, :]
    met = (rows >= 0) & (tiles >= 0)
    small = met & (rows < 3) & (tiles < 3)
    return int(small.sum()), int((met & ~small).sum())


# ---------------------------------------------------------------------------------------------------------------- the ROI tables
BINS = (0.25, 0.5, 1.0, 2.0, 4.0)


def exact_rois(r, n, h, w, ph, pw, seed, sampling_ratio=0, scale_inv=16, bins=BINS, corner=False):
    """ROIs on which every fp32 operation of every form is exact: starts on multiples of 1/8 cell from 3 cells outside the map to 2
    cells past its far edge, extents bin * P cells with bin in BINS (the adaptive grid is then 1, 1, 1, 2 or 4).  The first four
    rows are placed: their first sample lies exactly on -1 (rows 0 and 2, bins of 4 and 1 cells) and a sample of their second or
    third bin exactly on the map's size (rows 1 and 3), on both axes.  corner: the ROIs stay within the first 7 cells of image 0
    (other tiles are then reached by no ROI)."""
    rng = np.random.default_rng(seed)
    rois = np.zeros((r, 5), F)
    rois[:, 0] = (np.arange(r) % n) if not corner else 0
    rng.shuffle(rois[4:, 0])
    for k, (size, p) in enumerate(((w, pw), (h, ph))):
        lo, hi = (-3 * 8, (size + 2) * 8) if not corner else (0, 2 * 8)
        start = rng.integers(lo, hi + 1, r).astype(np.float64) / 8.0
        b = np.asarray(bins)[rng.integers(0, len(bins) if not corner else 2, r)]
        if not corner and r >= 4:
            for row, (bb, pp) in enumerate(((4.0, None), (4.0, 1), (1.0, None), (1.0, 2))):
                first = 0.5 * bb / (sampling_ratio if sampling_ratio > 0 else int(np.ceil(bb)))
                b[row], start[row] = bb, (-1.0 - first) if pp is None else (size - first - bb * pp)
        rois[:, 1 + k] = start * scale_inv
        rois[:, 3 + k] = (start + b * p) * scale_inv
    return rois


def gauss_rois(r, n, h, w, ph, pw, seed, scale_inv=16, corner=False):
    """Random ROIs in image coordinates, by index modulo 6: plain boxes; bins below one cell (extent below P cells); extents of exactly
    m * P cells (r / P an integer: the edge of the adaptive grid's ceil); malformed (end < start); entirely outside the map; boxes
    over the far border.  corner: small boxes within the first 6 cells of image 0."""
    rng = np.random.default_rng(seed)
    rois = np.zeros((r, 5), F)
    rois[:, 0] = (np.arange(r) % n) if not corner else 0
    rng.shuffle(rois[:, 0])
    kind = np.arange(r) % 6
    for k, (size, p) in enumerate(((w, pw), (h, ph))):
        px = size * scale_inv
        start = rng.uniform(-1.5 * scale_inv, px - scale_inv, r)
        ext = rng.uniform(0.3 * p, 1.6 * p, r) * scale_inv * rng.uniform(0.5, 1.0, r)
        ext = np.where(kind == 1, rng.uniform(0.15, 0.9, r) * p * scale_inv, ext)
        start = np.where(kind == 2, np.round(start), start)
        ext = np.where(kind == 2, rng.integers(1, 3, r) * p * scale_inv, ext)
        ext = np.where(kind == 3, -rng.uniform(1, 40, r), ext)
        start = np.where(kind == 4, rng.choice([-1.0, 1.0], r) * 10 * px + px / 2 + start, start)
        start = np.where(kind == 5, px - rng.uniform(0, 0.6 * p * scale_inv, r), start)
        if corner:
            start, ext = rng.uniform(-8, 2.0 * scale_inv, r), rng.uniform(0.15, 0.5, r) * p * scale_inv
        rois[:, 1 + k] = start
        rois[:, 3 + k] = start + ext
    return rois


def dyadic_bits(a):
    """The smallest k with a * 2^k integer everywhere (a float64 array of dyadic values)."""
    k = 0
    while not np.array_equal(np.round(a * 2.0 ** k), a * 2.0 ** k):
        k += 1
        assert k <= 60, "not dyadic"
    return k


def exact_range_ok(g, s_max):
    """Every term of a form is a multiple of 2^-k (k: both axes' weight bits and the division by count, a power of two) and the sum
    of the terms' absolute values stays below 2^(24 - k): every partial sum, in any order, is an fp32 value.  -> (ok, k)."""
    cnt = g.count
    assert np.array_equal(2.0 ** np.round(np.log2(cnt)), cnt), "count is not a power of two"
    k = dyadic_bits(g.y.A) + dyadic_bits(g.x.A) + int(np.log2(cnt.max()))
    return bool(s_max < 2.0 ** (24 - k)), k


# -------------------------------------------------------------------------------------------------------------- bf16 and windows
def rne_bf16(ref):
    """float64 (torch) -> the nearest bf16 (ties to even), decided on the float64 value itself (no double rounding through fp32)."""
    f = ref.float()
    bits = f.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    low, up = bits & 0xffff, (bits >> 16) & 1
    rounded = (bits + 0x7fff + up) >> 16
    tie = low == 0x8000
    away, toward = ref.abs() > f.double().abs(), ref.abs() < f.double().abs()
    rounded = torch.where(tie & away, (bits >> 16) + 1, rounded)
    rounded = torch.where(tie & toward, bits >> 16, rounded)
    out = (rounded << 16) & 0xffffffff
    out = torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)
    return out.view(torch.float32).to(torch.bfloat16)


def bf16_edges(got):
    """The closed real interval that rounds (to nearest, ties either way) to each bf16 element of got."""
    b = got.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag, neg = b & 0x7fff, (b >> 15) == 1
    val = lambda mm: (mm << 16).contiguous().view(torch.float32).double()
    v, up, dn = val(mag), val(mag + 1), val((mag - 1).clamp_min(0))
    hi_m = (v + up) / 2
    lo_m = torch.where(mag > 0, (v + dn) / 2, -up / 2)
    return torch.where(neg, -hi_m, lo_m), torch.where(neg, -lo_m, hi_m)


def midpoint_share(ref, noise):
    """The share of elements whose window ref +- noise holds a bf16 rounding midpoint (where either neighbour is accepted)."""
    return float((rne_bf16(ref - noise).view(torch.int16) != rne_bf16(ref + noise).view(torch.int16)).double().mean())


# ------------------------------------------------------------------------------------------------------------- the linear pair
def linear_pair(x, w1, b1, w2, b2):
    """y_i = x w_i^T + b_i -> (y1, S1, y2, S2) with S = |x| |w|^T + |b|."""
    out = []
    for w, b in ((w1, b1), (w2, b2)):
        y, s = x @ w.t(), x.abs() @ w.abs().t()
        out += [y, s] if b is None else [y + b, s + b.abs()]
    return out


def linear_pair_grads(g1, g2, x, w1, w2):
    """(gx, S_gx, [(gw_i, S_gw_i, gb_i, S_gb_i)])."""
    gx, sx = g1 @ w1 + g2 @ w2, g1.abs() @ w1.abs() + g2.abs() @ w2.abs()
    return gx, sx, [(g.t() @ x, g.abs().t() @ x.abs(), g.sum(0), g.abs().sum(0)) for g in (g1, g2)]


def ints(shape, amp, gen):
    return torch.randint(-amp, amp + 1, tuple(shape), generator=gen).double()


def ternary(shape, gen):
    return ints(shape, 1, gen)
