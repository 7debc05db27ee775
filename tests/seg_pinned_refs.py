"""Float64 references of the DeepLab layer kernels (csrc/afan_seg.hip), written from each operation's definition: bilinear resize
(align_corners=False) and its adjoint as dense per-axis matrices, per-pixel cross-entropy with ignore_index, max pooling with the
"first maximum in scan order, NaN wins" rule and the winner's position byte, global average pooling, the pointwise classifier, the
small linear layer and dropout with a host mask.  tests/test_seg_pinned_gpu.py holds the kernels to these;
tests/test_seg_pinned_ref.py checks them against torch in float64 on the CPU.  Nothing here reads the kernels or ops.py."""
import numpy as np
import torch

U = 2.0 ** -24                      # half an ulp of 1.0f: the unit of one fp32 rounding


# ------------------------------------------------------------------------------------------------------------------ bilinear resize
def axis_table(n_in, n_out):
    """The header's index rule, evaluated in fp32: src = max(0, scale * (dst + 0.5) - 0.5), scale = fl32(in) / fl32(out),
    i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.  Returns (i0, i1, l0, l1, src) with fp32 weights.
    (The product-and-subtract is taken with one rounding, as a fused multiply-add gives it: float64 holds the 48-bit product exactly.)"""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32) + np.float32(0.5)
    src = (np.float64(scale) * dst.astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    return i0, i1, l0, l1, src


def axis_matrix(n_in, n_out):
    """W [n_out, n_in] float64 with W[o, i0] += l0, W[o, i1] += l1: one axis of the resize as a dense linear map."""
    i0, i1, l0, l1, _ = axis_table(n_in, n_out)
    w = np.zeros((n_out, n_in), np.float64)
    o = np.arange(n_out)
    np.add.at(w, (o, i0), l0.astype(np.float64))
    np.add.at(w, (o, i1), l1.astype(np.float64))
    return w


def axis_src_ulp(n_in, n_out):
    """One fp32 ulp of src per output index: what a differently rounded src moves the two weights by."""
    src = axis_table(n_in, n_out)[4]
    return (np.nextafter(src, np.float32(np.inf)) - src).astype(np.float64)


def resize_fwd(x, ho, wo):
    """x [N, C, Hi, Wi] float64 (torch) -> (y [N, C, Ho, Wo], S = the same interpolation of |x|, T = the plain sum of the four taps'
    absolute values, which scales the effect of one ulp of src)."""
    hi, wi = x.shape[2:]
    wy, wx = torch.from_numpy(axis_matrix(hi, ho)), torch.from_numpy(axis_matrix(wi, wo))
    f = lambda t, a, b: torch.einsum("oi,ncij,pj->ncop", a, t, b)
    ny, nx = (wy != 0).double(), (wx != 0).double()
    return f(x, wy, wx), f(x.abs(), wy, wx), f(x.abs(), ny, nx)


def resize_bwd(dy, hi, wi):
    """dx = W_y^T dy W_x for dy [N, C, Ho, Wo] float64 -> (dx [N, C, Hi, Wi], S = the same map of |dy|)."""
    ho, wo = dy.shape[2:]
    wy, wx = torch.from_numpy(axis_matrix(hi, ho)), torch.from_numpy(axis_matrix(wi, wo))
    f = lambda t: torch.einsum("oi,ncop,pj->ncij", wy, t, wx)
    return f(dy), f(dy.abs())


def resize_terms(n_in, n_out):
    """The largest number of outputs one input feeds along an axis (the length of the backward's sum)."""
    return int((axis_matrix(n_in, n_out) != 0).sum(0).max())


# --------------------------------------------------------------------------------------------------------------------- cross-entropy
def ce2d(logits, target, ignore_index, grad_scale):
    """nn.CrossEntropyLoss(ignore_index, reduction='mean') on logits [N, C, H, W] float64, target [N, H, W] int64:
    (loss, grad_scale * dloss/dlogits, count).  No live pixel: loss NaN (0 / 0) and a zero gradient."""
    c = logits.shape[1]
    live = target != ignore_index
    count = int(live.sum())
    logp = torch.log_softmax(logits, 1)
    t = torch.where(live, target, torch.zeros_like(target)).clamp(0, c - 1)
    picked = logp.gather(1, t[:, None])[:, 0]
    loss = -(picked * live).sum() / count if count else torch.tensor(float("nan"), dtype=torch.float64)
    onehot = torch.zeros_like(logits).scatter_(1, t[:, None], 1.0)
    grad = (logp.exp() - onehot) * live[:, None] * (grad_scale / count if count else 0.0)
    return loss, grad, count


# ----------------------------------------------------------------------------------------------------------------------- max pooling
def pool_out(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def maxpool_fwd(x, k, s, p):
    """x [N, C, H, W] numpy float64 (may hold NaN, -inf) -> (y, idx uint8): windows scanned in (h, w) order over the in-bounds
    positions, the winner replaced where `v > best or isnan(v)`, best starting at -inf and idx at the first in-bounds position;
    idx = r * k + s of the winner inside its (padded) window."""
    n, c, h, w = x.shape
    ho, wo = pool_out(h, k, s, p), pool_out(w, k, s, p)
    xp = np.full((n, c, h + 2 * p + k, w + 2 * p + k), -np.inf)
    ok = np.zeros((h + 2 * p + k, w + 2 * p + k), bool)
    xp[:, :, p:p + h, p:p + w] = x
    ok[p:p + h, p:p + w] = True
    best = np.full((n, c, ho, wo), -np.inf)
    arg = np.zeros((n, c, ho, wo), np.int64)
    seen = np.zeros((ho, wo), bool)
    for r in range(k):
        for q in range(k):
            v = xp[:, :, r:r + s * ho:s, q:q + s * wo:s][:, :, :ho, :wo]
            valid = ok[r:r + s * ho:s, q:q + s * wo:s][:ho, :wo]
            first = valid & ~seen
            arg[:, :, first] = r * k + q
            seen |= valid
            with np.errstate(invalid="ignore"):
                upd = valid[None, None] & ((v > best) | np.isnan(v))
            best = np.where(upd, v, best)
            arg = np.where(upd, r * k + q, arg)
    assert seen.all()
    return best, arg.astype(np.uint8)


def maxpool_bwd(dy, idx, hi, wi, k, s, p):
    """Every output gradient added onto the input element its idx byte names: (dx, S = the same routing of |dy|, the largest
    number of gradients one input receives)."""
    n, c, ho, wo = dy.shape
    oy, ox = np.meshgrid(np.arange(ho), np.arange(wo), indexing="ij")
    iy = oy[None, None] * s - p + idx.astype(np.int64) // k
    ix = ox[None, None] * s - p + idx.astype(np.int64) % k
    assert iy.min() >= 0 and iy.max() < hi and ix.min() >= 0 and ix.max() < wi
    plane = np.arange(n * c, dtype=np.int64).reshape(n, c, 1, 1)
    flat = ((plane * hi + iy) * wi + ix).ravel()
    size = n * c * hi * wi
    dx = np.bincount(flat, weights=dy.ravel(), minlength=size).reshape(n, c, hi, wi)
    sa = np.bincount(flat, weights=np.abs(dy).ravel(), minlength=size).reshape(n, c, hi, wi)
    cnt = np.bincount(flat, minlength=size)
    return dx, sa, int(cnt.max())


# ------------------------------------------------------------------------------------------------------------------- average pooling
def avgpool_fwd(x):
    """x [N, C, HW] float64 -> (mean over HW, S = mean of |x|)."""
    return x.mean(2), x.abs().mean(2)


# ------------------------------------------------------------------------------------------------ pointwise classifier, small linear
def pointwise_fwd(x, w, b):
    """y[m, co] = b[co] + sum_ci x[m, ci] w[co, ci] -> (y, S = |b| + sum |x w|)."""
    y, s = x @ w.t(), x.abs() @ w.abs().t()
    return (y, s) if b is None else (y + b, s + b.abs())


def pointwise_bwd(dy, x, w):
    """(dx, S_dx, dw, S_dw, db, S_db) of pointwise_fwd; linear_small is the same without the bias."""
    return (dy @ w, dy.abs() @ w.abs(), dy.t() @ x, dy.abs().t() @ x.abs(), dy.sum(0), dy.abs().sum(0))


# --------------------------------------------------------------------------------------------------------------------------- dropout
def dropout(x, p, mask):
    """y = fl32(x * fl32(1 / (1 - p))) where mask != 0, else 0, as an fp32 tensor (the caller rounds it to the storage type)."""
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    return torch.where(mask != 0, x.float() * scale, torch.zeros((), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------ operands of the exact checks
def dyadic(a, b):
    return b % a == 0 and b // a in (1, 2, 4)


def ints(shape, amp, gen):
    return torch.randint(-amp, amp + 1, tuple(shape), generator=gen).double()


def ternary(shape, gen):
    return ints(shape, 1, gen)


def products_exact(a, b):
    """sum |a . b| of the matrix product a @ b stays below 2^24: fp32 accumulation in any order is exact."""
    return float((a.abs() @ b.abs()).max()) < 2.0 ** 24
