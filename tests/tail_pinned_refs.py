"""float64 references of the feature-mixing kernels (csrc/afan_mix.hip), the classifier head and the one-launch cross-entropy
(csrc/afan_head.hip) and the perturbation norms, written from the definitions; tests/test_tail_pinned_gpu.py holds every kernel
form to them elementwise, tests/test_tail_pinned_ref.py checks them on the CPU against torch in float64 and the fp32 C oracle.

Inputs are the stored values: a bf16 input is widened exactly.  Every reference returns, next to the value, S: the same operation on
absolute values, so that one fp32 rounding of a term moves the result by at most 2^-24 * S.

The host-side dispatch of the kernels is restated here (mix_plan, lerp_mix_plan, head_fwd_form, ce_form) with the source's
constants named, so that the GPU tables and the CPU coverage test share one statement of it.
"""
import numpy as np
import torch

from det_pinned_refs import U, bf16_edges, ints, midpoint_share, rne_bf16, ternary  # noqa: F401  (shared with the earlier pins)

F = np.float32
F32_MIN_NORMAL = 2.0 ** -126        # below it an fp32 expf may flush to zero: the absolute floor of the cross-entropy windows

# ---- constants of csrc/afan_mix.hip ------------------------------------------------------------------------------------------------
BLOCK = 256
WAVE = 64
LDS_DEFAULT = 64 * 1024             # dynamic LDS a launch gets without opting in
MAX_LDS_BYTES = 128 * 1024          # the staged tile's budget with the opt-in
LM_MAX = 4                          # points of one afan_lerp_mix launch
NHWC_GRID_CAP = 8192                # blocks of the channels-last kernels (4 waves = 4 pixels each)
MIXW_MAX_BLOCKS = 1024              # blocks of mix_w_dot_kernel (= the workspace's floats)
ELT_GRID_CAP = 256 * 8              # grid_for's default cap (mix_w_kernel, lerp_points_kernel)
KEEP_SMALL, KEEP_LARGE = 8, 20      # register-kept channels per lane of the channels-last kernels
# ---- constants of csrc/afan_head.hip -----------------------------------------------------------------------------------------------
MAXK = 16
DW_SLICES = 16
DW_COLS = 64
CE_BLOCK = 256
CEW_WAVES = 16
CE_WIDE_K = 64
CE_MAX_ELEMS = 1 << 16
# ---- csrc/afan_pgd.hip -------------------------------------------------------------------------------------------------------------
NORM_CHUNK = 4096
AFAN_ESHAPE = -3


# ================================================================================================================ dispatch, restated
def _stats_bytes(pix, sets):
    return sets * (BLOCK // pix) * pix * 3 * 4


def _tile(c):
    """The `pix`, `stage` pair both afan_mix_feature and afan_lerp_mix start from: the largest power-of-two pixel tile (<= 64, >= 8)
    whose staged clean column plus TWO sets of partial moments fits 64 KB, else 128 KB, else 64 pixels unstaged."""
    for budget in (LDS_DEFAULT, MAX_LDS_BYTES):
        pix = 64
        while pix >= 8 and c * pix * 4 + _stats_bytes(pix, 2) > budget:
            pix >>= 1
        if pix >= 8:
            return pix, True
    return 64, False


def _shrink(pix, hw):
    while pix > 8 and pix // 2 >= hw:          # tiny planes
        pix >>= 1
    return pix


def mix_plan(c, hw):
    """mix_impl: -> dict(pix, stage, lds, optin, tiles, tiny, groups)."""
    pix0, stage = _tile(c)
    pix = _shrink(pix0, hw)
    lds = _stats_bytes(pix, 2) + (c * pix * 4 if stage else 0)
    return dict(pix=pix, stage=stage, lds=lds, optin=stage and lds > LDS_DEFAULT, tiles=-(-hw // pix), tiny=pix != pix0, groups=BLOCK // pix)


def lerp_mix_bytes(c, pix, stage):
    return _stats_bytes(pix, 1 + LM_MAX) + (c * pix * 4 if stage else 0)


def lerp_mix_dead_branch(c):
    """The predicate afan_lerp_mix carried after its tile choice: `stage && bytes(pix, true) > 156 KB` (before the tiny-plane shrink)."""
    pix, stage = _tile(c)
    return stage and lerp_mix_bytes(c, pix, True) > 156 * 1024


def lerp_mix_plan(c, hw):
    """The NCHW branch of afan_lerp_mix: the tile of mix_plan, five sets of partial moments."""
    pix0, stage = _tile(c)
    pix = _shrink(pix0, hw)
    lds = lerp_mix_bytes(c, pix, stage)
    return dict(pix=pix, stage=stage, lds=lds, optin=stage and lds > LDS_DEFAULT, tiles=-(-hw // pix), tiny=pix != pix0, groups=BLOCK // pix)


def nhwc_keep(c):
    return KEEP_SMALL if c <= WAVE * KEEP_SMALL else KEEP_LARGE


def nhwc_grid(pixels):
    return max(1, min(NHWC_GRID_CAP, -(-pixels * WAVE // BLOCK)))


def mix_w_dot_grid(n):
    return max(1, min(MIXW_MAX_BLOCKS, -(-n // BLOCK))) if n > 0 else 1


def head_fwd_form(bf16, c, aligned16):
    if not bf16:
        return "scalar"
    return "vec" if c % 8 == 0 and c // 8 <= BLOCK and BLOCK % (c // 8) == 0 and aligned16 else "scalar"


def head_vec_groups(c):
    return BLOCK // (c // 8)


def ce_form(n, k):
    if n <= 0 or k <= 0 or n * k > CE_MAX_ELEMS:
        return None
    return "wide" if k >= CE_WIDE_K else "row"


# ======================================================================================================================= mix_feature
def moments(x):
    """mean and UNBIASED variance over the last axis; one channel gives 0 / 0 = NaN like torch.var."""
    n = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    return mu, ((x - mu) ** 2).sum(-1, keepdim=True) / (n - 1)


def _sens(x, mu, lanes):
    """Sensitivities of the kernels' one-pass moments.  Thread t of `lanes` (the 64 lanes of the channels-last kernels, the G channel
    groups of the pixel-tile kernels) takes channels t, t + lanes, ...; it sums d = x - shift (shift: its first value, x[t]) and
    d^2, forms mean = shift + sum d / cnt and M2 = sum d^2 - (sum d)^2 / cnt, and the `lanes` partials are merged by Chan's formula
    with fp32 means.
      mean: max |shift| + mean |x - shift|
      M2  : sum (x - shift)^2 + n_merges * |mu| * max |x - mu|: a merge squares d = mean_b - mean_a, and each mean carries
            |mu| * 2^-24; n_merges = min(lanes, n) - 1, the merges of two partials that both hold channels."""
    n = x.shape[-1]
    t = min(lanes, n)
    sh = x[..., torch.arange(n) % t]
    dev = (x - mu).abs().amax(-1, keepdim=True)
    s_mu = x[..., :t].abs().amax(-1, keepdim=True) + (x - sh).abs().mean(-1, keepdim=True)
    s_m2 = ((x - sh) ** 2).sum(-1, keepdim=True) + (t - 1) * mu.abs() * dev
    return s_mu, s_m2


def mix_feature(clean, adv, eps, lanes):
    """clean, adv: float64 [P, C], statistics over C per row.  out = (clean - mu_c) / sigma_c * sigma_a + mu_a with
    sigma = sqrt(var_unbiased + eps) -> (out, S).  S propagates the sensitivities of the four statistics through the expression:
    d out = d mu_c * sigma_a / sigma_c + d mu_a + |z sigma_a| * (d sigma_c / sigma_c + d sigma_a / sigma_a) + the roundings of the
    subtraction, division, product (|z sigma_a| each) and final sum (|out|), with d sigma / sigma = d M2 / (2 (n - 1) (var + eps))
    + the division, the sum with eps and the square root (3 in all for the two sigmas' own roundings, counted once each way)."""
    n = clean.shape[-1]
    mu_c, var_c = moments(clean)
    mu_a, var_a = moments(adv)
    sd_c, sd_a = (var_c + eps).sqrt(), (var_a + eps).sqrt()
    z = (clean - mu_c) / sd_c
    out = z * sd_a + mu_a
    smu_c, sm2_c = _sens(clean, mu_c, lanes)
    smu_a, sm2_a = _sens(adv, mu_a, lanes)
    t = (z * sd_a).abs()
    rel = sm2_c / (2 * (n - 1) * (var_c + eps)) + sm2_a / (2 * (n - 1) * (var_a + eps)) + 3 if n > 1 else torch.full_like(mu_c, float("nan"))
    s = 3 * t + out.abs() + smu_c * sd_a / sd_c + smu_a + t * rel
    return out, s


def rows_of(t, nhwc):
    """[N, C, H, W] (logical) -> [N * H * W, C] rows."""
    n, c = t.shape[:2]
    return t.reshape(n, c, -1).permute(0, 2, 1).reshape(-1, c)


def rows_back(r, shape):
    n, c = shape[:2]
    return r.reshape(n, -1, c).permute(0, 2, 1).reshape(shape)


# ====================================================================================================================== lerp / mix_w
def round_sum_f32(p, q):
    """RN_fp32(p + q) of float64 arrays WITHOUT double rounding: the float64 sum is taken to odd with the error term of an
    error-free two-sum (a sticky bit), after which the rounding to fp32 is that of the exact sum (53 >= 24 + 2 bits)."""
    s = p + q
    t = s - p
    err = (p - (s - t)) + (q - t)
    odd = (s.view(np.int64) & 1) == 1
    s = np.where((err != 0) & ~odd, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def lerp_f32(a, b, w):
    """ATen's two-form lerp of fp32 arrays as the kernels evaluate it: fmaf(w, b - a, a) for |w| < 0.5, else fmaf(w - 1, b - a, b);
    b - a and w - 1 round to fp32, the fused multiply-add rounds once (the 24 x 24 bit product is exact in float64)."""
    a, b, w = np.asarray(a, F), np.asarray(b, F), F(w)
    small = abs(w) < F(0.5)
    coeff = w if small else F(w - F(1))
    d = b - a
    assert d.dtype == F
    return round_sum_f32(np.float64(coeff) * d.astype(np.float64), (a if small else b).astype(np.float64))


def sample_weights(n_points):
    """The interior weights of get_sample_points(clean, adv, n_points) as fp32: j / (n_points - 1), j = 1 .. n_points - 2 (the
    n_points - 1 points after clean end with adv itself, which has no weight)."""
    return [F(j * (1.0 / (n_points - 1))) for j in range(1, n_points - 1)]


def mix_w_f32(clean, adv, w):
    """out = fl(c + fl(w * fl(a - c))): three fp32 roundings (numpy's fp32 arithmetic is IEEE, one rounding per operation)."""
    c, a, w = np.asarray(clean, F), np.asarray(adv, F), F(w)
    d = a - c
    m = w * d
    out = c + m
    assert out.dtype == F
    return out


def mix_w_grad(g, clean, adv):
    """dw = sum g * (a - c) -> (dw, S) in float64 of the stored values."""
    t = g.double() * (adv.double() - clean.double())
    return float(t.sum()), float(t.abs().sum())


# ============================================================================================================================== head
def head_forward(x, w, b):
    """x [B, HW, C], w [K, C], b [K] or None (float64) -> pooled, S_pooled, logits, S_logits."""
    pooled, sp = x.mean(1), x.abs().mean(1)
    logits, sl = pooled @ w.t(), sp @ w.abs().t()
    if b is not None:
        logits, sl = logits + b, sl + b.abs()
    return pooled, sp, logits, sl


def head_backward(dl, w, pooled, hw):
    """dx[b, c] (the same for every pixel) = (sum_k dl[b, k] w[k, c]) / HW; dW = dl^T pooled; db = sum_b dl -> each with its S."""
    return (dl @ w / hw, dl.abs() @ w.abs() / hw, dl.t() @ pooled, dl.abs().t() @ pooled.abs(), dl.sum(0), dl.abs().sum(0))


# ===================================================================================================================== cross-entropy
def cross_entropy(l, t):
    """l [N, K] float64, t [N] int64 -> dict(loss, s_loss, d, s_d).  A target outside [0, K) makes the loss and that row of d NaN.
    S of d: a probability p = exp(l - lse) moves by p * (|l| + |lse|) * 2^-24 per rounding of its argument, by p per rounding of its
    value; the one-hot term is exact.  S of the loss: mean_r (|lse_r| + |l[r, t_r]| + |lse_r - l[r, t_r]|)."""
    n, k = l.shape
    m = l.max(1, keepdim=True).values
    lse = m + (l - m).exp().sum(1, keepdim=True).log()
    p = (l - lse).exp()
    bad = (t < 0) | (t >= k)
    tc = torch.where(bad, torch.zeros_like(t), t)
    onehot = torch.zeros_like(l).scatter_(1, tc[:, None], 1.0)
    lt = l.gather(1, tc[:, None])
    rows = (lse - lt)[:, 0]
    loss = float("nan") if bool(bad.any()) else float(rows.mean())
    s_loss = float((lse.abs() + lt.abs() + (lse - lt).abs()).mean())
    d = (p - onehot) / n
    lfin = torch.where(torch.isfinite(l), l.abs(), torch.zeros_like(l))
    s_d = (p * (1 + lfin + lse.abs()) + onehot) / n
    d[bad] = float("nan")
    return dict(loss=loss, s_loss=s_loss, d=d, s_d=s_d, bad=bad)


def ce_loss_in_kernel_order(form, rows):
    """The mean of fp32 row losses in the fixed summation order of one kernel form, in fp32: "row" (ce_fwd_kernel: thread r % 256 adds
    its rows in order, the wave butterfly, the 4 waves in index order) or "wide" (ce_fwd_wide_kernel: wave r % 16 adds its rows in
    order, the 16 waves in index order); both end with * (1 / N).  With row losses that are exact in fp32 this names the kernel
    that ran: the two orders round differently."""
    rows = np.asarray(rows, F)
    n = len(rows)
    if form == "row":
        local = np.zeros(CE_BLOCK, F)
        for r in range(n):
            local[r % CE_BLOCK] = F(local[r % CE_BLOCK] + rows[r])
        parts = []
        for w in range(CE_BLOCK // WAVE):
            v = local[w * WAVE:(w + 1) * WAVE].copy()
            o = WAVE // 2
            while o:
                v = (v + v[np.arange(WAVE) ^ o]).astype(F)
                o >>= 1
            parts.append(v[0])
    else:
        parts = []
        for w in range(CEW_WAVES):
            acc = F(0)
            for r in range(w, n, CEW_WAVES):
                acc = F(acc + rows[r])
            parts.append(acc)
    s = F(0)
    for v in parts:
        s = F(s + v)
    return F(s * F(F(1) / F(n)))


# ============================================================================================================================= norms
def perturb_norms(xa, xc):
    """fp32 arrays [B, P] -> linf (bits: a max of fp32 differences), l2 and S = sum d^2 in float64 of the exact differences d."""
    d = (np.asarray(xa, F) - np.asarray(xc, F))
    assert d.dtype == F
    d64 = np.asarray(xa, np.float64) - np.asarray(xc, np.float64)
    ss = (d64 * d64).sum(1)
    return np.abs(d).max(1), np.sqrt(ss), ss
