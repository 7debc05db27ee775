"""What tests/test_conv_fused_pinned_gpu.py holds the FUSED forms of the tiled bf16 convolution to: the float64 references, the case
tables and the host-side predicates that pick an instantiation, restated (tests/test_conv_fused_pinned_ref.py checks the references
against torch autograd in float64 and the predicates at hand-computed points, on the CPU).

A fused reference is the composition  raw64 = conv64(x, w)  ->  raw = RNE_bf16(raw64)  ->  the BatchNorm definition on raw  (the
kernels normalise the rounded tile: the second pass of conv_igemm_body reads the bf16 tile it stored).  The convolution references and
the bf16 checks are test_conv_pinned_gpu.py's, the BatchNorm references and windows test_bn_pinned_gpu.py's: imported, not copied.
"""
import collections

import torch

from test_bn_pinned_gpu import (C_DB, C_DW, C_DX, C_STAT_INVSTD, C_STAT_MEAN, FWD_COMBOS, N_DX_ACC, N_INVSTD_ACC, N_MEAN_ACC, N_RUNNING,  # noqa: F401
                                N_UNBIAS, Report, U, _cv, check_affine_output, check_window, ref_affine, ref_bn_backward, ref_moments,
                                ref_running, ref_unbias, ulp32)
from test_conv_pinned_gpu import (C_BF16, C_WGRAD, EXPECTED_VARIANTS, FUSED_ALLOWLIST, _check_bf16, _check_exact, _density, _key,  # noqa: F401
                                  _ref_dgrad, _ref_fwd, _ref_wgrad, _ternary, _tuned)

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------- host-side predicates, restated
# (BM, BN, PF, WM, WN, PW, FBT, HL) as AFAN_TRACE_LAUNCH prints them
T64H, T64 = (64, 64, 7, 2, 2, 4, 4, 320), (64, 64, 5, 2, 2, 4, 4, 0)
H256, N128, N256 = (256, 128, 5, 4, 2, 4, 2, 328), (128, 64, 7, 2, 2, 4, 4, 320), (256, 64, 7, 4, 1, 4, 2, 400)
H64, H128 = (64, 128, 5, 2, 2, 4, 4, 320), (128, 128, 5, 2, 2, 4, 4, 320)
P64, P128 = (64, 128, 5, 2, 2, 4, 4, 0), (128, 128, 5, 2, 2, 4, 4, 0)
S64, S128 = (64, 128, 3, 2, 4, 0, 4, 0), (128, 128, 3, 2, 4, 0, 4, 0)
BK, CUS, LDS_PER_CU, THREADS_PER_CU = 64, 256, 160 * 1024, 2048
DEEP_MAX_BNF, DEEP_MAX = 384, 256          # dispatch_bnf's constexpr deep_max; dispatch()'s AFAN_CONV_DEEPMAX default


def kernel_name(direction, form, gs=0, bf=1):
    return "igemm_%s<%s,gs%d,bf%d>" % (direction, ",".join(map(str, form)), gs, bf)


def acc_slots(c):
    """afan_bn_nhwc.hip acc_slots: NS * C <= 1024, 1 <= NS <= 16, a power of two."""
    ns = 16
    while ns > 1 and ns * c > 1024:
        ns >>= 1
    return ns


def acc_ok(c):
    """afan_bn_acc_supported for bf16 (8 channels per vector, the vectors of a row divide a 256-thread block)."""
    return c > 0 and c % 8 == 0 and c // 8 <= 256 and 256 % (c // 8) == 0


def choose_bm(m, co, n_classes=1, equal_classes=False):
    n128 = co % 128 == 0
    cols = (co + (127 if n128 else 63)) // (128 if n128 else 64)
    if -(-m // 128) * cols * n_classes >= 256:
        return 128
    wg_64 = -(-m // 64) * cols * n_classes
    if n128 and (n_classes == 1 or equal_classes) and 256 < wg_64 <= 768:
        return 128
    return 64


def halo_ok(n, h, w, ci, co, k, dilation, bm, cap=320, n_classes=1, multi=False):
    """One dense 3x3 / stride-1 problem on whole 64-channel chunks whose every row tile's halo (first pixel's top-left tap to last
    pixel's bottom-right tap in the zero-padded raster) fits `cap` pixels."""
    if n_classes != 1 or multi or k != 3 or dilation != 1 or ci % 64 or co % 128:
        return False
    m = n * h * w

    def p0(i):
        t1, x = divmod(i, w)
        img, y = divmod(t1, h)
        return (img * (h + 2) + y) * (w + 2) + x

    for i in range(-(-m // bm)):
        m0, m1 = i * bm, min(i * bm + bm, m) - 1
        if p0(m1) + 2 * (w + 2) + 2 - p0(m0) + 1 > cap:
            return False
    return True


def lds_bytes(form):
    bm, bn, pf, _, _, _, _, hl = form
    stage = (pf - 1) * bn * BK * 2 + 2 * hl * BK * 2 + 1024 if hl else (2 if pf <= 3 else pf - 1) * (bm + bn) * (BK if pf >= 3 else BK + 8) * 2
    return max(stage, bm * (bn + 8) * 2)


def resident_cap(form):
    """An UPPER bound of launch_gs's residency cap (CUs x occupancy): what LDS and the thread count alone allow; registers may lower it."""
    threads = 64 * (form[3] * form[4] + form[5])
    return CUS * min(LDS_PER_CU // lds_bytes(form), THREADS_PER_CU // threads)


def launch_gs(form, m, co, n_classes=1, multi=False, bsc=False):
    """The in-launch form's own refusals (None) for a single-size problem: all workgroups that meet at the barrier resident, at least
    8 of them, at most 8 accumulator copies, the projection BatchNorm's backward on halo forms only."""
    bm, bn = form[0], form[1]
    meet = -(-co // bn) * -(-m // bm) * (1 if multi else n_classes)
    if acc_slots(co) > 8 or (form[7] == 0 and bsc) or meet > resident_cap(form) or meet < 8:
        return None
    return form


def dispatch_bnf(n, h, w, ci, co, k, dilation=1, n_classes=1, multi=False, bsc=False):
    """csrc/afan_conv_bnf.hip dispatch_bnf at default settings, in GEMM terms: ci = reduction channels, co = channels of the tensor the
    launch writes (an input gradient's are the layer's input channels), n * h * w = rows of one class.  None: AFAN_ESHAPE."""
    if co % 128 or not acc_ok(co):
        return None
    m = n * h * w
    bm = choose_bm(m, co, n_classes, multi)
    wgs = co // 128 * -(-m // bm) * n_classes
    hk = lambda b, cap=320: halo_ok(n, h, w, ci, co, k, dilation, b, cap, n_classes, multi)
    go = lambda f: launch_gs(f, m, co, n_classes, multi, bsc)
    if n_classes == 1 and ci >= 128:
        w64 = co // 64 * -(-m // 64)
        if 16 <= w64 <= 256:
            return go(T64H if hk(64) else T64)
    if bm == 128 and DEEP_MAX_BNF < wgs <= 2 * DEEP_MAX_BNF and hk(256, 328):
        return go(H256)
    if bm == 64 and ci >= 256:
        w_n64 = co // 64 * -(-m // 128) * n_classes
        if w_n64 <= DEEP_MAX_BNF and w_n64 >= wgs and hk(128):
            return go(N128)
    if bm == 128 and wgs <= DEEP_MAX_BNF and ci >= 256:
        w_n64 = co // 64 * -(-m // 256) * n_classes
        if w_n64 <= DEEP_MAX_BNF and w_n64 >= wgs and hk(256, 400):
            return go(N256)
    if wgs <= DEEP_MAX_BNF and hk(bm):
        return go(H64 if bm == 64 else H128)
    if wgs <= DEEP_MAX_BNF:
        r = go(P64 if bm == 64 else P128)
        if r is not None:
            return r
    return go(S64 if bm == 64 else S128)


def dispatch_grouped_dgrad(n, h, w, ci, co, k):
    """dispatch() for a stride-1 input gradient with grouped (groups = 2) BatchNorm-backward sums in accumulators, GEMM terms as above,
    for the three forms the workloads reach: (form, gs).  gs = the half-batch is not a whole number of this form's row tiles."""
    assert co % 128 == 0
    m = n * h * w
    bm = choose_bm(m, co)
    wgs = co // 128 * -(-m // bm)
    half = (n // 2) * h * w
    whole256 = half % 256 == 0
    hk = lambda b, cap=320: halo_ok(n, h, w, ci, co, k, 1, b, cap)
    if ci >= 128 and 16 <= co // 64 * -(-m // 64) <= 256:
        f = T64H if hk(64) else T64
    elif bm == 128 and DEEP_MAX < wgs <= 2 * DEEP_MAX and whole256 and hk(256, 328):
        f = H256
    elif bm == 64 and ci >= 256 and wgs <= co // 64 * -(-m // 128) <= DEEP_MAX and hk(128):
        f = N128
    elif bm == 128 and wgs <= DEEP_MAX and ci >= 256 and whole256 and wgs <= co // 64 * -(-m // 256) <= DEEP_MAX and hk(256, 400):
        f = N256
    elif wgs <= DEEP_MAX:
        f = (H64 if bm == 64 else H128) if hk(bm) else (P64 if bm == 64 else P128)
    else:
        f = S64 if bm == 64 else S128
    return f, int(half % f[0] != 0)


# ------------------------------------------------------------------------------------------------------------ float64 references
def rne_bf16(v):
    """float64 -> the nearest bf16 value (ties to even), as float64.  (float64 -> float32 first: exact for every value compared here
    that matters — integers and bf16 products — and otherwise a double rounding only on a 2^-29-relative band around a bf16 midpoint,
    where the checks accept both neighbours anyway.)"""
    return v.float().to(BF16).double()


def is_f32(v):
    return bool((v.float().double() == v).all())


def fma32(a, b, c):
    """fl32(a * b + c) for float64 tensors of fp32 values: the product is exact in float64; the sum rounds to 53 bits first, which
    changes the fp32 result only if it lands exactly on an fp32 midpoint.  Returns (value, tie): where tie, the neighbour on the other
    side of the float64 sum is as good."""
    s = a * b + c
    r = s.float().double()
    return r, (s - r).abs() * 2 == ulp32(r)


def ref_fwd_bn(raw, w, b, eps, res=None, sc=None, relu=True):
    """Train-mode BatchNorm of the bf16 tile `raw` (float64 tensor of bf16 values) (+ res | + BatchNorm of sc = (raw_sc, w_sc, b_sc,
    eps_sc)) (+ ReLU) from the definition: dict(mean, var, invstd, alpha, beta, y, [mean2, var2, invstd2, alpha2, beta2])."""
    mean, var = ref_moments(raw)
    invstd = 1.0 / torch.sqrt(var + eps)
    alpha = invstd * w
    beta = b - mean * alpha
    y = raw * _cv(alpha) + _cv(beta)
    out = dict(mean=mean, var=var, invstd=invstd, alpha=alpha, beta=beta)
    if sc is not None:
        r2, w2, b2, eps2 = sc
        m2, v2 = ref_moments(r2)
        is2 = 1.0 / torch.sqrt(v2 + eps2)
        a2 = is2 * w2
        be2 = b2 - m2 * a2
        y = y + r2 * _cv(a2) + _cv(be2)
        out.update(mean2=m2, var2=v2, invstd2=is2, alpha2=a2, beta2=be2)
    elif res is not None:
        y = y + res
    out["y"] = y.clamp_min(0.0) if relu else y
    return out


def ref_dgrad_bn(g, x, mean, invstd, alpha, mask, sc=None):
    """The BatchNorm backward behind an input gradient g (float64 of the bf16 gradient, the other branch's share already added): the
    masked gradient, dx, dweight, dbias and their scales (ref_bn_backward, from GIVEN statistics); sc = (sc_x, mean, invstd, alpha):
    the projection shortcut's BatchNorm (no ReLU) receives the masked gradient too: entries prefixed sc_."""
    r = ref_bn_backward(g, x, mean, invstd, alpha, mask)
    if sc is not None:
        sx, m2, is2, a2 = sc
        r2 = ref_bn_backward(r["g"], sx, m2, is2, a2, None)
        r.update({"sc_" + k: v for k, v in r2.items()})
    return r


# ----------------------------------------------------------------------------------------------------------------------- tables
# Forward / backward cases of the in-launch BatchNorm: LAYER terms (n, ci, co, h, k, dilation); `form` = the instantiation
# dispatch_bnf must send the launch to (forward: GEMM (ci, co); backward: GEMM (co, ci)).  The smallest shapes each instantiation
# admits with every workgroup count well inside the residency cap; M = n * h * h a power of two wherever the instantiation admits
# one away from the cap (N128, N256 and H256 take a power of two only at 256 workgroups = one per CU, the cap itself).
Case = collections.namedtuple("Case", "tag n ci co h k d form")
FWD_CASES = [
    Case("t64h_8x8", 8, 128, 128, 8, 3, 1, T64H),                # 16 workgroups, M = 512, 8 accumulator copies
    Case("t64h_partial_7x7", 11, 128, 128, 7, 3, 1, T64H),       # M = 539: partial last row tile, tiles straddle images
    Case("t64h_cols_8x8", 8, 128, 256, 8, 3, 1, T64H),           # four column tiles, 4 accumulator copies
    Case("t64_1x1", 8, 128, 128, 8, 1, 1, T64),
    Case("t64_dil2", 8, 128, 128, 8, 3, 2, T64),                 # atrous 3x3: per-tap form
    Case("t64_cols_1x1", 4, 128, 512, 8, 1, 1, T64),             # eight column tiles, 2 accumulator copies
    Case("p64_1x1", 8, 64, 128, 8, 1, 1, P64),                   # 8 workgroups: the barrier's minimum
    Case("p64_cols_1x1", 8, 64, 256, 8, 1, 1, P64),
    Case("p128_1x1", 65, 128, 128, 16, 1, 1, P128),              # 130 workgroups of 128 rows (choose_bm's tall rule)
    Case("p128_cols_1x1", 130, 128, 256, 8, 1, 1, P128),         # 130 workgroups, two column tiles
    Case("s128_1x1", 65, 128, 256, 16, 1, 1, S128),              # 260 workgroups: beyond the four-stage form's one per CU
    Case("n128_8x8", 65, 256, 256, 8, 3, 1, N128),               # 132 workgroups of 128 x 64, partial last row tile
    Case("n256_8x8", 130, 256, 256, 8, 3, 1, N256),              # 132 workgroups of 256 x 64 (four 8 x 8 images per tile)
    Case("h256_16x16", 97, 64, 256, 16, 3, 1, H256),             # 194 workgroups of 256 x 128 (one 16 x 16 image per tile)
]
BWD_CASES = [
    Case("t64h_8x8", 8, 128, 128, 8, 3, 1, T64H),
    Case("t64h_partial_7x7", 11, 128, 128, 7, 3, 1, T64H),
    Case("t64h_cols_8x8", 8, 256, 128, 8, 3, 1, T64H),
    Case("t64_1x1", 8, 128, 128, 8, 1, 1, T64),
    Case("t64_dil2", 8, 128, 128, 8, 3, 2, T64),
    Case("p64_1x1", 8, 128, 64, 8, 1, 1, P64),
    Case("p64_cols_1x1", 8, 256, 64, 8, 1, 1, P64),
    Case("p128_1x1", 65, 128, 128, 16, 1, 1, P128),
    Case("p128_cols_1x1", 130, 256, 128, 8, 1, 1, P128),
    Case("s128_1x1", 65, 256, 128, 16, 1, 1, S128),
    Case("n128_8x8", 65, 256, 256, 8, 3, 1, N128),
    Case("n256_8x8", 130, 256, 256, 8, 3, 1, N256),
    Case("h256_16x16", 97, 256, 64, 16, 3, 1, H256),
]
# the stride-2 pair forms (a block's first 3x3 / 2 and its 1x1 / 2 projection): (tag, n, ci, co, h) with h the INPUT's size
MULTI_FWD_CASES = [("multi_16x16", 8, 64, 128, 16, P64)]          # problem 0 meets at the barrier on 8 workgroups
PAIR_BWD_CASES = [("pair_16x16", 8, 128, 256, 16, P64)]           # four parity classes of 8 x 8: 32 workgroups
# frozen-BatchNorm epilogues (tag, n, ci, co, h, w, k, stride, dilation): a tiled 1x1, a 3x3, a 3x3 / 2 and one dilated shape
FROZEN_CASES = [("frozen_1x1", 3, 64, 256, 10, 12, 1, 1, 1), ("frozen_3x3", 2, 128, 128, 9, 11, 3, 1, 1),
                ("frozen_3x3s2", 2, 128, 128, 13, 11, 3, 2, 1), ("frozen_dil2", 2, 128, 128, 9, 11, 3, 1, 2)]
# grouped (groups = 2) input gradients with BatchNorm-backward sums, half-batch not a whole number of row tiles: layer terms
GROUPED_CASES = [Case("gs_h128_15x15", 74, 128, 128, 15, 3, 1, H128), Case("gs_p128_15x15", 74, 128, 128, 15, 1, 1, P128),
                 Case("gs_s128_15x15", 74, 256, 128, 15, 1, 1, S128)]
# weight gradients of several layers in one launch: lists of (n, ci, co, h, k, stride, dilation)
# (make_plan of afan_wgrad.hip: 128 rows where co % 128 == 0, 128 columns where ci % 128 == 0; the incremental pixel walk where the
# output width divides 64)
WGRAD_MULTI_CASES = {
    "wgrad_multi<64,64,inc0>": [(2, 64, 64, 9, 3, 1, 1), (3, 64, 64, 9, 1, 1, 1)],
    "wgrad_multi<64,64,inc1>": [(2, 64, 64, 8, 3, 1, 1), (3, 64, 64, 8, 1, 1, 1)],
    "wgrad_multi<128,64,inc0>": [(2, 64, 128, 9, 1, 1, 1), (2, 64, 256, 9, 3, 1, 1)],
    "wgrad_multi<128,128,inc0>": [(2, 128, 128, 9, 3, 1, 1), (2, 128, 128, 9, 3, 1, 2), (2, 128, 256, 9, 1, 1, 1), (1, 256, 128, 9, 1, 1, 1)],
    "wgrad_multi<128,128,inc1>": [(4, 128, 128, 8, 3, 1, 1), (4, 128, 256, 8, 1, 1, 1)],
}


def gemm_dims(case, backward):
    """(reduction channels, written channels) of the launch."""
    return (case.co, case.ci) if backward else (case.ci, case.co)
