"""Every BatchNorm kernel variant of csrc/afan_bn.hip and csrc/afan_bn_nhwc.hip pinned ELEMENTWISE to float64: the NCHW kernels (vector
and scalar access, shift fast path, slice caps), the channels-last slab kernels (butterfly fold and wide fold, generic mapping in both
forms, capped grids), the accumulator consumers (self-reducing, consumer only, grouped, dual), the partial-slab consumers, the eval
forms and afan_affine_relu_bwd.  The references are float64 torch code written here from the BatchNorm definition
(tests/test_bn_pinned_ref.py checks them against torch.nn.functional.batch_norm and autograd in double on the CPU).

Two checks per case:
  * exact: small integer operands (exact in bf16) whose channel means are integers and whose sums stay below 2^24 (asserted), so that
    fp32 / f64 accumulation is exact in any order and tiling.  dbias must equal the integer sum BIT FOR BIT, dweight the one rounding
    fl(invstd * integer), mean / invstd / running buffers float64 within the fp32 roundings of that path's finalisation (counted from
    the code, N_* below).  A missed, doubled or cross-wired row or channel shows here.
  * rounding-aware: Gaussian operands.  The published alpha / beta must be fl(invstd * w) and fma(-mean, alpha, b) of the published
    mean / invstd; given the published coefficients every output element must round from the float64 value of
    relu(x * alpha + beta + res) (bf16: the RNE bf16, the other neighbour only where a rounding midpoint lies within
    2^-23 * (|x * alpha + beta| + |res|), the two fp32 roundings of the formula; fp32: within that window).  No fraction is exempt.
    The ReLU mask of the backward is reproduced exactly (stored y > 0, or the sign of x * alpha + beta evaluated without rounding);
    dres must be the masked gradient bit for bit; dx, dweight, dbias are held to float64 from the published statistics and float64
    sums within C * 2^-24 * S, S = the sum of the absolute values of the terms, C = about three times the worst ratio over this
    table measured on an MI355X (*_MEASURED below), or the counted roundings where the sums themselves are exact f64.

The accumulator and partial-slab consumers are tested on their own: the test fills their input in float64 (every accumulator slot
gets a share, chosen so that the float64 total stays exact; the shift is a non-integer snapshot).

What the code specifies more loosely than a uniform rule would:
  * the biased variance is published only through invstd = 1 / sqrt(var + eps); invstd is what is compared;
  * the NCHW kernels publish mean | invstd only (rows 2, 3 of their stats block are not written); alpha / beta are derived on the
    host the way affine_coeffs() defines them, with one ulp of doubt on beta (the host emulation of the fp32 fma rounds twice): the
    window of an NCHW output grows by 2^-23 * |beta|, and a recomputed NCHW mask is exempt where |x * alpha + beta| lies within that
    doubt, for at most 1e-5 of the elements (test_bn_pinned_ref.py shows that the table's inputs have none there);
  * the NCHW backward multiplies by invstd inside the sum (sum g * ((x - mean) * invstd)): its dweight is not one rounding of an
    integer and is held to the rounding-aware bound in the exact check as well; the NCHW moments are Chan merges in fp32 and held to the measured bounds in both checks;
  * afan_bn_running_update_batched recovers the variance as 1 / invstd^2 - eps: relative to var + eps that is invstd's own ulp.

Coverage: EXPECTED_VARIANTS lists every path the table must reach; the host-side predicates that pick a path are restated here
(checked against afan_bn_acc_supported / ops.bn_acc_ok / the constants in the sources).
"""
import collections
import ctypes
import functools
import os
import re
import types
import zlib

import pytest
import torch

F32, BF16 = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF16: "bf16"}
DTC = {F32: 0, BF16: 1}
VEC = {F32: 4, BF16: 8}
NCHW, NHWC = 0, 1
U = 2.0 ** -24                      # half an ulp of 1.0f: the unit of one fp32 rounding
BLOCK, MAX_SLICES, MAX_G, APPLY_CAP = 256, 64, 512, 512      # afan_bn.hip / afan_bn_nhwc.hip (test_constants_match_sources)
SENTINEL = -777.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- fp32 roundings of each path's finalisation (exact check: the sums themselves carry none) ------------------------------------------
# slab / partials (finalize_kernel MODE 0): mean = (float)(shift + a / M) in double: 1.  invstd: m2 -> float 1, inv_m = 1.0f / M 1,
# m2 * inv_m 1, + eps 1, sqrtf 1, 1.0f / . 1 = 6 (each at most one unit relative; the square root halves the first four).
N_MEAN_SLAB, N_INVSTD_SLAB = 1, 6
# accumulator (apply_acc_kernel derive): mean in double, rounded once: 1 ulp.  invstd: (float)(m2 * inv_m) 1, + eps 1, sqrtf 1, divide 1.
N_MEAN_ACC, N_INVSTD_ACC = 1, 4
# (NCHW: the moments are Chan merges in fp32, up to 15 on the longest path; a worst-case count is far looser than what the kernels do, so
# the NCHW statistics are held to the measured STAT_*_MEASURED["nchw"] bounds in the exact check as well.)
# r <- (1 - momentum) * r + momentum * stat: 1 - momentum 1, two products 2, add 1 = 4 per update, relative to |r| + |stat|; the unbiased
# variance adds the division / product by M / (M - 1): 2
N_RUNNING = 4
N_UNBIAS = 2
# dx on the consumer-only accumulator paths (bwd_apply_acc_kernel, sums exact f64): x - mean 1; B: (float)b 1, * is 1, * inv_m -> float 1,
# alpha * is 1, product 1 = 5; D: (float)a 1, * inv_m -> float 1, alpha * . 1 = 3; two fma 2.  All relative to terms of S: 1 + 5 + 2 = 8.
N_DX_ACC = 8
# dweight = (float)b * is (+ the other group's): 2 (4 grouped); dbias = (float)a: 1 (3 grouped)
N_DW_ACC, N_DB_ACC = 4, 3

# ---- measured constants: worst |kernel - float64| / (2^-24 * S) over THIS table (FWD_CASES / BWD_CASES, exact and Gaussian runs, every
# combination) on an MI355X, float64 = the references of this module; each bound is three times its worst.  Every test prints its
# figures ("BNPIN <key> <ratio> <case>", run with -s) before it asserts.
# keys: accumulation type ("f32sum": bf16 tensors and every NCHW kernel sum in fp32; "f64sum": fp32 channels-last tensors sum in f64)
# dx: S = |g * alpha| + |x - mean| * |B| + |D| as the sum of the terms' absolute values.  The worst ratios are large because B and D are
# proportional to sum g (x - mean) and sum g, which cancel by chance in some channel of a wide layer, while the noise of the sums does not
# cancel with them: the slab kernels store every block partial as fp32 (also where the block summed in f64), so the sums carry
# 2^-24 * |partial| each, relative to sum |g| and not to |sum g|.  It shows at masked elements (g = 0), where S is |x - mean| |B| + |D| alone.
# Worst: f32sum bwd-bf16-2x2048x33x33-nhwc (relu, recomputed mask), f64sum bwd-f32-2x1024x33x29-nhwc (relu, recomputed mask).
DX_MEASURED = {"f32sum": 33.88, "f64sum": 504.88}
DW_MEASURED = {"f32sum": 3.02, "f64sum": 1.21}           # S = sum |g * xhat|; worst bwd_acc0-bf16-1x512x1x7-nhwc, bwd-f32-2x1024x33x29-nhwc
DB_MEASURED = {"f32sum": 0.79, "f64sum": 1.27}           # S = sum |g|; worst bwd-f32-2x5x4x8-nchw-off1, bwd-f32-5x200x6x5-nhwc
C_DX = {k: 3.0 * v for k, v in DX_MEASURED.items()}
C_DW = {k: 3.0 * v for k, v in DW_MEASURED.items()}
C_DB = {k: 3.0 * v for k, v in DB_MEASURED.items()}
# statistics of a stored Gaussian tensor against float64 of that tensor, per scheme: mean in units of 2^-24 * (|mean| + std), invstd in
# units of 2^-24 relative.  Worst cases: mean: the |mean| >> std cases (mean 40, std 0.5) except slab (train-bf16-2x16x33x29, train-f32-1x64x1x7);
# invstd: train-f32-4x6x8x8-nchw-cancel, train-bf16-3x304x5x7 (15 rows per fp32 thread sum), train-f32-5x200x6x5, acc0-bf16-65x16x64x64,
# acc0-f32-2x1024x33x29
STAT_MEAN_MEASURED = {"nchw": 1.69, "slab_f32sum": 0.80, "slab_f64sum": 1.12, "acc_f32sum": 0.79, "acc_f64sum": 0.79}
# ... and of accumulators a CONVOLUTION epilogue filled (bf16 tile minus a non-integer shift summed in fp32 within a row tile, f64 across
# tiles), consumed by afan_bn_train_forward_acc[_dual] or inside the launch: tests/test_conv_fused_pinned_gpu.py's table, where the
# two-launch and the in-launch form alike pass 3 * 0.79 (worst, both forms: fwd_bn t64h_cols_8x8, 64-row tiles of 8 accumulator slots)
STAT_MEAN_MEASURED["conv_acc_f64sum"] = 2.74
STAT_INVSTD_MEASURED = {"nchw": 4.11, "slab_f32sum": 16.45, "slab_f64sum": 4.62, "acc_f32sum": 7.74, "acc_f64sum": 1.93}
C_STAT_MEAN = {k: 3.0 * v for k, v in STAT_MEAN_MEASURED.items()}
C_STAT_INVSTD = {k: 3.0 * v for k, v in STAT_INVSTD_MEASURED.items()}
# afan_bn_running_update[_batched]: |running_var - float64 of the stored tensor| / (2^-24 * (|r| + (var + eps) * M / (M - 1))) over the three
# BatchNorms of test_running_update_replay_pinned (batched and single alike): about 1e-7 relative, inside the source's "~1e-6"
REPLAY_MEASURED = 1.73
C_REPLAY = 3.0 * REPLAY_MEASURED

FWD_COMBOS = [(0, 0), (0, 1), (1, 1)]                                            # (res, relu)
BWD_COMBOS = [(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]  # (relu, have_y, dres): all the dispatch has
AFFINE_BWD_COMBOS = [(0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 0, 1), (1, 1, 1)]      # (relu, dx, dres)

Case = collections.namedtuple("Case", "entry dt shape layout off cancel")


def _c(entry, dt, shape, layout=NHWC, off=0, cancel=False):
    return Case(entry, dt, tuple(shape), layout, off, cancel)


# ------------------------------------------------------------------------------------------------- host-side predicates, restated
def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def nhwc_vec_ok(dt, c, aligned=True):
    """make_plan<T> of afan_bn_nhwc.hip (and acc_supported, which is the same without the pointers)."""
    v = VEC[dt]
    return c % v == 0 and c // v <= BLOCK and BLOCK % (c // v) == 0 and aligned


def nhwc_grids(dt, m, c, vec):
    """(G of the reduction, blocks of the apply pass, capped?) as make_plan / apply_grid compute them."""
    nvec = m * (c // VEC[dt]) if vec else 0
    work = -(-nvec // BLOCK) if vec else (m + 15) // 16
    g = max(1, (work + 3) // 4)
    items = -(-nvec // 4) if vec else m * c
    blocks = max(1, -(-items // BLOCK))
    return min(g, MAX_G), min(blocks, APPLY_CAP), g > MAX_G and blocks > APPLY_CAP


def nchw_plan(dt, n, c, hw, aligned=True):
    """make_plan<T> of afan_bn.hip: (elements per access, hwv a power of two, S, what limits S)."""
    vec = VEC[dt] if (hw % VEC[dt] == 0 and aligned) else 1
    hwv = hw // vec
    chunks = -(-(n * hwv) // BLOCK)
    by_c = -(-2048 // c)
    s = max(1, min(by_c, chunks, MAX_SLICES))
    lim = "S_max" if (s == MAX_SLICES and chunks > MAX_SLICES) else ("S_chunks" if (s == chunks and chunks < by_c and chunks > 1) else "S_other")
    return vec, _pow2(hwv), s, lim


def acc_slots(lib, c):
    """NS recovered from afan_bn_acc_doubles (acc[slot][q][C] doubles, then C floats of shift) and the stride of one group's block."""
    d = int(lib.afan_bn_acc_doubles(c))
    ns, rem = divmod(d - (c + 1) // 2, 2 * c)
    assert rem == 0 and _pow2(ns) and ns <= 16, (c, d, ns)
    return ns, (d + 1) & ~1


def _aligned(case):
    return (case.off * (4 if case.dt == F32 else 2)) % 16 == 0


def paths_of(case):
    """The path names a case reaches, from the predicates alone."""
    n, c, h, w = case.shape
    m, dt, e = n * h * w, case.dt, case.entry
    p = set()
    if e in ("train", "bwd", "apply"):
        pre = {"train": "", "bwd": "bwd_", "apply": "apply_"}[e]
        if case.layout == NCHW:
            if e == "apply":
                return {"apply_nchw"}
            vec, p2, s, lim = nchw_plan(dt, n, c, h * w, _aligned(case))
            if e == "bwd":
                return {"bwd_nchw_vec" if vec > 1 else "bwd_nchw_scalar"}
            p.add("nchw_vec" if vec > 1 else ("nchw_scalar_view" if (h * w) % VEC[dt] == 0 else "nchw_scalar_hw"))
            p.add("nchw_pow2" if p2 else "nchw_div")
            if lim != "S_other":
                p.add("nchw_" + lim)
            return p
        vec = nhwc_vec_ok(dt, c, _aligned(case))
        if e == "apply":
            return {"apply_nhwc"}
        if e == "bwd":
            return {"bwd_nhwc_vec" if vec else "bwd_nhwc_generic"}
        if vec:
            p.add("nhwc_slab_fold" if c // VEC[dt] < 64 else "nhwc_slab_wide")
            if nhwc_grids(dt, m, c, True)[2]:
                p.add("nhwc_cap")
        elif nhwc_vec_ok(dt, c):
            p.add("nhwc_generic_view")
        else:
            p.add("nhwc_generic_rows" if c <= BLOCK else "nhwc_generic_wide")
        return p
    assert case.layout == NHWC or e == "affine_bwd"
    if e in ("acc0", "acc1", "acc_g2", "dual", "bwd_acc0", "bwd_acc1", "bwd_acc_g2"):
        assert nhwc_vec_ok(dt, c, _aligned(case)), case
    name = {"acc0": "acc_self", "acc1": "acc_ready", "acc_g2": "acc_groups2", "partials": "partials", "dual": "dual", "affine": "affine",
            "bwd_partials": "bwd_partials", "bwd_acc0": "bwd_acc_self", "bwd_acc1": "bwd_acc_ready", "bwd_acc_g2": "bwd_acc_groups2",
            "affine_bwd": "affine_relu_bwd"}[e]
    p.add(name)
    if e == "acc1":       # fold_ahead_ok(C, NS): C > 256 and NS <= 2 (NS * C <= 1024)
        p.add("acc_fold_ahead" if c > BLOCK else "acc_fold_plain")
    if e == "acc0" and nhwc_grids(dt, m, c, True)[2]:
        p.add("nhwc_cap")
    return p


# ---------------------------------------------------------------------------------------------------------------------- the table
S1, S7, SB = (1, 1, 1), (1, 1, 7), (2, 33, 29)          # (n, h, w): M = 1, 7, 2 * 33 * 29 (no multiple of 256 / CV for any CV > 1... 1914)


def _sh(c, s):
    return (s[0], c, s[1], s[2])


FWD_CASES = [
    # NCHW: vector / scalar access, hwv a power of two or not, S at MAX_SLICES / limited by the chunks
    _c("train", BF16, (2, 5, 8, 8), NCHW), _c("train", F32, (2, 5, 4, 8), NCHW),
    _c("train", BF16, (3, 4, 6, 8), NCHW), _c("train", F32, (3, 4, 3, 4), NCHW),
    _c("train", BF16, (3, 5, 7, 9), NCHW), _c("train", F32, (3, 5, 7, 9), NCHW),
    _c("train", BF16, (2, 5, 8, 8), NCHW, off=1), _c("train", BF16, (2, 5, 8, 8), NCHW, off=4), _c("train", F32, (2, 5, 4, 8), NCHW, off=1),
    _c("train", BF16, (4, 3, 128, 264), NCHW), _c("train", F32, (2, 3, 128, 264), NCHW),
    _c("train", BF16, (2, 5, 32, 40), NCHW), _c("train", F32, (2, 5, 16, 40), NCHW),
    _c("train", BF16, (1, 6, 1, 1), NCHW), _c("train", F32, (4, 6, 8, 8), NCHW, cancel=True),
    # channels-last, vector mapping, slab scheme: CV < 64 (butterfly fold) and CV >= 64
    _c("train", BF16, _sh(8, S1)), _c("train", BF16, _sh(16, S7)), _c("train", BF16, _sh(16, SB)), _c("train", BF16, _sh(64, SB)),
    _c("train", BF16, _sh(512, S7)), _c("train", BF16, _sh(512, SB)), _c("train", BF16, _sh(64, (3, 5, 7)), cancel=True),
    _c("train", F32, _sh(4, S1)), _c("train", F32, _sh(4, SB)), _c("train", F32, _sh(64, S7)), _c("train", F32, _sh(64, SB)),
    _c("train", F32, _sh(1024, SB)), _c("train", F32, _sh(64, (3, 5, 7)), cancel=True),
    # both caps (MAX_G of the reduction grid, 512 blocks of apply_grid) with a tail
    _c("train", BF16, (2, 2048, 33, 33)), _c("train", BF16, (65, 16, 64, 64)),
    # generic mapping: several rows per block pass (C <= 256), thread per channel (C > 256), vector shape on a misaligned view
    _c("train", BF16, (2, 48, 33, 29)), _c("train", F32, (2, 48, 33, 29)), _c("train", BF16, _sh(3, S7)), _c("train", F32, _sh(3, S1)),
    _c("train", BF16, (5, 200, 6, 5)), _c("train", F32, (5, 200, 6, 5)), _c("train", BF16, (3, 304, 5, 7)), _c("train", F32, (3, 304, 5, 7)),
    _c("train", BF16, (2, 48, 9, 9), cancel=True),
    _c("train", BF16, (2, 64, 5, 7), off=1), _c("train", BF16, (2, 64, 5, 7), off=4), _c("train", F32, (2, 64, 5, 7), off=1),
    # accumulator scheme: self-reducing, consumer only (plain and look-ahead fold of the slots), two groups, dual
    _c("acc0", BF16, _sh(8, S1)), _c("acc0", BF16, _sh(64, SB)), _c("acc0", BF16, _sh(512, S7)), _c("acc0", BF16, (2, 2048, 33, 33)),
    _c("acc0", BF16, (65, 16, 64, 64)), _c("acc0", BF16, _sh(64, (3, 5, 7)), cancel=True),
    _c("acc0", F32, _sh(4, S7)), _c("acc0", F32, _sh(64, SB)), _c("acc0", F32, _sh(1024, SB)), _c("acc0", F32, _sh(64, (3, 5, 7)), cancel=True),
    _c("acc1", BF16, _sh(8, S1)), _c("acc1", BF16, _sh(64, SB)), _c("acc1", BF16, _sh(512, SB)), _c("acc1", BF16, _sh(2048, S7)),
    _c("acc1", F32, _sh(4, S7)), _c("acc1", F32, _sh(64, SB)), _c("acc1", F32, _sh(1024, SB)), _c("acc1", BF16, _sh(64, (3, 5, 7)), cancel=True),
    _c("acc_g2", BF16, (4, 64, 5, 7)), _c("acc_g2", BF16, (4, 512, 5, 7)), _c("acc_g2", F32, (4, 64, 5, 7)), _c("acc_g2", F32, (4, 512, 5, 7)),
    _c("dual", BF16, (2, 64, 33, 29)), _c("dual", BF16, (3, 128, 5, 7)), _c("dual", F32, (2, 64, 33, 29)), _c("dual", F32, (3, 128, 5, 7)),
    # test-filled partial slabs (G below and above one wave of the finalize)
    _c("partials", BF16, (2, 64, 33, 29)), _c("partials", BF16, (2, 48, 9, 9)), _c("partials", F32, (2, 64, 33, 29)), _c("partials", F32, (5, 200, 6, 5)),
    # eval forms
    _c("apply", BF16, (3, 5, 7, 9), NCHW), _c("apply", F32, (2, 5, 4, 8), NCHW), _c("apply", BF16, (2, 64, 33, 29)), _c("apply", F32, (2, 48, 9, 9)),
    _c("affine", BF16, (2, 64, 33, 29)), _c("affine", BF16, (2, 48, 9, 9)), _c("affine", F32, (2, 64, 33, 29)), _c("affine", F32, (3, 304, 5, 7)),
]

BWD_CASES = [
    _c("bwd", BF16, (2, 5, 8, 8), NCHW), _c("bwd", F32, (3, 4, 3, 4), NCHW), _c("bwd", BF16, (3, 5, 7, 9), NCHW), _c("bwd", F32, (2, 5, 4, 8), NCHW, off=1),
    _c("bwd", BF16, (4, 3, 128, 264), NCHW), _c("bwd", F32, (2, 5, 16, 40), NCHW),
    _c("bwd", BF16, _sh(8, S1)), _c("bwd", BF16, _sh(16, SB)), _c("bwd", BF16, _sh(512, SB)), _c("bwd", BF16, (2, 2048, 33, 33)),
    _c("bwd", BF16, (65, 16, 64, 64)), _c("bwd", F32, _sh(4, S7)), _c("bwd", F32, _sh(64, SB)), _c("bwd", F32, _sh(1024, SB)),
    _c("bwd", BF16, (2, 48, 33, 29)), _c("bwd", F32, (5, 200, 6, 5)), _c("bwd", BF16, (3, 304, 5, 7)), _c("bwd", F32, _sh(3, S7)),
    _c("bwd", BF16, (2, 64, 5, 7), off=1), _c("bwd", F32, (2, 64, 5, 7), off=1),
    _c("bwd_partials", BF16, (2, 64, 33, 29)), _c("bwd_partials", F32, (5, 200, 6, 5)),
    _c("bwd_acc0", BF16, _sh(64, SB)), _c("bwd_acc0", BF16, _sh(512, S7)), _c("bwd_acc0", F32, _sh(64, SB)), _c("bwd_acc0", BF16, (65, 16, 64, 64)),
    _c("bwd_acc1", BF16, _sh(64, SB)), _c("bwd_acc1", BF16, _sh(512, SB)), _c("bwd_acc1", F32, _sh(64, SB)), _c("bwd_acc1", F32, _sh(1024, S7)),
    _c("bwd_acc_g2", BF16, (4, 64, 5, 7)), _c("bwd_acc_g2", BF16, (4, 512, 5, 7)), _c("bwd_acc_g2", F32, (4, 64, 5, 7)), _c("bwd_acc_g2", F32, (4, 512, 5, 7)),
]
AFFINE_BWD_CASES = [_c("affine_bwd", BF16, (2, 64, 33, 29)), _c("affine_bwd", BF16, (2, 48, 9, 9)), _c("affine_bwd", F32, (3, 5, 7, 9), NCHW),
                    _c("affine_bwd", F32, (2, 64, 5, 7), off=1)]


def case_id(c):
    return f"{c.entry}-{DTN[c.dt]}-{'x'.join(map(str, c.shape))}-{'nhwc' if c.layout == NHWC else 'nchw'}" + (f"-off{c.off}" if c.off else "") + \
        ("-cancel" if c.cancel else "")


FWD_PATHS = ["nchw_vec", "nchw_scalar_hw", "nchw_scalar_view", "nchw_pow2", "nchw_div", "nchw_S_max", "nchw_S_chunks",
             "nhwc_slab_fold", "nhwc_slab_wide", "nhwc_generic_rows", "nhwc_generic_wide", "nhwc_generic_view", "nhwc_cap",
             "acc_self", "acc_ready", "acc_fold_plain", "acc_fold_ahead", "acc_groups2", "partials", "apply_nchw", "apply_nhwc", "affine"]
BWD_PATHS = ["bwd_nchw_vec", "bwd_nchw_scalar", "bwd_nhwc_vec", "bwd_nhwc_generic", "bwd_partials", "bwd_acc_self", "bwd_acc_ready",
             "bwd_acc_groups2"]


def _combo_s(combo):
    return "".join(map(str, combo))


EXPECTED_VARIANTS = sorted(
    [f"{p}|{d}|res{r}relu{u}" for p in FWD_PATHS for d in ("f32", "bf16") for r, u in FWD_COMBOS if not (p == "nhwc_cap" and d == "f32")] +
    [f"dual|{d}|res1relu1" for d in ("f32", "bf16")] +
    [f"{p}|{d}|relu{a}y{b}dres{e}" for p in BWD_PATHS for d in ("f32", "bf16") for a, b, e in BWD_COMBOS] +
    [f"affine_relu_bwd|{d}|relu{a}dx{b}dres{e}" for d in ("f32", "bf16") for a, b, e in AFFINE_BWD_COMBOS])


def variants_of(case):
    if case.entry == "dual":
        combos = ["res1relu1"]
    elif case.entry == "affine_bwd":
        combos = [f"relu{a}dx{b}dres{e}" for a, b, e in AFFINE_BWD_COMBOS]
    elif case.entry.startswith("bwd"):
        combos = [f"relu{a}y{b}dres{e}" for a, b, e in BWD_COMBOS]
    else:
        combos = [f"res{r}relu{u}" for r, u in FWD_COMBOS]
    return {f"{p}|{DTN[case.dt]}|{s}" for p in paths_of(case) for s in combos}


# ------------------------------------------------------------------------------------------------------------ float64 references
def _cv(v):
    return v.view(1, -1, 1, 1)


def ref_moments(x):
    """Per-channel mean and BIASED variance of a [N, C, H, W] tensor, float64, two passes."""
    xd = x.double()
    mean = xd.mean((0, 2, 3))
    var = ((xd - _cv(mean)) ** 2).mean((0, 2, 3))
    return mean, var


def ref_running(r0, stat, momentum, updates=1):
    r = r0.double().clone()
    for _ in range(updates):
        r = (1.0 - momentum) * r + momentum * stat
    return r


def ref_unbias(m):
    return m / (m - 1.0) if m > 1 else 1.0          # one row: the kernels leave the biased estimate (0) alone


def ref_affine(x, alpha, beta, res, relu):
    """relu(x * alpha + beta + res) in float64 and the window scale |x * alpha + beta| + |res|."""
    v = x.double() * _cv(alpha.double()) + _cv(beta.double())
    s = v.abs()
    if res is not None:
        v = v + res.double()
        s = s + res.double().abs()
    return (v.clamp_min(0.0) if relu else v), v, s


def ref_bn_forward(x, w, b, eps, res, relu):
    mean, var = ref_moments(x)
    invstd = 1.0 / torch.sqrt(var + eps)
    alpha = invstd * w.double()
    beta = b.double() - mean * alpha
    return ref_affine(x, alpha, beta, res, relu)[0], mean, var, invstd


def ref_bn_backward(dy, x, mean, invstd, alpha, mask):
    """dx, dweight, dbias of y = [relu](xhat * w + b [+ res]) from given statistics (float64 tensors), alpha = invstd * w; mask = the ReLU
    mask or None.  Also the masked gradient, the sums and the scales S of the three results."""
    g = dy.double()
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    m = float(x.shape[0] * x.shape[2] * x.shape[3])
    xm = x.double() - _cv(mean)
    sg, sgx = g.sum((0, 2, 3)), (g * xm).sum((0, 2, 3))
    bcoef = -alpha * invstd * invstd * sgx / m
    dcoef = -alpha * sg / m
    dx = g * _cv(alpha) + xm * _cv(bcoef) + _cv(dcoef)
    s_dx = (g * _cv(alpha)).abs() + xm.abs() * _cv(bcoef.abs()) + _cv(dcoef.abs())
    return dict(dx=dx, dw=invstd * sgx, db=sg, g=g, sg=sg, sgx=sgx, s_dx=s_dx, s_dw=(g * xm).abs().sum((0, 2, 3)) * invstd,
                s_db=g.abs().sum((0, 2, 3)))


# ------------------------------------------------------------------------------------------------------------------- input makers
def _seed(case, salt):
    return (zlib.crc32(repr(tuple(case)).encode()) * 31 + salt) % (1 << 31)


@functools.lru_cache(maxsize=2)
def exact_inputs(case, salt=0):
    """Integer x (|x| <= 4, exact in bf16) with an exact integer mean per channel (per half-batch for the grouped entries) that differs
    between neighbouring channels, integer gradient and residual.  Returns float64 CPU tensors [N, C, H, W] (read-only: cached) and the
    channel means."""
    n, c, h, w = case.shape
    m = n * h * w
    groups = 2 if case.entry.endswith("_g2") else 1
    mg = m // groups
    g = torch.Generator().manual_seed(_seed(case, 11 + salt))
    amp = 2 if m <= 100000 else 1
    halves = []
    for _ in range(groups):
        r = torch.randint(-amp, amp + 1, (c, mg // 2), generator=g, dtype=torch.int64)
        d = torch.cat([r, -r] + ([torch.zeros(c, 1, dtype=torch.int64)] if mg % 2 else []), 1)
        halves.append(d.gather(1, torch.rand(c, mg, generator=g).argsort(1)))
    d = torch.cat(halves, 1)
    mean = (torch.arange(c) % (2 * amp + 1)) - amp
    x = (d + mean[:, None]).view(c, n, h, w).permute(1, 0, 2, 3).double()
    dy = torch.randint(-2, 3, case.shape, generator=g).double()
    res = torch.randint(-3, 4, case.shape, generator=g).double()
    return x, dy, res, mean.double()


def assert_exact_preconditions(x, dy, mean, shift=None):
    """Every sum the kernels take is an integer (or a dyadic fraction with few bits) below 2^24 in magnitude even as a sum of absolute
    values, so no order of fp32 additions rounds."""
    sh = x[0:1, :, 0:1, 0:1] if shift is None else _cv(shift)
    d = x - sh
    xm = x - _cv(mean)
    assert bool((ref_moments(x)[0] == mean).all()), "channel means are not the intended integers"
    for name, v in (("sum |x - shift|", d.abs()), ("sum (x - shift)^2", d * d), ("sum |g|", dy.abs()), ("sum |g (x - mean)|", (dy * xm).abs())):
        assert float(v.sum((0, 2, 3)).max()) < 2.0 ** 24, f"{name} >= 2^24: fp32 partial sums may round"


@functools.lru_cache(maxsize=2)
def gauss_inputs(case, salt=0):
    """Gaussian x per channel (mean in [-1.5, 1.5], std in [0.5, 1.5]; cancel: mean 40, std 0.5), gradient and residual, rounded to the
    case's storage type; float64 CPU tensors."""
    n, c, h, w = case.shape
    g = torch.Generator().manual_seed(_seed(case, 23 + salt))
    if case.cancel:
        mu, sd = torch.full((c,), 40.0), torch.full((c,), 0.5)
    else:
        mu, sd = torch.rand(c, generator=g) * 3.0 - 1.5, torch.rand(c, generator=g) + 0.5
    q = lambda t: t.to(case.dt).double()
    x = q(torch.randn(case.shape, generator=g) * _cv(sd) + _cv(mu))
    return x, q(torch.randn(case.shape, generator=g)), q(torch.randn(case.shape, generator=g))


def params(case, salt=0):
    """weight, bias, running_mean, running_var (fp32 values as float64 CPU tensors), eps, momentum (as the float the kernel receives)."""
    c = case.shape[1]
    g = torch.Generator().manual_seed(_seed(case, 37 + salt))
    f = lambda t: t.float().double()
    w, b = f(torch.rand(c, generator=g) + 0.5), f(torch.randn(c, generator=g))
    rm, rv = f(torch.randn(c, generator=g)), f(torch.rand(c, generator=g) * 1.5 + 0.5)
    eps = float(torch.tensor([1e-5, 1e-3][salt % 2], dtype=torch.float32))
    mom = float(torch.tensor([0.1, 0.3][salt % 2], dtype=torch.float32))
    return w, b, rm, rv, eps, mom


def near_zero_count(case, exact=False):
    """How many activations x * alpha + beta of the case's Gaussian (or exact) input lie within 2^-22 * (|x * alpha| + |beta|) of zero in
    the float64 reference: the elements whose recomputed ReLU mask a differently rounded alpha / beta could flip."""
    x = exact_inputs(case)[0] if exact else gauss_inputs(case)[0]
    w, b, _, _, eps, _ = params(case, salt=int(exact))
    mean, var = ref_moments(x)
    alpha = w / torch.sqrt(var + eps)
    beta = b - mean * alpha
    act = x * _cv(alpha) + _cv(beta)
    return int((act.abs() <= 2.0 ** -22 * ((x * _cv(alpha)).abs() + _cv(beta.abs()))).sum())


# ------------------------------------------------------------------------------------------------------------------ device helpers
class Buf:
    """A tensor of logical shape [N, C, H, W] placed `off` elements into a larger sentinel-filled buffer, in NCHW or channels-last order:
    the kernels must leave every element outside it alone."""

    def __init__(self, shape, dt, layout, off, dev, vals=None):
        n, c, h, w = shape
        numel = n * c * h * w
        self.raw = torch.full((numel + 32,), SENTINEL, dtype=dt, device=dev)
        self.off, self.numel = off, numel
        flat = self.raw[off:off + numel]
        self.t = flat.view(n, h, w, c).permute(0, 3, 1, 2) if layout == NHWC else flat.view(n, c, h, w)
        if vals is not None:
            self.t.copy_(vals.to(dev))

    def guard_ok(self):
        s = torch.full((1,), SENTINEL, dtype=self.raw.dtype, device=self.raw.device)
        return bool((self.raw[:self.off] == s).all()) and bool((self.raw[self.off + self.numel:] == s).all())


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(v, dev):
    return v.float().to(dev)


def _bf16_edges(got):
    """The closed real interval that rounds (to nearest, ties either way) to each bf16 element of got."""
    b = got.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag, neg = b & 0x7fff, (b >> 15) == 1
    val = lambda mm: (mm << 16).contiguous().view(torch.float32).double()
    v, up, dn = val(mag), val(mag + 1), val((mag - 1).clamp_min(0))
    hi_m = (v + up) / 2
    lo_m = torch.where(mag > 0, (v + dn) / 2, -up / 2)
    return torch.where(neg, -hi_m, lo_m), torch.where(neg, -lo_m, hi_m)


class Report:
    """Collects the failures of one case so that every figure is printed before the test asserts."""

    def __init__(self, what):
        self.what, self.fails = what, []

    def expect(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def figure(self, key, value):
        print(f"BNPIN {key} {value:.4f} {self.what}")

    def done(self):
        assert not self.fails, f"{self.what}:\n  " + "\n  ".join(self.fails)


def check_window(rep, name, got, lo, hi):
    """got (bf16 or fp32 tensor) must round from a real value in [lo, hi] (float64 tensors)."""
    ok_f = torch.isfinite(got.float()).all()
    rep.expect(bool(ok_f), f"{name}: non-finite values")
    if got.dtype == BF16:
        glo, ghi = _bf16_edges(got)
        bad = (glo > hi) | (ghi < lo)
    else:
        g = got.double()
        bad = (g > hi) | (g < lo)
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements outside the window; first at {i}: got {float(got[i])!r}, "
                          f"window [{float(lo[i])!r}, {float(hi[i])!r}]")


def ratio_of(got, ref, unit):
    """Worst distance between ref and the reals that round to got, in units of `unit` (elementwise float64)."""
    if got.dtype == BF16:
        glo, ghi = _bf16_edges(got)
        need = torch.maximum(glo - ref, ref - ghi).clamp_min(0.0)
    else:
        need = (got.double() - ref).abs()
    unit = unit.expand_as(need) if unit.dim() else unit
    pos = unit > 0
    if not bool(pos.any()):
        return 0.0 if float(need.max()) == 0.0 else float("inf")
    r = float((need[pos] / unit[pos]).max())
    return float("inf") if float(need[~pos].max() if bool((~pos).any()) else 0.0) > 0 else r


def ulp32(v):
    """Spacing of fp32 at |v| (float64 tensor of fp32 values)."""
    f = v.float().abs()
    return (torch.nextafter(f, torch.full_like(f, float("inf"))) - f).double()


def split_exact(total, parts, gen, coarse=torch.float32):
    """total [C] float64 -> [parts, C] float64 whose sum in slot order is total EXACTLY (asserted): shares 1 .. parts - 1 are coarse
    (24-bit) fractions of total, share 0 the exact remainder."""
    if parts == 1:
        return total[None].clone()
    wts = (torch.rand(parts - 1, total.numel(), generator=gen) * 0.9 + 0.05) / parts
    rest = (total[None] * wts.double()).to(coarse).double()
    s = torch.zeros_like(total)
    for k in range(parts - 1):
        s = s + rest[k]
    out = torch.cat([(total - s)[None], rest])
    s = torch.zeros_like(total)
    for k in range(parts):
        s = s + out[k]
    assert bool((s == total).all()), "the split does not add back to the float64 total exactly"
    return out


def split_f32(total, parts, gen, integer=False):
    """[parts, C] fp32-representable shares (a slab of fp32 partials) and their float64 sum (what the slab holds, the reference);
    integer: integer shares of an integer total, so that the slab holds the total exactly."""
    wts = (torch.rand(parts, total.numel(), generator=gen) + 0.5)
    wts = wts / wts.sum(0, keepdim=True)
    out = (total[None] * wts.double())
    out = out.round() if integer else out.float().double()
    out[0] = (total - out[1:].sum(0)).float().double() if parts > 1 else total.float().double()
    return out, out.sum(0)


def fill_acc(lib, dev, c, sums0, sums1, shift, gen):
    """One accumulator block per entry of the lists (groups): acc[slot][q][C] doubles with the sums split over ALL NS slots, then the
    C floats of shift.  Returns the float64 device tensor."""
    ns, stride = acc_slots(lib, c)
    acc = torch.zeros(stride * len(sums0), dtype=torch.float64)
    for gi, (a, b, sh) in enumerate(zip(sums0, sums1, shift)):
        blk = acc[gi * stride:(gi + 1) * stride]
        pa, pb = split_exact(a, ns, gen), split_exact(b, ns, gen)
        if ns > 1:
            assert bool((pa[1:] != 0).any()) and bool((pb[1:] != 0).any()) or not bool(b.any())
        for s in range(ns):
            blk[(2 * s) * c:(2 * s + 1) * c] = pa[s]
            blk[(2 * s + 1) * c:(2 * s + 2) * c] = pb[s]
        blk[2 * ns * c:2 * ns * c + (c + 1) // 2].view(torch.float32)[:c] = sh.float()
    return acc.to(dev)


def shifted_sums(x, shift):
    d = x - _cv(shift)
    return d.sum((0, 2, 3)), (d * d).sum((0, 2, 3))


def snapshot_shift(mean, gen, exact):
    """A non-integer shift near the mean, as a running-mean snapshot would be (exact check: a multiple of 1/64, so that the shifted sums
    stay exact in float64)."""
    c = mean.numel()
    if exact:
        j = torch.randint(1, 64, (c,), generator=gen).double() * torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
        return mean + j / 64.0
    return (mean + (torch.rand(c, generator=gen).double() - 0.5) * 0.7).float().double()


# --------------------------------------------------------------------------------------------------------------- forward runner
def _scheme(case):
    sums = "f64sum" if case.dt == F32 else "f32sum"
    if case.layout == NCHW:
        return "nchw"
    return ("acc_" if case.entry == "acc0" else "slab_") + sums


def run_forward(pkg, dev, case, exact, res_on, relu, rep, updates=1):
    lib = pkg._lib.load()
    n, c, h, w = case.shape
    hw, m, dt = h * w, n * h * w, case.dt
    groups = 2 if case.entry == "acc_g2" else 1
    mg = m // groups
    gen = torch.Generator().manual_seed(_seed(case, 5))
    if exact:
        x64, dy64, r64, imean = exact_inputs(case)
        for i in range(groups):
            hs = slice(i * (n // groups), (i + 1) * (n // groups))
            assert_exact_preconditions(x64[hs], dy64[hs], imean)
    else:
        x64, _, r64 = gauss_inputs(case)
    w64, b64, rm64, rv64, eps, mom = params(case, salt=int(exact))
    X = Buf(case.shape, dt, case.layout, case.off, dev, x64)
    R = Buf(case.shape, dt, case.layout, case.off, dev, r64) if res_on else None
    Y = Buf(case.shape, dt, case.layout, case.off, dev)
    wd, bd, rm, rv = (_f32(v, dev) for v in (w64, b64, rm64, rv64))
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    stats = torch.full((groups, 4, c), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(lib.afan_bn_workspace_floats(c)), 1024), dtype=torch.float32, device=dev)
    halves = [x64[i * (n // groups):(i + 1) * (n // groups)] for i in range(groups)]
    true = [ref_moments(xh) for xh in halves]                   # float64 moments of the stored tensor, per group
    ref_stats = true
    derived = False                                             # statistics bound: counted roundings (sums given exactly) or measured
    e = case.entry
    common = (DTC[dt], n, c, hw, eps, mom, P(wd), P(bd), int(relu))
    with pkg.ops.bn_running_updates(updates):
        if e == "train":
            rc = lib.afan_bn_train_forward(P(X.t), P(R.t) if R else None, P(Y.t), DTC[dt], case.layout, n, c, hw, eps, mom, P(wd), P(bd), int(relu),
                                           P(ws), P(stats), P(rm), P(rv), P(nbt), _st())
        elif e == "acc0":
            ns, stride = acc_slots(lib, c)
            acc = torch.zeros(stride, dtype=torch.float64, device=dev)
            rc = lib.afan_bn_train_forward_acc(P(X.t), P(R.t) if R else None, P(Y.t), *common, P(acc), 0, P(stats), P(rm), P(rv), P(nbt), 1, _st())
        elif e in ("acc1", "acc_g2"):
            shifts = [snapshot_shift(t[0], gen, exact) for t in true]
            s0, s1 = zip(*[shifted_sums(xh, sh) for xh, sh in zip(halves, shifts)])
            acc = fill_acc(lib, dev, c, s0, s1, shifts, gen)
            rc = lib.afan_bn_train_forward_acc(P(X.t), P(R.t) if R else None, P(Y.t), *common, P(acc), 1, P(stats), P(rm), P(rv), P(nbt), groups,
                                               _st())
            derived = True
        elif e == "partials":
            gparts = 5 if c <= 64 else 70
            sh = snapshot_shift(true[0][0], gen, exact)
            a, b = shifted_sums(x64, sh)
            (pa, a2), (pb, b2) = split_f32(a, gparts, gen), split_f32(b, gparts, gen)
            slab = torch.stack([pa.t(), pb.t()]).contiguous().float().to(dev)       # ws[(q * C + c) * G + g]
            dm = a2 / m
            ref_stats = [(sh + dm, (b2 - a2 * dm).clamp_min(0.0) / m)]              # what the slab says, in float64
            rc = lib.afan_bn_train_forward_partials(P(X.t), P(R.t) if R else None, P(Y.t), *common, P(slab), gparts, P(_f32(sh, dev)), P(stats),
                                                    P(rm), P(rv), P(nbt), _st())
            derived = True
        else:
            raise AssertionError(e)
    assert rc == 0, f"{e}: rc {rc}"
    torch.cuda.synchronize()
    rep.expect(X.guard_ok() and Y.guard_ok() and (R is None or R.guard_ok()), "a launch wrote outside its tensors")
    st = stats.double().cpu()
    xmax = float(x64.abs().max())
    nchw = case.layout == NCHW
    n_mean, n_is = (N_MEAN_ACC, N_INVSTD_ACC) if e.startswith("acc") else (N_MEAN_SLAB, N_INVSTD_SLAB)
    rm_ref, rv_ref = rm64, rv64
    for gi in range(groups):
        mean_p, is_p = st[gi, 0], st[gi, 1]
        mean_r, var_r = ref_stats[gi]
        is_r = 1.0 / torch.sqrt(var_r + eps)
        if exact:
            rep.expect(bool((true[gi][0] == imean).all()), "generator: means not integer")
        if (exact or derived) and not nchw:
            em = float(((mean_p - mean_r).abs() / (U * max(xmax, 1e-30))).max())
            ei = float(((is_p - is_r).abs() / (U * is_r)).max())
            rep.expect(em <= n_mean, f"group {gi}: mean off float64 by {em:.2f} units of 2^-24 * max|x| > {n_mean}")
            rep.expect(ei <= n_is, f"group {gi}: invstd off float64 by {ei:.2f} units of 2^-24 > {n_is}")
            stat_mean_tol = n_mean * U * xmax
            stat_var_rel = 2.0 * n_is * U
        else:
            sch = _scheme(case)
            em = float(((mean_p - mean_r).abs() / (U * (mean_r.abs() + torch.sqrt(var_r))).clamp_min(1e-300)).max())
            ei = float(((is_p - is_r).abs() / (U * is_r)).max())
            rep.figure(f"stat_mean[{sch}]", em)
            rep.figure(f"stat_invstd[{sch}]", ei)
            rep.expect(em <= C_STAT_MEAN[sch], f"mean off float64 by {em:.2f} units of 2^-24 * (|mean| + std) > {C_STAT_MEAN[sch]}")
            rep.expect(ei <= C_STAT_INVSTD[sch], f"invstd off float64 by {ei:.2f} units of 2^-24 > {C_STAT_INVSTD[sch]}")
            stat_mean_tol = float((C_STAT_MEAN[sch] * U * (mean_r.abs() + torch.sqrt(var_r))).max())
            stat_var_rel = 2.0 * C_STAT_INVSTD[sch] * U
        # running statistics: the groups come as consecutive passes
        var_u = var_r * ref_unbias(mg)
        rm_prev, rv_prev = rm_ref, rv_ref
        rm_ref, rv_ref = ref_running(rm_ref, mean_r, mom, updates), ref_running(rv_ref, var_u, mom, updates)
        tol_rm = N_RUNNING * updates * U * (rm_prev.abs() + mean_r.abs()) + stat_mean_tol
        tol_rv = (N_RUNNING * updates + N_UNBIAS) * U * (rv_prev.abs() + var_u) + stat_var_rel * (var_u + eps * ref_unbias(mg))
        if gi == 0:
            tol_rm_acc, tol_rv_acc = tol_rm, tol_rv
        else:
            tol_rm_acc, tol_rv_acc = tol_rm_acc + tol_rm, tol_rv_acc + tol_rv
    rep.expect(bool(((rm.double().cpu() - rm_ref).abs() <= tol_rm_acc).all()),
               f"running_mean off float64: worst {float((rm.double().cpu() - rm_ref).abs().max()):.3e}, bound {float(tol_rm_acc.max()):.3e}")
    rep.expect(bool(((rv.double().cpu() - rv_ref).abs() <= tol_rv_acc).all()),
               f"running_var off float64: worst {float((rv.double().cpu() - rv_ref).abs().max()):.3e}, bound {float(tol_rv_acc.max()):.3e}")
    rep.expect(int(nbt) == updates * groups, f"num_batches_tracked {int(nbt)} != {updates * groups}")
    # coefficients from the published statistics, outputs from the published coefficients
    for gi in range(groups):
        sl = slice(gi * (n // groups), (gi + 1) * (n // groups))
        mean_p, is_p = st[gi, 0], st[gi, 1]
        alpha_h = (is_p * w64).float().double()
        beta_h = (b64 - mean_p * alpha_h).float().double()
        if nchw:
            alpha, beta, slack = alpha_h, beta_h, 2.0 * U * beta_h.abs()
        else:
            alpha, beta, slack = st[gi, 2], st[gi, 3], torch.zeros(c, dtype=torch.float64)
            rep.expect(bool((alpha == alpha_h).all()), f"group {gi}: published alpha is not fl(invstd * w)")
            rep.expect(bool(((beta - beta_h).abs() <= ulp32(beta_h)).all()), f"group {gi}: published beta is not fma(-mean, alpha, b) within an ulp")
        check_affine_output(rep, f"y[group {gi}]", Y.t[sl], X.t[sl], R.t[sl] if R else None, alpha.to(dev), beta.to(dev), slack.to(dev), relu)


def check_affine_output(rep, name, y, x, res, alpha, beta, slack, relu):
    """Every element of y rounds from relu(x * alpha + beta + res) in float64 within 2^-23 * (|x * alpha + beta| + |res|) (+ slack)."""
    val, pre, s = ref_affine(x, alpha, beta, res, False)
    tol = 2.0 * U * s + _cv(slack)
    lo, hi = val - tol, val + tol
    if relu:
        lo, hi = lo.clamp_min(0.0), hi.clamp_min(0.0)
    check_window(rep, name, y, lo, hi)


# ------------------------------------------------------------------------------------------------------------------------ tests
gpu_mark = pytest.mark.gpu


@gpu_mark
@pytest.mark.parametrize("case", [c for c in FWD_CASES if c.entry in ("train", "acc0", "acc1", "acc_g2", "partials")], ids=case_id)
def test_forward_pinned(pkg, gpu, case):
    rep = Report(case_id(case))
    nhwc_plain = case.layout == NHWC and case.entry != "acc_g2"      # (the NCHW kernels refuse a repeat count, grouped launches apply one each)
    for res_on, relu in FWD_COMBOS:
        if not case.cancel:
            run_forward(pkg, gpu, case, True, res_on, relu, rep, updates=2 if (nhwc_plain and relu and not res_on) else 1)
        run_forward(pkg, gpu, case, False, res_on, relu, rep)
    rep.done()


@gpu_mark
@pytest.mark.parametrize("case", [c for c in FWD_CASES if c.entry == "dual"], ids=case_id)
def test_forward_dual_pinned(pkg, gpu, case):
    """y = relu(bn_a(x_a) + bn_b(x_b)), apply_acc_dual_kernel: t = fmaf(x_a, alpha_a, beta_a) + fmaf(x_b, alpha_b, beta_b), three fp32
    roundings, each at most one unit of |x_a alpha_a + beta_a| + |x_b alpha_b + beta_b| in total two: the same 2^-23 window."""
    lib = pkg._lib.load()
    rep = Report(case_id(case))
    n, c, h, w = case.shape
    m, dt = n * h * w, case.dt
    for exact in (True, False):
        gen = torch.Generator().manual_seed(_seed(case, 7 + exact))
        side = []
        for k in range(2):
            x64 = exact_inputs(case, salt=k)[0] if exact else gauss_inputs(case, salt=k)[0]
            w64, b64, rm64, rv64, eps, mom = params(case, salt=k)
            mean, var = ref_moments(x64)
            sh = snapshot_shift(mean, gen, exact)
            a, b = shifted_sums(x64, sh)
            side.append(types.SimpleNamespace(x64=x64, X=Buf(case.shape, dt, NHWC, 0, gpu, x64), w64=w64, b64=b64, rm64=rm64, rv64=rv64, eps=eps,
                                              mom=mom, mean=mean, var=var, acc=fill_acc(lib, gpu, c, [a], [b], [sh], gen), w=_f32(w64, gpu),
                                              b=_f32(b64, gpu), rm=_f32(rm64, gpu), rv=_f32(rv64, gpu),
                                              nbt=torch.zeros((), dtype=torch.int64, device=gpu),
                                              stats=torch.full((4, c), float("nan"), dtype=torch.float32, device=gpu)))
        Y = Buf(case.shape, dt, NHWC, 0, gpu)
        A, B = side
        args = lambda s: (s.eps, s.mom, P(s.w), P(s.b), P(s.acc), P(s.stats), P(s.rm), P(s.rv), P(s.nbt))
        rc = lib.afan_bn_train_forward_acc_dual(P(A.X.t), P(B.X.t), P(Y.t), DTC[dt], n, c, h * w, *args(A), *args(B), _st())
        assert rc == 0
        torch.cuda.synchronize()
        rep.expect(Y.guard_ok(), "the dual launch wrote outside y")
        val = torch.zeros(case.shape, dtype=torch.float64, device=gpu)
        scale = torch.zeros_like(val)
        xmax = max(float(A.x64.abs().max()), float(B.x64.abs().max()))
        for s in side:
            st = s.stats.double().cpu()
            is_r = 1.0 / torch.sqrt(s.var + s.eps)
            em = float(((st[0] - s.mean).abs() / (U * xmax)).max())
            ei = float(((st[1] - is_r).abs() / (U * is_r)).max())
            rep.expect(em <= N_MEAN_ACC and ei <= N_INVSTD_ACC, f"dual statistics off float64: mean {em:.2f}, invstd {ei:.2f} units")
            alpha_h = (st[1] * s.w64).float().double()
            beta_h = (s.b64 - st[0] * alpha_h).float().double()
            rep.expect(bool((st[2] == alpha_h).all()) and bool(((st[3] - beta_h).abs() <= ulp32(beta_h)).all()), "dual: published alpha / beta")
            var_u = s.var * ref_unbias(m)
            for name, got, ref, tol in (("running_mean", s.rm, ref_running(s.rm64, s.mean, s.mom), (N_RUNNING + N_MEAN_ACC) * U * (s.rm64.abs() + xmax)),
                                        ("running_var", s.rv, ref_running(s.rv64, var_u, s.mom),
                                         (N_RUNNING + N_UNBIAS + 2 * N_INVSTD_ACC) * U * (s.rv64.abs() + var_u + s.eps))):
                rep.expect(bool(((got.double().cpu() - ref).abs() <= tol).all()), f"dual {name} off float64")
            rep.expect(int(s.nbt) == 1, "dual num_batches_tracked")
            v = s.X.t.double() * _cv(st[2].to(gpu)) + _cv(st[3].to(gpu))
            val, scale = val + v, scale + v.abs()
        tol = 2.0 * U * scale
        check_window(rep, f"y ({'exact' if exact else 'Gaussian'})", Y.t, (val - tol).clamp_min(0.0), (val + tol).clamp_min(0.0))
    rep.done()


@gpu_mark
@pytest.mark.parametrize("case", [c for c in FWD_CASES if c.entry in ("apply", "affine")], ids=case_id)
def test_eval_forms_pinned(pkg, gpu, case):
    """afan_bn_apply (both layouts) and afan_affine_coefs + afan_affine_apply with given mean / invstd."""
    lib = pkg._lib.load()
    rep = Report(case_id(case))
    n, c, h, w = case.shape
    dt = case.dt
    x64, _, r64 = gauss_inputs(case)
    w64, b64, rm64, rv64, eps, _ = params(case)
    mean64 = rm64
    is64 = (1.0 / torch.sqrt(rv64 + eps)).float().double()
    X, R = Buf(case.shape, dt, case.layout, case.off, gpu, x64), Buf(case.shape, dt, case.layout, case.off, gpu, r64)
    wd, bd, md, isd = (_f32(v, gpu) for v in (w64, b64, mean64, is64))
    alpha_h = (is64 * w64).float().double()
    beta_h = (b64 - mean64 * alpha_h).float().double()
    ws = torch.empty(max(int(lib.afan_bn_workspace_floats(c)), 1024), dtype=torch.float32, device=gpu)
    for res_on, relu in FWD_COMBOS:
        Y = Buf(case.shape, dt, case.layout, case.off, gpu)
        r = R.t if res_on else None
        if case.entry == "apply":
            rc = lib.afan_bn_apply(P(X.t), P(r), P(Y.t), DTC[dt], case.layout, n, c, h * w, P(md), P(isd), P(wd), P(bd), int(relu), P(ws), _st())
            assert rc == 0
            alpha, beta, slack = alpha_h, beta_h, 2.0 * U * beta_h.abs()
        else:
            coefs = torch.full((4, c), float("nan"), dtype=torch.float32, device=gpu)
            assert lib.afan_affine_coefs(P(md), P(isd), P(wd), P(bd), c, P(coefs), _st()) == 0
            assert lib.afan_affine_apply(P(X.t), P(r), P(Y.t), DTC[dt], n, c, h * w, P(coefs), int(relu), _st()) == 0
            k = coefs.double().cpu()
            rep.expect(bool((k[0] == mean64).all()) and bool((k[1] == is64).all()) and bool((k[2] == alpha_h).all()) and
                       bool(((k[3] - beta_h).abs() <= ulp32(beta_h)).all()), "afan_affine_coefs: mean | invstd | alpha | beta")
            alpha, beta, slack = k[2], k[3], torch.zeros(c, dtype=torch.float64)
        torch.cuda.synchronize()
        rep.expect(Y.guard_ok(), "wrote outside y")
        check_affine_output(rep, f"y res{res_on} relu{relu}", Y.t, X.t, r, alpha.to(gpu), beta.to(gpu), slack.to(gpu), relu)
    rep.done()


# -------------------------------------------------------------------------------------------------------------- backward runner
def run_backward(pkg, dev, case, exact, combo, rep):
    lib = pkg._lib.load()
    relu, have_y, want_dres = combo
    n, c, h, w = case.shape
    hw, m, dt, e = h * w, n * h * w, case.dt, case.entry
    groups = 2 if e == "bwd_acc_g2" else 1
    ng = n // groups
    gen = torch.Generator().manual_seed(_seed(case, 9))
    if exact:
        x64, dy64, r64, imean = exact_inputs(case)
    else:
        x64, dy64, r64 = gauss_inputs(case)
    if exact:
        for i in range(groups):
            assert_exact_preconditions(x64[i * ng:(i + 1) * ng], dy64[i * ng:(i + 1) * ng], imean)
    w64, b64, _, _, eps, mom = params(case, salt=int(exact))
    nchw = case.layout == NCHW
    x64, dy64, r64, w64, b64 = (t.to(dev) for t in (x64, dy64, r64, w64, b64))        # the float64 picture is computed on the device
    if exact:
        imean = imean.to(dev)
    X, DY = Buf(case.shape, dt, case.layout, case.off, dev, x64), Buf(case.shape, dt, case.layout, case.off, dev, dy64)
    R = Buf(case.shape, dt, case.layout, case.off, dev, r64)
    Yf = Buf(case.shape, dt, case.layout, case.off, dev)
    DX = Buf(case.shape, dt, case.layout, case.off, dev)
    DR = Buf(case.shape, dt, case.layout, case.off, dev) if want_dres else None
    wd, bd = _f32(w64, dev), _f32(b64, dev)
    ws = torch.empty(max(int(lib.afan_bn_workspace_floats(c)), 1024), dtype=torch.float32, device=dev)
    stats = torch.full((groups, 4, c), float("nan"), dtype=torch.float32, device=dev)
    # the forward that publishes the statistics (and y: with a residual, so that the stored mask differs from the recomputed one)
    for gi in range(groups):
        sl = slice(gi * ng, (gi + 1) * ng)
        rc = lib.afan_bn_train_forward(P(X.t[sl]), P(R.t[sl]) if have_y else None, P(Yf.t[sl]), DTC[dt], case.layout, ng, c, hw, eps, mom, P(wd),
                                       P(bd), int(relu), P(ws), P(stats[gi]), None, None, None, _st())
        assert rc == 0
    torch.cuda.synchronize()
    st = stats.double()
    if exact:
        if nchw:      # Chan merges in fp32: not exact, the measured bound of the forward check
            sd = torch.sqrt(ref_moments(x64)[1])
            em = float(((st[0, 0] - imean).abs() / (U * (imean.abs() + sd)).clamp_min(1e-300)).max())
            rep.expect(em <= C_STAT_MEAN["nchw"], f"forward: published mean off the integer mean by {em:.2f} units > {C_STAT_MEAN['nchw']}")
        else:
            rep.expect(bool((st[:, 0] == imean).all()), "forward: published mean is not the integer mean")
    dwb = torch.zeros(2, c, dtype=torch.float32, device=dev)
    dw0, db0 = (0.0, 3.0) if exact else (0.0, 0.0)
    dwb[1] += db0
    accumulate = int(exact)
    # the float64 picture, per group, from the PUBLISHED statistics
    refs = []
    n_amb = 0
    for gi in range(groups):
        sl = slice(gi * ng, (gi + 1) * ng)
        mean_p, is_p = st[gi, 0], st[gi, 1]
        alpha_h = (is_p * w64).float().double()
        alpha, beta = (alpha_h, (b64 - mean_p * alpha_h).float().double()) if nchw else (st[gi, 2], st[gi, 3])
        mask, amb = None, None
        if relu and have_y:
            mask = Yf.t[sl].double() > 0
        elif relu:
            act = x64[sl] * _cv(alpha) + _cv(beta)          # the product is exact in float64, the sum keeps its sign
            mask = act > 0
            if nchw:                                        # beta of the kernel may sit one ulp from the host's
                amb = act.abs() <= _cv(ulp32(beta))
                n_amb += int(amb.sum())
        refs.append((ref_bn_backward(dy64[sl], x64[sl], mean_p, is_p, alpha, mask), mask, amb, alpha))
    # sums given by the test
    acc = slab = None
    gparts = 0
    if e in ("bwd_acc1", "bwd_acc_g2"):
        acc = fill_acc(lib, dev, c, [r[0]["sg"].cpu() for r in refs], [r[0]["sgx"].cpu() for r in refs],
                       [torch.zeros(c, dtype=torch.float64)] * groups, gen)
    elif e == "bwd_acc0":
        acc = torch.zeros(acc_slots(lib, c)[1], dtype=torch.float64, device=dev)
    elif e == "bwd_partials":
        gparts = 70
        (pa, a2), (pb, b2) = split_f32(refs[0][0]["sg"].cpu(), gparts, gen, exact), split_f32(refs[0][0]["sgx"].cpu(), gparts, gen, exact)
        slab = torch.stack([pa.t(), pb.t()]).contiguous().float().to(dev)
        a2, b2 = a2.to(dev), b2.to(dev)
        if exact:
            assert bool((a2 == refs[0][0]["sg"]).all()) and bool((b2 == refs[0][0]["sgx"]).all()) and float(pb.abs().sum(0).max()) < 2.0 ** 24
        r0 = refs[0][0]
        m_ = float(m)
        is_p, alpha = st[0, 1], refs[0][3]
        bco, dco = -alpha * is_p * is_p * b2 / m_, -alpha * a2 / m_
        xm = x64 - _cv(st[0, 0])
        r0.update(sg=a2, sgx=b2, db=a2, dw=is_p * b2, dx=r0["g"] * _cv(alpha) + xm * _cv(bco) + _cv(dco),
                  s_dx=(r0["g"] * _cv(alpha)).abs() + xm.abs() * _cv(bco.abs()) + _cv(dco.abs()))
    yarg = P(Yf.t) if (relu and have_y) else None
    if e in ("bwd", "bwd_partials"):
        rc = lib.afan_bn_backward(P(DY.t), P(X.t), yarg, P(DX.t), P(DR.t) if DR else None, DTC[dt], case.layout, n, c, hw, P(stats), P(wd), P(bd),
                                  int(relu), P(ws), P(dwb[0]), P(dwb[1]), accumulate, P(slab), gparts, _st())
    else:
        rc = lib.afan_bn_backward_acc(P(DY.t), P(X.t), yarg, P(DX.t), P(DR.t) if DR else None, DTC[dt], n, c, hw, P(stats), int(relu), P(acc),
                                      int(e != "bwd_acc0"), P(dwb[0]), P(dwb[1]), accumulate, groups, _st())
    assert rc == 0, f"{e}: rc {rc}"
    torch.cuda.synchronize()
    rep.expect(DX.guard_ok() and (DR is None or DR.guard_ok()) and X.guard_ok() and DY.guard_ok(), "a launch wrote outside its tensors")
    tag = f"{'exact' if exact else 'Gaussian'} relu{relu} y{have_y} dres{want_dres}"
    # mask / dres
    # an NCHW kernel's own beta may sit one ulp from the host's: the table's inputs keep every activation further from zero than that
    # (test_bn_pinned_ref.py), so no element is exempt and everything below is checked
    rep.expect(n_amb == 0, f"{tag}: {n_amb} activations within an ulp of beta of zero: the recomputed mask is not reproducible there")
    if DR is not None:
        got = DR.t.double()
        want = torch.cat([r[0]["g"] for r in refs])
        bad = got != want
        rep.expect(not bool(bad.any()), f"{tag}: dres differs from the masked gradient at {int(bad.sum())} elements")
    sums = "f64sum" if (dt == F32 and not nchw) else "f32sum"
    given = e in ("bwd_acc1", "bwd_acc_g2")
    c_dx, c_dw, c_db = (N_DX_ACC, N_DW_ACC, N_DB_ACC) if given else (C_DX[sums], C_DW[sums], C_DB[sums])
    dw_ref = sum(r[0]["dw"] for r in refs)
    db_ref = sum(r[0]["db"] for r in refs)
    s_dw = sum(r[0]["s_dw"] for r in refs)
    s_db = sum(r[0]["s_db"] for r in refs)
    dw_got, db_got = dwb[0].double() - dw0, dwb[1].double()
    if exact:
        rep.expect(bool((db_got == db_ref + db0).all()), f"{tag}: dbias is not the integer sum bit for bit "
                                                        f"(worst {float((db_got - db_ref - db0).abs().max())})")
        if not nchw:
            want = sum((r[0]["sgx"] * st[gi, 1]).float().double() for gi, r in enumerate(refs))
            lim = ulp32(want) * (groups - 1)        # grouped: one more fp32 addition
            rep.expect(bool(((dw_got - want).abs() <= lim).all()), f"{tag}: dweight is not fl(invstd * integer sum) "
                                                                   f"(worst {float((dw_got - want).abs().max()):.3e})")
    rdw = ratio_of(dwb[0] - dw0, dw_ref, U * s_dw)
    rdb = ratio_of(dwb[1] - db0, db_ref, U * s_db)
    dx_ref = torch.cat([r[0]["dx"] for r in refs])
    s_dx = torch.cat([r[0]["s_dx"] for r in refs])
    rdx = ratio_of(DX.t, dx_ref, U * s_dx)
    if not given:
        rep.figure(f"dx[{sums}]", rdx)
        rep.figure(f"dw[{sums}]", rdw)
        rep.figure(f"db[{sums}]", rdb)
    rep.expect(rdw <= c_dw, f"{tag}: dweight off float64 by {rdw:.2f} units of 2^-24 * sum |g xhat| > {c_dw}")
    rep.expect(rdb <= c_db, f"{tag}: dbias off float64 by {rdb:.2f} units of 2^-24 * sum |g| > {c_db}")
    tol = c_dx * U * s_dx
    check_window(rep, f"{tag}: dx (worst ratio {rdx:.2f}, bound {c_dx})", DX.t, dx_ref - tol, dx_ref + tol)


@gpu_mark
@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_backward_pinned(pkg, gpu, case):
    rep = Report(case_id(case))
    for combo in BWD_COMBOS:
        run_backward(pkg, gpu, case, True, combo, rep)
        run_backward(pkg, gpu, case, False, combo, rep)
    rep.done()


@gpu_mark
@pytest.mark.parametrize("case", AFFINE_BWD_CASES, ids=case_id)
def test_affine_relu_bwd_pinned(pkg, gpu, case):
    """g = dy where the stored y > 0 (relu) else dy; dres = g bit for bit; dx = g * alpha[c]: ONE fp32 rounding, so dx must be the RNE
    of the float64 product (bf16: through fp32, the other neighbour only within 2^-24 * |g alpha| of a midpoint)."""
    lib = pkg._lib.load()
    rep = Report(case_id(case))
    n, c, h, w = case.shape
    dt = case.dt
    y64, dy64, _ = gauss_inputs(case)
    alpha64 = params(case)[0]
    DY, Y = Buf(case.shape, dt, case.layout, case.off, gpu, dy64), Buf(case.shape, dt, case.layout, case.off, gpu, y64)
    al = _f32(alpha64, gpu)
    for relu, want_dx, want_dres in AFFINE_BWD_COMBOS:
        DX = Buf(case.shape, dt, case.layout, case.off, gpu) if want_dx else None
        DR = Buf(case.shape, dt, case.layout, case.off, gpu) if want_dres else None
        rc = lib.afan_affine_relu_bwd(P(DY.t), P(Y.t) if relu else None, P(al), P(DX.t) if DX else None, P(DR.t) if DR else None, DTC[dt],
                                      case.layout, n, c, h * w, int(relu), _st())
        assert rc == 0
        torch.cuda.synchronize()
        g = torch.where(y64 > 0, dy64, torch.zeros_like(dy64)) if relu else dy64
        tag = f"relu{relu} dx{want_dx} dres{want_dres}"
        if DR:
            rep.expect(DR.guard_ok() and bool((DR.t.double().cpu() == g).all()), f"{tag}: dres is not the masked gradient bit for bit")
        if DX:
            ref = (g * _cv(alpha64)).to(gpu)
            tol = U * ref.abs()
            rep.expect(DX.guard_ok(), f"{tag}: wrote outside dx")
            check_window(rep, f"{tag}: dx", DX.t, ref - tol, ref + tol)
    rep.done()


# ------------------------------------------------------------------------------------------------------------ running-stat replay
@gpu_mark
def test_running_update_replay_pinned(pkg, gpu):
    """ops.record_bn_updates().replay() (afan_bn_running_update_batched) and the single-item afan_bn_running_update: one more update
    from saved mean | invstd, the variance recovered as 1 / invstd^2 - eps, for three BatchNorms of different C, M, eps and momentum."""
    lib = pkg._lib.load()
    rep = Report("replay")
    items = [((2, 64, 5, 7), 1e-5, 0.1, BF16), ((3, 48, 9, 9), 1e-3, 0.3, F32), ((1, 8, 1, 2), 1e-2, 0.01, BF16)]
    bns = []
    with pkg.ops.record_bn_updates() as rec:
        for i, (shape, eps, mom, dt) in enumerate(items):
            case = _c("train", dt, shape)
            x64 = gauss_inputs(case, salt=i)[0]
            w64, b64, rm64, rv64, _, _ = params(case, salt=i)
            eps, mom = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(mom, dtype=torch.float32))
            x = Buf(shape, dt, NHWC, 0, gpu, x64).t
            rm, rv, nbt = _f32(rm64, gpu), _f32(rv64, gpu), torch.zeros((), dtype=torch.int64, device=gpu)
            _, stats = pkg.ops.bn_train_forward(x, _f32(w64, gpu), _f32(b64, gpu), None, False, eps, mom, rm, rv, nbt)
            sch = ("acc_" if pkg.ops.bn_acc_ok(x) else "slab_") + ("f64sum" if dt == F32 else "f32sum")     # the scheme ops took
            bns.append((shape, eps, mom, rm, rv, nbt, stats, (x64, sch)))
    torch.cuda.synchronize()
    before = [(b[3].double().cpu(), b[4].double().cpu()) for b in bns]
    singles = [(b[3].clone(), b[4].clone(), b[5].clone()) for b in bns]
    rec.replay()
    for (shape, eps, mom, rm, rv, nbt, stats, _), (rm1, rv1, nbt1) in zip(bns, singles):
        m = shape[0] * shape[2] * shape[3]
        assert lib.afan_bn_running_update(P(stats), shape[1], float(m), eps, mom, P(rm1), P(rv1), P(nbt1), _st()) == 0
    torch.cuda.synchronize()
    for (shape, eps, mom, rm, rv, nbt, stats, x64), (rm0, rv0), (rm1, rv1, nbt1) in zip(bns, before, singles):
        m = shape[0] * shape[2] * shape[3]
        st = stats.double().cpu()
        x64, sch = x64
        mean_r, var_r = ref_moments(x64)                                              # float64 of the stored tensor
        var_u = var_r * ref_unbias(m)
        rm_ref, rv_ref = ref_running(rm0, mean_r, mom), ref_running(rv0, var_u, mom)
        unit = U * (rv0.abs() + (var_u + eps * ref_unbias(m)))
        for name, gm, gv, gn in (("batched", rm, rv, nbt), ("single", rm1, rv1, nbt1)):
            r = float(((gv.double().cpu() - rv_ref).abs() / unit).max())
            rep.figure(f"replay[{name}]", r)
            rep.expect(r <= C_REPLAY, f"{name} {shape}: running_var off float64 by {r:.2f} units > {C_REPLAY}")
            rep.expect(bool(((gm.double().cpu() - rm_ref).abs() <= (N_RUNNING + C_STAT_MEAN[sch]) * U * (rm0.abs() + mean_r.abs() + var_r.sqrt())).all()),
                       f"{name} {shape}: running_mean")
            rep.expect(int(gn) == 2, f"{name} {shape}: num_batches_tracked {int(gn)} != 2")
    rep.done()


# --------------------------------------------------------------------------------------------------------------------- coverage
def test_table_reaches_every_listed_variant():
    """Every case reaches at least one listed variant, every listed variant is reached by a case: from the restated predicates alone."""
    reached = collections.Counter()
    for case in FWD_CASES + BWD_CASES + AFFINE_BWD_CASES:
        v = variants_of(case)
        assert v & set(EXPECTED_VARIANTS), f"{case_id(case)} reaches no listed variant: {sorted(v)}"
        reached.update(v)
    missing = [v for v in EXPECTED_VARIANTS if not reached[v]]
    assert not missing, f"listed variants that no case reaches: {missing}"
    extra = sorted(set(reached) - set(EXPECTED_VARIANTS))
    assert not extra, f"variants reached but not listed: {extra}"
    assert len(set(EXPECTED_VARIANTS)) == len(EXPECTED_VARIANTS)


def test_constants_match_sources():
    """The constants the predicates use are the ones in the sources."""
    src = lambda f: open(os.path.join(ROOT, "cv_a-fan_amd", "csrc", f)).read()
    nchw, nhwc = src("afan_bn.hip"), src("afan_bn_nhwc.hip")
    assert int(re.search(r"constexpr int MAX_SLICES = (\d+);", nchw).group(1)) == MAX_SLICES
    assert int(re.search(r"constexpr int BLOCK = (\d+);", nchw).group(1)) == BLOCK == int(re.search(r"constexpr int BLOCK = (\d+);", nhwc).group(1))
    assert int(re.search(r"constexpr int MAX_G = (\d+);", nhwc).group(1)) == MAX_G
    assert int(re.search(r'"AFAN_BN_MAXBLOCKS"\); return v \? atoi\(v\) : (\d+);', nhwc).group(1)) == APPLY_CAP
    shapes = {(c.dt, c.shape) for c in FWD_CASES if "nhwc_cap" in paths_of(c)}
    assert {(BF16, (2, 2048, 33, 33)), (BF16, (65, 16, 64, 64))} <= shapes
    for c in FWD_CASES:
        assert c.shape[0] * c.shape[1] * c.shape[2] * c.shape[3] * (4 if c.dt == F32 else 2) < 20e6, case_id(c)


@gpu_mark
def test_predicates_agree_with_library(pkg, gpu):
    """afan_bn_acc_supported / ops.bn_acc_ok against the restated predicate; NS of every channel count of the table."""
    lib = pkg._lib.load()
    assert not [k for k in os.environ if k.startswith("AFAN_BN_")], "tuning variables change the paths this table expects"
    for dt in (F32, BF16):
        for c in sorted({c.shape[1] for c in FWD_CASES + BWD_CASES} | {1, 2, 12, 24, 40, 96, 256, 4096, 8192}):
            want = nhwc_vec_ok(dt, c)
            assert bool(lib.afan_bn_acc_supported(DTC[dt], c)) == want, (dt, c)
            x = torch.zeros((2, c, 2, 2), dtype=dt, device=gpu).contiguous(memory_format=torch.channels_last)
            assert pkg.ops.bn_acc_ok(x) == (want and pkg.ops.BN_ACC), (dt, c)
            if want:
                ns, stride = acc_slots(lib, c)
                assert ns == max(1, min(16, 1 << max(0, (1024 // c).bit_length() - 1))) and stride == pkg.ops.acc_block_doubles(c)
    assert lib.afan_bn_acc_supported(7, 64) == 0
