"""The feature-mixing kernels of csrc/afan_mix.hip (mix_feature in both layouts, the fused SAT lerp_mix, the learnable mix_w pair), the
classifier head and the one-launch cross-entropy of csrc/afan_head.hip, and the perturbation norms, pinned ELEMENTWISE to float64.
Every kernel is called through the C ABI with ctypes, so that buffers, alignment, NULLs and workspaces are the test's choice.  The
references are tests/tail_pinned_refs.py (float64, written from the definitions; tests/test_tail_pinned_ref.py checks them on the
CPU against torch in float64 and the fp32 C oracle, and holds the coverage test of the tables below).

Two checks per kernel:
  * exact, where fp32 cannot round: the head on small-integer x, ternary W, integer bias and dlogits with HW a power of two (pooled,
    logits, dW, db, fp32 dx equal float64 bit for bit in any summation order, bf16 dx is its RNE; accumulate = 1 onto integer
    contents too), the mix_w gradient on ternary gradients and integer operands; unmasked lerp points, the mix_w forward and linf
    are bit for bit on ANY operands (the reference reproduces their fp32 roundings).
  * rounding-aware: |got - float64| <= C * 2^-24 * S elementwise, S the same operation on absolute values (for mix_feature: the
    sensitivities of the one-pass moments propagated through the expression, tail_pinned_refs.mix_feature).  C is counted from the
    kernel's expression (the c_* functions below) where that is practical; for the propagated statistic error of mix_feature and
    for the device library's expf / logf it is three times the worst ratio measured on an MI355X against the float64 reference
    (the *_MEASURED constants, each next to the case it came from): room for another summation order, none for a dropped term.
    A bf16 result must be the RNE bf16 of float64; the other neighbour only where float64 lies within that noise of the rounding
    midpoint, for at most 1 % of a case's elements.
Every case prints "TAILPIN <form> <worst ratio> <case>" (run with -s) before it asserts: the worst |got - float64| / (C * 2^-24 * S).

Worst ratios on an MI355X (this table, against the final constants; every exact and bit-for-bit check holds; the share of bf16 outputs
that are not the RNE bf16 of float64 is at most 1e-4 in every case):
    mix_feature f32    nchw staged 0.307 (C = 2048)   nchw re-read 0.264 (C = 6000)   nhwc KEEP 8 0.333 (C = 2, 32 769 pixels)   KEEP 20 0.165
    mix_feature bf16   nchw staged 0.017   nchw re-read 0.003   nhwc KEEP 8 0.000   KEEP 20 0.025
    special rows f32   nchw / nhwc: clean == adv 0.015 / 0.022   constant clean 0.008 / 0.005   constant adv 0.079 / 0.112
                       ill-conditioned 0.061 / 0.091   outlier shift 0.248 / 0.184   eps = 0 the same figures (gauss 0.115 / 0.088)
    lerp_mix           mixed points nchw 0.333 (C = 6000, 4 points)   nhwc 0.214; unmasked points and fused == separate: bit for bit
    mix_w gradient     f32 0.054   bf16 0.030 (n = 5; forward bit for bit)
    head               pooled scalar 0.574 (HW = 3)   vec 0.267   logits scalar 0.030   vec 0.038   dx f32 0.650 (K = 1)   bf16 0.000
                       dW 0.147   db 0.109
    cross-entropy      dlogits row 0.327   wide 0.333   loss row 0.131   wide 0.333
    perturb_norms      l2 0.053 (linf bit for bit)
*_MEASURED (3 x the worst ratio against the float64 reference with the constant at 1): MIX_NCHW 4.18 (1.3921, lerp_mix nchw C = 6000),
MIX_NHWC 2.94 (0.9779, mix_feature nhwc C = 2, 32 769 pixels), CE_GRAD 5.57 (1.8542, 1024 x 64 with -inf), CE_LOSS 3.54 (1.1790, 20 x 1000).
The module's 100 GPU cases take 2.9 s in all on an MI355X, the slowest 0.16 s.

Coverage: EXPECTED_VARIANTS lists every instantiation and inner path the tables must reach; tests/test_tail_pinned_ref.py holds the test
that the dispatch predicates restated in tests/tail_pinned_refs.py map the tables onto exactly that list.
"""
import collections
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import tail_pinned_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF16: "bf16"}
DTC = {F32: 0, BF16: 1}
NCHW, NHWC = 0, 1
LAY = {NCHW: "nchw", NHWC: "nhwc"}
U = R.U
BF16_SHARE_CAP = 0.01
EPS = 1e-5

# ---- measured constants: 3 x the worst ratio |got - float64| / (2^-24 * S) over the tables, on an MI355X -----------------------------
MIX_NCHW_MEASURED = 4.18      # 3 x 1.3921: lerp_mix nchw-n1-c6000-hw6-points4 (the unstaged re-read: 188 channels per thread's chain)
MIX_NHWC_MEASURED = 2.94      # 3 x 0.9779: mix_feature nhwc-f32-n1-c2-hw32769 (two channels: one rounding of the mean is the whole error)
CE_GRAD_MEASURED = 5.57       # 3 x 1.8542: cross-entropy 1024x64, the table with a row of equal logits and a -inf class, ce_fwd_wide_kernel
CE_LOSS_MEASURED = 3.54       # 3 x 1.1790: cross-entropy 20x1000, Gaussian logits, ce_fwd_wide_kernel


# ---- roundings counted from the kernels' expressions (-ffp-contract=off: every operation rounds once) ------------------------------
def c_mix_w_dot(n, acc):
    """mix_w_dot_kernel + mix_w_dot_finalize_kernel: s += g * (adv - clean) per element of the thread's grid-stride chain (the
    difference 1, the product 1, one add per element), the wave butterfly (6), the block's 4 waves (4), the finalize wave's chain
    over the block partials (ceil(blocks / 64)) and butterfly (6), the add onto *dw (accumulate)."""
    grid = R.mix_w_dot_grid(n)
    return 2 + -(-n // (grid * R.BLOCK)) + 6 + 4 + -(-grid // R.WAVE) + 6 + acc


def c_pool(form, c, hw):
    """pooled = (sum over HW) * (1 / HW): the scalar kernel adds HW values in order (HW - 1), the vector kernel ceil(HW / G) per pixel
    group and then the G group sums (those of empty groups are exact zeros); 1 / HW rounds (1), the product rounds (1)."""
    if form == "scalar":
        return hw + 1
    g = R.head_vec_groups(c)
    return -(-hw // g) + min(g, hw) + 1


def c_logits(form, c, hw):
    """logits: one fused multiply-add per channel of the thread's chain (ceil(C / 256)) on a pooled value carrying c_pool, the wave
    butterfly (6), bias + the 4 waves (4)."""
    return c_pool(form, c, hw) + -(-c // R.BLOCK) + 6 + 4


def c_dx(k):
    """head_bwd_dx_kernel: K fused multiply-adds, 1 / HW rounds, the product rounds."""
    return k + 2


def c_dw(b, acc):
    """head_bwd_dw_kernel: a slice's chain of ceil(B / 16) fused multiply-adds (plain adds for db), the 16 slice sums, the add onto
    the contents (accumulate)."""
    return -(-b // R.DW_SLICES) + R.DW_SLICES + acc


def c_norm_ss(per_sample):
    """pgd_step_norms_kernel<STEP = false> + norms_finalize_kernel: d = xa - xc rounds (2 on d * d), the product (1), a thread's
    chain over its chunk (NORM_CHUNK / 256), the wave butterfly (6), the 4 waves (4), the finalize chain over the slices
    (ceil(slices / 64)) and butterfly (6).  l2 = sqrt(ss): half the relative error of ss, plus the root's own rounding."""
    slices = -(-per_sample // R.NORM_CHUNK)
    return 3 + R.NORM_CHUNK // R.BLOCK + 6 + 4 + -(-slices // R.WAVE) + 6


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def fptr(ws):
    return (ctypes.c_float * max(len(ws), 1))(*[float(w) for w in ws])


class Report:
    def __init__(self, what):
        self.what, self.fails = what, []

    def expect(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def figure(self, key, value):
        print(f"TAILPIN {key} {value:.4f} {self.what}")

    def done(self):
        assert not self.fails, f"{self.what}:\n  " + "\n  ".join(self.fails[:12])


def bits_equal(a, b):
    """Same bits (NaNs included) of two tensors of one dtype."""
    v = torch.int32 if a.dtype == F32 else torch.int16
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def check_bits(rep, name, got, want):
    """got and want (same dtype) bit for bit, -0.0 and 0.0 taken as equal values."""
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements differ; first at {i}: got {float(got[i])!r}, expected {float(want[i])!r}")


def check_exact(rep, name, got, ref):
    """ref (float64) is an fp32 value: fp32 got equals it bit for bit, bf16 got is its RNE rounding."""
    assert bool((ref.float().double() == ref).all()), f"{name}: the float64 result is not an fp32 value"
    check_bits(rep, name, got, R.rne_bf16(ref) if got.dtype == BF16 else ref.float())


def check_window(rep, key, name, got, ref, noise):
    """got must round from a real value within `noise` of ref (float64); prints the worst ratio.  bf16: at most BF16_SHARE_CAP of
    the elements may be anything but the RNE bf16 of ref."""
    rep.expect(bool(torch.isfinite(got.float()).all()), f"{name}: non-finite values")
    if got.dtype == BF16:
        glo, ghi = R.bf16_edges(got)
        need = torch.maximum(glo - ref, ref - ghi).clamp_min(0.0)
        share = float((got != R.rne_bf16(ref)).double().mean())
        rep.figure(key + "|share", share)
        rep.expect(share <= BF16_SHARE_CAP, f"{name}: {share:.4f} of the elements are not the RNE bf16 of float64")
    else:
        need = (got.double() - ref).abs()
    need = torch.nan_to_num(need, nan=float("inf"))
    noise = noise.expand_as(need)
    pos = noise > 0
    ratio = float((need[pos] / noise[pos]).max()) if bool(pos.any()) else 0.0
    if bool((need[~pos] > 0).any()):
        ratio = float("inf")
    rep.figure(key, ratio)
    bad = need > noise
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements outside the window (worst ratio {ratio:.3f}); first at {i}: got "
                          f"{float(got[i])!r}, float64 {float(ref[i])!r} +- {float(noise[i])!r}")


def to_dev(t64, dt, dev, off=0):
    """A device copy of the values starting `off` elements past a 16-byte boundary."""
    buf = torch.zeros((t64.numel() + 16,), dtype=dt, device=dev)
    view = buf[off:off + t64.numel()]
    view.copy_(t64.reshape(-1).to(dt))
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return view


def stored(t, dt):
    """float64 of the values as dtype dt stores them."""
    return t.to(dt).double()


# ================================================================================================================== mix_feature
MC = collections.namedtuple("MC", "layout dt n c hw kind")


def mix_id(c):
    return f"{LAY[c.layout]}-{DTN[c.dt]}-n{c.n}-c{c.c}-hw{c.hw}" + ("" if c.kind == "gauss" else "-" + c.kind)


MIX_CASES = []
for _dt in (F32, BF16):
    MIX_CASES += [
        # each pixel tile of mix_feature_kernel, hw = 7 x 11 above the tile with a ragged last tile
        MC(NCHW, _dt, 1, 19, 77, "gauss"), MC(NCHW, _dt, 1, 304, 77, "gauss"), MC(NCHW, _dt, 1, 512, 77, "gauss"), MC(NCHW, _dt, 1, 1024, 77, "gauss"),
        # tiny plane (hw below half the tile: 64 -> 8 pixels, 32 channel groups for 19 channels); empty and ragged channel groups
        MC(NCHW, _dt, 1, 19, 5, "gauss"), MC(NCHW, _dt, 1, 2, 15, "gauss"), MC(NCHW, _dt, 1, 3, 15, "gauss"),
        # opt-in LDS (staged tile of 71 680 B); the unstaged re-read; more than one sample
        MC(NCHW, _dt, 1, 2048, 9, "gauss"), MC(NCHW, _dt, 1, 6000, 6, "gauss"), MC(NCHW, _dt, 3, 19, 77, "gauss"),
        # a single plane pixel: the channels-last kernel
        MC(NCHW, _dt, 5, 2048, 1, "gauss"), MC(NCHW, _dt, 5, 40, 1, "gauss"),
        # the special rows on both layouts
        MC(NCHW, _dt, 1, 512, 6, "rows"), MC(NHWC, _dt, 1, 512, 6, "rows"),
    ]
    # mix_feature_nhwc_kernel<T, KEEP>
    MIX_CASES += [MC(NHWC, _dt, 2, _c, 9, "gauss") for _c in (2, 40, 65, 512, 520, 1280, 1300)]
    MIX_CASES += [MC(NHWC, _dt, 1, 2, 4 * R.NHWC_GRID_CAP + 1, "gauss")]
# one channel: the unbiased variance is 0 / 0
MIX_CASES += [MC(NCHW, F32, 1, 1, 6, "c1"), MC(NHWC, F32, 1, 1, 6, "c1")]


def mix_is_nhwc(c):
    return c.layout == NHWC or c.hw == 1


def mix_lanes(c):
    """Threads that share one pixel's channels: the 64 lanes of a wave, the G channel groups of the pixel-tile kernel."""
    return R.WAVE if mix_is_nhwc(c) else R.mix_plan(c.c, c.hw)["groups"]


def mix_measured(c):
    return MIX_NHWC_MEASURED if mix_is_nhwc(c) else MIX_NCHW_MEASURED


def mix_form(c):
    d = DTN[c.dt]
    if mix_is_nhwc(c):
        return f"mix_nhwc<{d},{R.nhwc_keep(c.c)}>"
    return f"mix<{d},{'stage' if R.mix_plan(c.c, c.hw)['stage'] else 'reread'}>"


def mix_labels(c):
    d = DTN[c.dt]
    out = {mix_form(c)}
    if c.kind != "gauss":
        return out | {f"mix|{d}|{LAY[c.layout]}|{c.kind}"}
    if mix_is_nhwc(c):
        keep = R.nhwc_keep(c.c)
        if c.layout == NCHW:
            out.add(f"mix|{d}|hw1|keep{keep}")
        if c.c < R.WAVE:
            out.add(f"mix_nhwc|{d}|empty_lanes")
        if c.c == R.WAVE * keep:
            out.add(f"mix_nhwc<{d},{keep}>|full")
        elif c.c > R.WAVE * R.KEEP_LARGE:
            out.add(f"mix_nhwc|{d}|reread")
        if c.n * c.hw > R.nhwc_grid(c.n * c.hw) * (R.BLOCK // R.WAVE):
            out.add(f"mix_nhwc|{d}|grid_trip2")
        return out
    p = R.mix_plan(c.c, c.hw)
    out.add(f"mix|{d}|tiny" if p["tiny"] else f"mix|{d}|pix{p['pix']}")
    if p["optin"]:
        out.add(f"mix|{d}|optin")
    if c.hw > p["pix"] and c.hw % p["pix"]:
        out.add(f"mix|{d}|ragged_tile")
    if c.n > 1:
        out.add(f"mix|{d}|n>1")
    if c.c < p["groups"]:
        out.add(f"mix|{d}|empty_groups")
    elif c.c % p["groups"]:
        out.add(f"mix|{d}|c%g")
    return out


@functools.lru_cache(maxsize=None)
def mix_rows(c):
    """(clean, adv) as float64 [N, HW, C] of the stored values; the seed depends on the shape only."""
    gen = torch.Generator().manual_seed(c.c * 31 + c.hw + c.n)
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    # (means a few standard deviations off zero, as behind a ReLU: the outputs do not crowd around zero, where every window is wide
    # against the bf16 spacing and the reference itself could not keep the midpoint rule)
    clean, adv = rn(c.n, c.hw, c.c) * 0.5 + 1.5, rn(c.n, c.hw, c.c) * 0.35 + 1.0
    if c.kind == "rows":
        assert c.n == 1 and c.hw == 6
        adv[0, 0] = clean[0, 0]                                                  # clean == adv: the output is clean
        clean[0, 1] = 0.75                                                       # a constant pixel: var = 0, eps alone
        adv[0, 2] = -1.5
        clean[0, 3], adv[0, 3] = 1e3 + 1e-2 * rn(c.c), 1e3 + 1e-2 * rn(c.c)      # |mean| / std = 1e5: the one-pass moments' weak spot
        clean[0, 4, 0], adv[0, 4, 0] = 1e3, -1e3                                 # the first channel (a shift) is an outlier
    return stored(clean, c.dt), stored(adv, c.dt)


# rows of the "rows" case that are not constant as stored, so that eps = 0 leaves them finite (bf16 stores 1e3 + 1e-2 N(0, 1) as 1e3)
ROWS_EPS0 = {F32: (0, 3, 4, 5), BF16: (0, 4, 5)}


def run_mix(lib, dev, c, clean, adv, eps, nhwc_entry=False):
    """clean, adv float64 [N, HW, C] -> (rc, out [N, HW, C] of dtype c.dt on the CPU); the output is prefilled with NaN."""
    n, hw, ch = clean.shape
    mem = (lambda t: t) if c.layout == NHWC else (lambda t: t.permute(0, 2, 1))
    cd, ad = to_dev(mem(clean).contiguous(), c.dt, dev), to_dev(mem(adv).contiguous(), c.dt, dev)
    out = torch.full((n * hw * ch,), float("nan"), dtype=c.dt, device=dev)
    fn = lib.afan_mix_feature_nhwc if (c.layout == NHWC or nhwc_entry) else lib.afan_mix_feature
    rc = fn(P(cd), P(ad), P(out), n, ch, hw, eps, DTC[c.dt], _st())
    o = out.cpu()
    return rc, (o.view(n, hw, ch) if c.layout == NHWC else o.view(n, ch, hw).permute(0, 2, 1))


@pytest.mark.parametrize("case", MIX_CASES, ids=mix_id)
def test_mix_feature_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    form = mix_form(c)
    rep = Report(f"{mix_id(c)} expected {form}")
    clean, adv = mix_rows(c)
    runs = [("", EPS, clean, adv)]
    if c.kind == "rows":
        runs.append(("|eps0", 0.0, clean[:, ROWS_EPS0[c.dt], :], adv[:, ROWS_EPS0[c.dt], :]))
    for tag, eps, cl, ad in runs:
        rc, got = run_mix(lib, gpu, c, cl, ad, eps)
        rep.expect(rc == 0, f"afan_mix_feature{tag} returned {rc}")
        if rc:
            continue
        ref, s = R.mix_feature(cl.reshape(-1, c.c), ad.reshape(-1, c.c), eps, mix_lanes(c))
        got = got.reshape(-1, c.c)
        if c.kind == "c1":
            rep.expect(bool(torch.isnan(ref).all()) and bool(torch.isnan(got).all()), "one channel: NaN expected everywhere")
            continue
        noise = mix_measured(c) * U * s
        if c.kind == "rows":
            key = f"mix_rows|{LAY[c.layout]}|{DTN[c.dt]}{tag}"
            names = ("clean==adv", "constant clean", "constant adv", "ill-conditioned", "outlier shift", "gauss")
            for j, r in enumerate(range(6) if not tag else ROWS_EPS0[c.dt]):
                check_window(rep, f"{key}|{names[r].replace(' ', '_')}", f"row {names[r]}{tag}", got[j:j + 1], ref[j:j + 1], noise[j:j + 1])
        else:
            check_window(rep, form, "out", got, ref, noise)
        if c.layout == NCHW and c.hw == 1:       # the same bytes either way, and the same kernel: the same bits
            rc2, got2 = run_mix(lib, gpu, c, cl, ad, eps, nhwc_entry=True)
            rep.expect(rc2 == 0 and bits_equal(got2.reshape(-1, c.c), got), "hw == 1: afan_mix_feature and afan_mix_feature_nhwc differ in bits")
    rep.done()


# ================================================================================================================ afan_lerp_mix
LMC = collections.namedtuple("LMC", "layout n c hw n_points")
LERP_CASES = [LMC(_l, 2, _c, 77 if _l == NCHW else 9, _p) for _l, _c in ((NCHW, 19), (NHWC, 65)) for _p in (2, 3, 4, 5)] + [
    LMC(NCHW, 1, 232, 72, 5),            # 5 sets of partial moments push the staged launch over 64 KB: an opt-in only the fused kernel has
    LMC(NCHW, 1, 6000, 6, 4), LMC(NHWC, 1, 6000, 3, 4),
    LMC(NCHW, 3, 40, 1, 5), LMC(NCHW, 3, 2048, 1, 3),
]


def lerp_id(c):
    return f"{LAY[c.layout]}-n{c.n}-c{c.c}-hw{c.hw}-points{c.n_points}"


def lerp_masks(n_points):
    """All-on, all-off, mixed with the end point on, mixed with the end point off (bit j - 1: point j is mixed)."""
    npts = n_points - 1
    full = (1 << npts) - 1
    alt_on = sum(1 << k for k in range(npts) if (npts - 1 - k) % 2 == 0)       # every other point, the end point among them
    return sorted({full, 0, alt_on, full ^ alt_on})


def lerp_is_nhwc(c):
    return c.layout == NHWC or c.hw == 1


def lerp_labels(c):
    out = {f"lerp_mix|{LAY[c.layout]}|points{c.n_points}"}
    if lerp_is_nhwc(c):
        out.add(f"lerp_mix_nhwc<{R.nhwc_keep(c.c)}>")
        if c.layout == NCHW:
            out.add("lerp_mix|hw1")
        if c.c > R.WAVE * R.KEEP_LARGE:
            out.add("lerp_mix_nhwc|reread")
        return out
    p = R.lerp_mix_plan(c.c, c.hw)
    out.add(f"lerp_mix<{'stage' if p['stage'] else 'reread'}>")
    if p["optin"] and not R.mix_plan(c.c, c.hw)["optin"]:
        out.add("lerp_mix|optin_fused_only")
    return out


@pytest.mark.parametrize("case", LERP_CASES, ids=lerp_id)
def test_lerp_mix_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    npts = c.n_points - 1
    rep = Report(f"lerp_mix {lerp_id(c)}")
    mc = MC(c.layout, F32, c.n, c.c, c.hw, "gauss")
    clean, adv = mix_rows(mc)
    ws = R.sample_weights(c.n_points)
    assert len(ws) == npts - 1
    mem = (lambda t: t) if c.layout == NHWC else (lambda t: t.permute(0, 2, 1))
    back = (lambda o: o.view(c.n, c.hw, c.c)) if c.layout == NHWC else (lambda o: o.view(c.n, c.c, c.hw).permute(0, 2, 1))
    cd, ad = to_dev(mem(clean).contiguous(), F32, gpu), to_dev(mem(adv).contiguous(), F32, gpu)
    total = c.n * c.hw * c.c
    # the points in float64 of their fp32 bits, and the separate launches
    cl32, ad32 = clean.float().numpy(), adv.float().numpy()
    pts = [torch.from_numpy(R.lerp_f32(cl32, ad32, w)) for w in ws] + [adv.float()]
    sep_pts = torch.full((max(npts - 1, 1) * total,), float("nan"), device=gpu)
    if npts > 1:
        rc = lib.afan_lerp_points(P(cd), P(ad), P(sep_pts), total, fptr(ws), npts - 1, _st())
        rep.expect(rc == 0, f"afan_lerp_points returned {rc}")
    sep = [sep_pts[k * total:(k + 1) * total] for k in range(npts - 1)] + [ad]
    for k in range(npts - 1):
        check_bits(rep, f"afan_lerp_points point {k + 1}", back(sep[k].cpu()), pts[k])
    sep_mix = []
    for k in range(npts):
        o = torch.full((total,), float("nan"), device=gpu)
        fn = lib.afan_mix_feature_nhwc if c.layout == NHWC else lib.afan_mix_feature
        rc = fn(P(cd), P(sep[k]), P(o), c.n, c.c, c.hw, EPS, 0, _st())
        rep.expect(rc == 0, f"afan_mix_feature on point {k + 1} returned {rc}")
        sep_mix.append(o.cpu())
    SENT = -12345.0
    for mask in lerp_masks(c.n_points):
        out = torch.full((npts * total,), SENT, device=gpu)
        rc = lib.afan_lerp_mix(P(cd), P(ad), P(out), c.n, c.c, c.hw, fptr(ws), c.n_points, mask, EPS, c.layout, _st())
        rep.expect(rc == 0, f"afan_lerp_mix mask {mask:#x} returned {rc}")
        if rc:
            continue
        o = out.cpu()
        for k in range(npts):
            got = o[k * total:(k + 1) * total]
            nm = f"mask {mask:#x} point {k + 1}"
            if (mask >> k) & 1:
                ref, s = R.mix_feature(clean.reshape(-1, c.c), pts[k].double().reshape(-1, c.c), EPS, mix_lanes(mc))
                check_window(rep, f"lerp_mix|{LAY[c.layout]}|mixed", nm + " mixed", back(got).reshape(-1, c.c), ref, mix_measured(mc) * U * s)
                rep.expect(bits_equal(got, sep_mix[k]), f"{nm}: the fused result differs in bits from afan_lerp_points + afan_mix_feature")
            elif k < npts - 1:
                check_bits(rep, nm + " unmasked", back(got), pts[k])
            else:
                rep.expect(bool((got == SENT).all()), f"{nm}: an end point without its mask bit was written")
    rep.done()


def test_lerp_mix_rejects_bad_arguments(pkg, gpu):
    lib = pkg._lib.load()
    x = torch.zeros(64, device=gpu)
    out = torch.full((5 * 64,), 7.0, device=gpu)
    for n_points, mask in ((1, 0), (R.LM_MAX + 2, 0), (3, 0b100)):
        assert lib.afan_lerp_mix(P(x), P(x), P(out), 1, 8, 8, fptr([0.25] * 4), n_points, mask, EPS, NCHW, _st()) == R.AFAN_ESHAPE
    assert bool((out == 7.0).all())


# ================================================================================================================= mix_w pair
MIXW_N = (1, 5, 4099, 262144 + 5)


@pytest.mark.parametrize("n", MIXW_N)
def test_mix_w_pinned(pkg, gpu, n):
    lib = pkg._lib.load()
    rep = Report(f"mix_w n={n}: {R.mix_w_dot_grid(n)} blocks")
    assert int(lib.afan_mix_w_workspace_floats()) == R.MIXW_MAX_BLOCKS
    gen = torch.Generator().manual_seed(n)
    wsd = torch.full((R.MIXW_MAX_BLOCKS,), float("nan"), device=gpu)
    for exact in (False, True):
        tag = "exact" if exact else "gauss"
        if exact:
            clean, adv, g = R.ints((n,), 8, gen), R.ints((n,), 8, gen), R.ternary((n,), gen)
        else:
            clean, adv, g = (torch.randn(n, generator=gen, dtype=torch.float64).float().double() for _ in range(3))
        cd, ad = to_dev(clean, F32, gpu), to_dev(adv, F32, gpu)
        if not exact:
            # forward: three fp32 roundings, bit for bit; bf16 is the RNE of that fp32 value
            w = 0.3137
            wd = torch.tensor([w], device=gpu)
            want = torch.from_numpy(R.mix_w_f32(clean.numpy(), adv.numpy(), w))
            for dt in (F32, BF16):
                out = torch.full((n,), float("nan"), dtype=dt, device=gpu)
                rc = lib.afan_mix_w(P(cd), P(ad), P(wd), P(out), DTC[dt], n, _st())
                rep.expect(rc == 0, f"afan_mix_w {DTN[dt]} returned {rc}")
                check_bits(rep, f"mix_w forward {DTN[dt]}", out.cpu(), want.to(dt))
        for gdt in (F32, BF16):
            g_s = stored(g, gdt)
            gd = to_dev(g_s, gdt, gpu)
            ref, s = R.mix_w_grad(g_s, clean, adv)
            for acc in (0, 1):
                start = 3.0 if exact else 0.8125
                dw = torch.tensor([start], device=gpu)
                rc = lib.afan_mix_w_backward(P(gd), DTC[gdt], P(cd), P(ad), n, P(wsd), P(dw), acc, _st())
                rep.expect(rc == 0, f"afan_mix_w_backward returned {rc}")
                want, ss = ref + acc * start, s + acc * abs(start)
                nm = f"dw {tag} grad {DTN[gdt]} accumulate={acc}"
                if exact:
                    assert ss < 2.0 ** 24
                    check_exact(rep, nm, dw.cpu(), torch.tensor([want], dtype=torch.float64))
                else:
                    check_window(rep, f"mix_w_dot|{DTN[gdt]}", nm, dw.cpu(), torch.tensor([want], dtype=torch.float64),
                                 torch.tensor([c_mix_w_dot(n, acc) * U * ss], dtype=torch.float64))
    rep.done()


def test_mix_w_backward_of_nothing(pkg, gpu):
    """n = 0: dw is set to 0 or left alone, per the flag (and the forward is a no-op)."""
    lib = pkg._lib.load()
    wsd = torch.full((R.MIXW_MAX_BLOCKS,), float("nan"), device=gpu)
    for acc, want in ((0, 0.0), (1, 2.5)):
        dw = torch.tensor([2.5], device=gpu)
        assert lib.afan_mix_w_backward(None, 0, None, None, 0, P(wsd), P(dw), acc, _st()) == 0
        assert float(dw.cpu()[0]) == want
    assert lib.afan_mix_w(None, None, None, None, 0, 0, _st()) == 0


# ====================================================================================================================== the head
HC = collections.namedtuple("HC", "dt n c hw k bias off")
HEAD_FWD_CASES = [
    HC(F32, 3, 300, 3, 7, True, 0), HC(F32, 1, 20, 16, 1, True, 0), HC(F32, 2, 64, 49, 16, False, 0),
    # the 16-byte-load kernel: C = 8 (256 pixel groups, HW below them), 64 (32 groups, HW no multiple), 512 (4 groups), 2048 (1 group)
    HC(BF16, 2, 8, 3, 7, True, 0), HC(BF16, 2, 64, 49, 16, True, 0), HC(BF16, 3, 512, 16, 7, True, 0), HC(BF16, 2, 512, 1, 7, False, 0),
    HC(BF16, 2, 512, 3, 1, True, 0), HC(BF16, 1, 2048, 3, 16, True, 0),
    # the scalar kernel by each reason it is chosen: 256 % (C / 8), C % 8, C / 8 > 256, a base pointer offset by one element
    HC(BF16, 2, 24, 16, 7, True, 0), HC(BF16, 2, 20, 49, 7, True, 0), HC(BF16, 2, 2056, 3, 7, True, 0), HC(BF16, 2, 64, 16, 7, True, 1),
    HC(BF16, 2, 300, 3, 16, True, 0),
]
HW_EXACT = {1: 1, 3: 4, 16: 16, 49: 64}       # the exact table's plane: 1 / HW and the mean are exact


def head_id(c):
    return f"{DTN[c.dt]}-n{c.n}-c{c.c}-hw{c.hw}-k{c.k}" + ("" if c.bias else "-nobias") + (f"-off{c.off}" if c.off else "")


def head_form(c):
    return R.head_fwd_form(c.dt == BF16, c.c, c.off == 0)


def head_labels(c):
    form = head_form(c)
    out = {f"head_fwd|k{c.k}", f"head_fwd|hw{c.hw}"}
    if c.dt == F32:
        out.add("head_fwd<f32>")
    elif form == "vec":
        g = R.head_vec_groups(c.c)
        out.add(f"head_fwd_vec|c{c.c}")
        if c.hw < g:
            out.add("head_fwd_vec|hw<g")
        elif c.hw % g:
            out.add("head_fwd_vec|hw%g")
    else:
        why = "unaligned" if c.off else "c%8" if c.c % 8 else "c/8>256" if c.c // 8 > R.BLOCK else "256%(c/8)"
        out.add(f"head_fwd<bf16>|{why}")
    if c.c > R.BLOCK and c.c % R.BLOCK:
        out.add("head_fwd|channel_loop_trip2_ragged")
    if not c.bias:
        out.add("head_fwd|nobias")
    if c.n == 1:
        out.add("head_fwd|n1")
    return out


@pytest.mark.parametrize("case", HEAD_FWD_CASES, ids=head_id)
def test_head_forward_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    form = head_form(c)
    rep = Report(f"head forward {head_id(c)} expected {form}")
    gen = torch.Generator().manual_seed(c.c + c.hw * 7 + c.k)
    for exact in (True, False):
        hw = HW_EXACT[c.hw] if exact else c.hw
        if exact:
            x, w, b = R.ints((c.n, hw, c.c), 4, gen), R.ternary((c.k, c.c), gen), R.ints((c.k,), 3, gen)
        else:
            x = stored(torch.randn((c.n, hw, c.c), generator=gen, dtype=torch.float64).relu() + 0.1, c.dt)
            w, b = (torch.randn(s, generator=gen, dtype=torch.float64).float().double() for s in ((c.k, c.c), (c.k,)))
        b = b if c.bias else None
        pooled, sp, logits, sl = R.head_forward(x, w, b)
        xd, wd, bd = to_dev(x, c.dt, gpu, c.off), to_dev(w, F32, gpu), (to_dev(b, F32, gpu) if c.bias else None)
        pd, ld = torch.full((c.n, c.c), float("nan"), device=gpu), torch.full((c.n, c.k), float("nan"), device=gpu)
        rc = lib.afan_head_forward(P(xd), DTC[c.dt], c.n, c.c, hw, P(wd), P(bd), c.k, P(pd), P(ld), _st())
        tag = "exact" if exact else "gauss"
        rep.expect(rc == 0, f"afan_head_forward {tag} returned {rc}")
        if rc:
            continue
        if exact:
            assert float(sl.max()) * hw < 2.0 ** 24 and float(sp.max()) * hw < 2.0 ** 24
            check_exact(rep, "pooled exact", pd.cpu(), pooled)
            check_exact(rep, "logits exact", ld.cpu(), logits)
        else:
            check_window(rep, f"head_pooled|{form}", "pooled", pd.cpu(), pooled, c_pool(form, c.c, hw) * U * sp)
            check_window(rep, f"head_logits|{form}", "logits", ld.cpu(), logits, c_logits(form, c.c, hw) * U * sl)
    rep.done()


def test_head_rejects_too_many_classes(pkg, gpu):
    """K = 17 returns AFAN_ESHAPE and writes nothing, forward and backward."""
    lib = pkg._lib.load()
    assert int(lib.afan_head_max_classes()) == R.MAXK
    k = R.MAXK + 1
    x, w, b = torch.ones((2, 4, 8), device=gpu), torch.ones((k, 8), device=gpu), torch.ones((k,), device=gpu)
    pd, ld = torch.full((2, 8), 7.0, device=gpu), torch.full((2, k), 7.0, device=gpu)
    assert lib.afan_head_forward(P(x), 0, 2, 8, 4, P(w), P(b), k, P(pd), P(ld), _st()) == R.AFAN_ESHAPE
    dx, dw, db = torch.full((2, 4, 8), 7.0, device=gpu), torch.full((k, 8), 7.0, device=gpu), torch.full((k,), 7.0, device=gpu)
    assert lib.afan_head_backward(P(ld), P(w), P(pd), 2, 8, 4, k, P(dx), 0, P(dw), P(db), 0, _st()) == R.AFAN_ESHAPE
    for t in (pd, ld, dx, dw, db):
        assert bool((t == 7.0).all())


HB = collections.namedtuple("HB", "b c hw k")
HEAD_BWD_CASES = [HB(1, 20, 3, 7), HB(5, 300, 16, 16), HB(17, 20, 1, 7), HB(40, 64, 49, 1)]


def head_bwd_gauss(c):
    """Gaussian dlogits, W, pooled and start values of a case.  With K = MAXK terms the window of a sum with cancellation,
    (K + 2) * 2^-24 * S, holds a bf16 rounding midpoint for 0.6 % of Gaussian results: more than half the 1 % cap, so the reference
    itself could not pass; that case takes non-negative dlogits and W (no cancellation: S = |dx|, the tightest window there is)."""
    gen = torch.Generator().manual_seed(c.b * 11 + c.c + c.k + 1)
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64).float().double()
    dl, w, pooled, start_w, start_b = rn(c.b, c.k), rn(c.k, c.c), rn(c.b, c.c), rn(c.k, c.c), rn(c.k)
    if c.k == R.MAXK:
        dl, w = dl.abs(), w.abs()
    return dl, w, pooled, start_w, start_b


def head_bwd_id(c):
    return f"b{c.b}-c{c.c}-hw{c.hw}-k{c.k}"


def head_bwd_labels(c):
    out = {f"head_bwd|b{c.b}"}
    if c.b < R.DW_SLICES:
        out.add("head_bwd|fewer_images_than_slices")
    elif c.b % R.DW_SLICES:
        out.add("head_bwd|uneven_slices")
    if (c.k * c.c) % R.DW_COLS and (c.k * c.c + c.k) % R.DW_COLS:
        out.add("head_bwd|dW_and_db_in_one_block")
    return out


@pytest.mark.parametrize("case", HEAD_BWD_CASES, ids=head_bwd_id)
def test_head_backward_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    rep = Report(f"head backward {head_bwd_id(c)}")
    gen = torch.Generator().manual_seed(c.b * 11 + c.c + c.k)
    for exact in (True, False):
        hw = HW_EXACT[c.hw] if exact else c.hw
        tag = "exact" if exact else "gauss"
        if exact:
            dl, w = R.ints((c.b, c.k), 3, gen), R.ternary((c.k, c.c), gen)
            pooled = R.ints((c.b, c.c), 4 * hw, gen) / hw
            start_w, start_b = R.ints((c.k, c.c), 5, gen), R.ints((c.k,), 5, gen)
        else:
            dl, w, pooled, start_w, start_b = head_bwd_gauss(c)
        dx, sdx, dw, sdw, db, sdb = R.head_backward(dl, w, pooled, hw)
        dld, wd, pd = to_dev(dl, F32, gpu), to_dev(w, F32, gpu), to_dev(pooled, F32, gpu)

        def hold(key, name, got, ref, s, cc):
            if exact:
                assert float(s.max()) * hw < 2.0 ** 24, f"{name}: sum |a * b| is not below 2^24"
                check_exact(rep, f"{name} exact", got, ref)
            else:
                check_window(rep, key, name, got, ref, cc * U * s)

        # dx in both types, alone (dweight = NULL)
        for dt in (F32, BF16):
            dxd = torch.full((c.b, hw, c.c), float("nan"), dtype=dt, device=gpu)
            rc = lib.afan_head_backward(P(dld), P(wd), P(pd), c.b, c.c, hw, c.k, P(dxd), DTC[dt], None, None, 0, _st())
            rep.expect(rc == 0, f"dx {tag} {DTN[dt]} returned {rc}")
            if rc == 0:
                e = lambda t: t[:, None, :].expand(c.b, hw, c.c)
                hold(f"head_dx|{DTN[dt]}", f"dx {DTN[dt]}", dxd.cpu(), e(dx), e(sdx), c_dx(c.k))
        # dW and db without dx; dW without db (db's buffer must stay as it is)
        for acc in (0, 1):
            for with_db in (True, False):
                dwd, dbd = to_dev(start_w, F32, gpu), to_dev(start_b, F32, gpu)
                rc = lib.afan_head_backward(P(dld), P(wd), P(pd), c.b, c.c, hw, c.k, None, 0, P(dwd), P(dbd) if with_db else None, acc, _st())
                nm = f"{tag} accumulate={acc}" + ("" if with_db else " dbias=NULL")
                rep.expect(rc == 0, f"dW {nm} returned {rc}")
                if rc:
                    continue
                aw, ab = acc * start_w.float().double(), acc * start_b.float().double()
                hold("head_dW", f"dW {nm}", dwd.cpu().view(c.k, c.c), dw + aw, sdw + aw.abs(), c_dw(c.b, acc))
                if with_db:
                    hold("head_db", f"db {nm}", dbd.cpu(), db + ab, sdb + ab.abs(), c_dw(c.b, acc))
                else:
                    check_bits(rep, f"db untouched {nm}", dbd.cpu(), start_b.float())
    rep.done()


# ================================================================================================================ cross-entropy
CE_SHAPES = [(1, 1), (7, 3), (300, 10), (17, 63), (17, 64), (17, 65), (20, 1000), (1024, 64)]
CE_KINDS = ("gauss", "mag80", "mag1e4", "special")


def ce_labels(n, k):
    form = R.ce_form(n, k)
    out = {f"ce<{form}>|{n}x{k}"}
    if form == "row" and n > R.CE_BLOCK:
        out.add("ce<row>|row_loop_trip2")
    if form == "wide" and n > R.CEW_WAVES:
        out.add("ce<wide>|row_loop_trip2")
    if form == "wide" and k % R.WAVE:
        out.add("ce<wide>|ragged_classes")
    if n * k == R.CE_MAX_ELEMS:
        out.add("ce|on_the_limit")
    return out


def run_ce(lib, dev, l, t):
    n, k = l.shape
    ld, td = to_dev(l, F32, dev), t.to(dev)
    loss, d = torch.full((1,), float("nan"), device=dev), torch.full((n, k), 7.0, device=dev)
    rc = lib.afan_cross_entropy(P(ld), P(td), n, k, P(loss), P(d), _st())
    return rc, loss.cpu(), d.cpu()


@pytest.mark.parametrize("shape", CE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_entropy_pinned(pkg, gpu, shape):
    n, k = shape
    lib = pkg._lib.load()
    form = R.ce_form(n, k)
    rep = Report(f"cross-entropy {n}x{k} expected ce<{form}>")
    gen = torch.Generator().manual_seed(n * 1000 + k)
    for kind in CE_KINDS:
        l = (torch.randn((n, k), generator=gen, dtype=torch.float64) * 3).float().double()
        t = torch.randint(0, k, (n,), generator=gen)
        if kind == "mag80":
            l = (l * (80 / 9)).clamp(-80, 80).float().double()
            l[0, 0] = 80.0
            l[0, k - 1] = -80.0 if k > 1 else 80.0
        elif kind == "mag1e4":
            l = (l * (1e4 / 9)).float().double()
        elif kind == "special":
            l[0] = 1.25                                                   # a row of equal logits
            if k > 1:
                r = n - 1
                l[r, (int(t[r]) + 1) % k] = float("-inf")                 # -inf in a non-target class: probability 0, gradient 0
        ref = R.cross_entropy(l, t)
        rc, loss, d = run_ce(lib, gpu, l, t)
        rep.expect(rc == 0, f"afan_cross_entropy {kind} returned {rc}")
        if rc:
            continue
        check_window(rep, f"ce_loss<{form}>|{kind}", f"loss {kind}", loss, torch.tensor([ref["loss"]], dtype=torch.float64),
                     torch.tensor([CE_LOSS_MEASURED * U * ref["s_loss"]], dtype=torch.float64))
        check_window(rep, f"ce_grad<{form}>|{kind}", f"dlogits {kind}", d, ref["d"], CE_GRAD_MEASURED * U * ref["s_d"] + R.F32_MIN_NORMAL)
        if kind == "special" and k > 1:
            rep.expect(float(d[n - 1, (int(t[n - 1]) + 1) % k]) == 0.0, "the gradient of a -inf class is not 0")
    rep.done()


@pytest.mark.parametrize("shape", [(7, 3), (17, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_entropy_bad_target_poisons_its_row_only(pkg, gpu, shape):
    n, k = shape
    lib = pkg._lib.load()
    form = R.ce_form(n, k)
    rep = Report(f"cross-entropy bad target {n}x{k} ce<{form}>")
    gen = torch.Generator().manual_seed(n + k)
    l = (torch.randn((n, k), generator=gen, dtype=torch.float64) * 3).float().double()
    for badv in (k, -1):
        t = torch.randint(0, k, (n,), generator=gen)
        t[3] = badv
        ref = R.cross_entropy(l, t)
        rc, loss, d = run_ce(lib, gpu, l, t)
        rep.expect(rc == 0, f"returned {rc}")
        rep.expect(math.isnan(ref["loss"]) and bool(torch.isnan(loss).all()), "the loss is not NaN")
        rep.expect(bool(torch.isnan(d[3]).all()), "the bad row of dlogits is not all NaN")
        keep = torch.arange(n) != 3
        check_window(rep, f"ce_grad<{form}>|bad_target", "other rows", d[keep], ref["d"][keep], CE_GRAD_MEASURED * U * ref["s_d"][keep] + R.F32_MIN_NORMAL)
    rep.done()


@pytest.mark.parametrize("shape", [(17, 63), (17, 64), (17, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_entropy_summation_order_names_the_kernel(pkg, gpu, shape):
    """Both kernels are right at K = 63 .. 65, so values alone cannot tell which one the `k >= 64` dispatch launched.  Rows whose loss
    is exact in fp32 can: class 0 at 0, the target class at -A with expf(-A) = 0, every other class at -inf, so that lse = 0 and the
    row's loss is A bit for bit; A = 2^31 in row 0 and 160 elsewhere (160 is above half the fp32 spacing of 256 at 2^31).  The mean
    must carry the bits of the expected kernel's summation order, which differ from the other kernel's."""
    n, k = shape
    lib = pkg._lib.load()
    form = R.ce_form(n, k)
    a = np.full(n, 160.0, np.float32)
    a[0] = 2.0 ** 31
    l = torch.full((n, k), float("-inf"), dtype=torch.float64)
    l[:, 0] = 0.0
    t = torch.arange(n) % (k - 1) + 1
    l[torch.arange(n), t] = -torch.from_numpy(a).double()
    want, other = R.ce_loss_in_kernel_order(form, a), R.ce_loss_in_kernel_order("row" if form == "wide" else "wide", a)
    assert want != other, "the operands do not tell the two summation orders apart"
    rc, loss, d = run_ce(lib, gpu, l, t)
    assert rc == 0
    print(f"TAILPIN ce_order<{form}> {float(loss[0])!r} expected {float(want)!r}, the other kernel's order gives {float(other)!r}")
    assert float(loss[0]) == float(want), f"ce<{form}> expected: got {float(loss[0])!r}, its order gives {float(want)!r}, the other kernel's {float(other)!r}"
    ref = R.cross_entropy(l, t)
    assert torch.equal(d.double(), (ref["d"] * n).round() * float(np.float32(1) / np.float32(n))), "dlogits: (1 or 0 or -1) * (1 / N) exactly"


def test_cross_entropy_rejects_more_than_one_block_of_work(pkg, gpu):
    lib = pkg._lib.load()
    n, k = R.CE_MAX_ELEMS + 1, 1
    assert R.ce_form(n, k) is None
    l, t = torch.zeros((n, k), device=gpu), torch.zeros((n,), dtype=torch.int64, device=gpu)
    loss, d = torch.full((1,), 7.0, device=gpu), torch.full((n, k), 7.0, device=gpu)
    assert lib.afan_cross_entropy(P(l), P(t), n, k, P(loss), P(d), _st()) == R.AFAN_ESHAPE
    assert float(loss.cpu()[0]) == 7.0 and bool((d == 7.0).all())


# ======================================================================================================================= norms
@pytest.mark.parametrize("shape", [(3, 7), (2, 4 * R.NORM_CHUNK + 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_perturb_norms_pinned(pkg, gpu, shape):
    b, per = shape
    lib = pkg._lib.load()
    rep = Report(f"perturb_norms {b}x{per}")
    gen = torch.Generator().manual_seed(per)
    xc = torch.randn((b, per), generator=gen)
    xa = xc + 0.03 * torch.randn((b, per), generator=gen)
    linf, l2, ss = R.perturb_norms(xa.numpy(), xc.numpy())
    nws = int(lib.afan_norms_workspace_floats(b, per))
    assert nws == 2 * b * -(-per // R.NORM_CHUNK)
    ws = torch.full((nws,), float("nan"), device=gpu)
    o2, oi = torch.full((b,), float("nan"), device=gpu), torch.full((b,), float("nan"), device=gpu)
    xad, xcd = xa.to(gpu), xc.to(gpu)
    rc = lib.afan_perturb_norms(P(xad), P(xcd), b, per, P(ws), P(o2), P(oi), _st())
    rep.expect(rc == 0, f"returned {rc}")
    if rc == 0:
        check_bits(rep, "linf", oi.cpu(), torch.from_numpy(linf))
        l2t, sst = torch.from_numpy(l2), torch.from_numpy(ss)
        check_window(rep, "norms_l2", "l2", o2.cpu(), l2t, U * (c_norm_ss(per) * sst / (2 * l2t) + l2t))
    rep.done()


# ==================================================================================================================== coverage
_D = ("f32", "bf16")
EXPECTED_VARIANTS = sorted(
    [f"mix<{d},{s}>" for d in _D for s in ("stage", "reread")] +
    [f"mix|{d}|{v}" for d in _D for v in ("pix64", "pix32", "pix16", "pix8", "tiny", "optin", "ragged_tile", "n>1", "empty_groups", "c%g",
                                           "hw1|keep8", "hw1|keep20", "nchw|rows", "nhwc|rows")] +
    [f"mix_nhwc<{d},{k}>" for d in _D for k in (8, 20)] + [f"mix_nhwc<{d},{k}>|full" for d in _D for k in (8, 20)] +
    [f"mix_nhwc|{d}|{v}" for d in _D for v in ("empty_lanes", "reread", "grid_trip2")] +
    ["mix|f32|nchw|c1", "mix|f32|nhwc|c1"] +
    [f"lerp_mix|{lay}|points{p}" for lay in ("nchw", "nhwc") for p in (2, 3, 4, 5)] +
    ["lerp_mix<stage>", "lerp_mix<reread>", "lerp_mix|optin_fused_only", "lerp_mix|hw1", "lerp_mix_nhwc<8>", "lerp_mix_nhwc<20>",
     "lerp_mix_nhwc|reread"] +
    [f"mix_w|n{n}" for n in MIXW_N] + ["mix_w|grid_trip2"] +
    ["head_fwd<f32>"] + [f"head_fwd_vec|c{c}" for c in (8, 64, 512, 2048)] + ["head_fwd_vec|hw<g", "head_fwd_vec|hw%g"] +
    [f"head_fwd<bf16>|{w}" for w in ("256%(c/8)", "c%8", "c/8>256", "unaligned")] +
    [f"head_fwd|hw{h}" for h in (1, 3, 16, 49)] + [f"head_fwd|k{k}" for k in (1, 7, 16)] +
    ["head_fwd|channel_loop_trip2_ragged", "head_fwd|nobias", "head_fwd|n1"] +
    [f"head_bwd|b{b}" for b in (1, 5, 17, 40)] + ["head_bwd|fewer_images_than_slices", "head_bwd|uneven_slices", "head_bwd|dW_and_db_in_one_block"] +
    ["ce<row>|1x1", "ce<row>|7x3", "ce<row>|300x10", "ce<row>|17x63", "ce<wide>|17x64", "ce<wide>|17x65", "ce<wide>|20x1000", "ce<wide>|1024x64",
     "ce<row>|row_loop_trip2", "ce<wide>|row_loop_trip2", "ce<wide>|ragged_classes", "ce|on_the_limit"])


def mix_w_labels(n):
    out = {f"mix_w|n{n}"}
    if n > R.MIXW_MAX_BLOCKS * R.BLOCK:
        out.add("mix_w|grid_trip2")
    return out


def table_variants():
    got = set()
    for c in MIX_CASES:
        got |= mix_labels(c)
    for c in LERP_CASES:
        got |= lerp_labels(c)
    for n in MIXW_N:
        got |= mix_w_labels(n)
    for c in HEAD_FWD_CASES:
        got |= head_labels(c)
    for c in HEAD_BWD_CASES:
        got |= head_bwd_labels(c)
    for n, k in CE_SHAPES:
        got |= ce_labels(n, k)
    return got
