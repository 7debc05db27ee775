"""The FUSED forms of the tiled bf16 convolution pinned ELEMENTWISE to float64, instantiation by instantiation: the in-launch
BatchNorm (ops.conv_fwd_bn / conv_fwd_multi_bn / conv_dgrad_bn, every `bf1` form dispatch_bnf picks), the frozen-BatchNorm epilogues
(conv_fwd_affine, conv_dgrad_affine, conv_dgrad_dual, conv_dgrad(sc=)), the grouped input gradient (`gs1`) and conv_wgrad_multi: the
24 instantiations tests/test_conv_pinned_gpu.py's FUSED_ALLOWLIST names.  References, tables and the restated dispatch:
tests/conv_fused_pinned_refs.py (checked on the CPU by tests/test_conv_fused_pinned_ref.py).

Two tables per form, the conv and BatchNorm pins' convention:
  * exact: ternary x / w / dy, integer shifts, residuals, addends and BatchNorm inputs, so that the raw tile is a small integer
    (asserted: |raw| <= 256, sum |a*b| < 2^24) and every sum is exact in any order.  Forward: raw bit for bit; mean = fl(shift + sum / M)
    (bit for bit where M is a power of two, else within N_MEAN_ACC roundings); invstd within N_INVSTD_ACC roundings; alpha = fl(invstd *
    w), beta = fma(-mean, alpha, b) of the PUBLISHED mean | invstd; every y_act element rounds from the float64 value of the published
    coefficients (no exempt fraction; a NaN in the residual poisons its element only); running buffers and num_batches_tracked for 1
    and 2 updates.  Backward: the test writes the statistics block itself, dyadic (integer mean, powers of two); the ReLU mask and
    dres, dbias and dweight (written over garbage, then accumulated onto integers) bit for bit; dx the RNE bf16 of the float64
    alpha * g + (x - mean) * k0 + k1 where every term is an fp32 value (M a power of two), else within N_DX_ACC roundings.
  * Gaussian: bf16 Gaussian operands.  Raw tiles / masked gradients through _check_bf16 (C_BF16); statistics, dx, dweight, dbias within
    C * 2^-24 * S with the BatchNorm pins' constants of the accumulator path (C_STAT_*["acc_f64sum"], C_DX / C_DW / C_DB["f64sum"]),
    wgrad_multi within C_WGRAD.  Every test prints its figures ("BNPIN <key> <ratio> <case>", run with -s) before it asserts.

Each in-launch form is launched twice in a row (the barrier resets itself) and ops.grid_barrier_error is read after each case.  The
shapes are the smallest dispatch_bnf sends to each instantiation (asserted per case with ops.conv_trace), nowhere near the residency
cap.  test_tables_reach_exactly_the_fused_instantiations keeps the allowlist honest: the kernels traced over these tables are the
allowlist's keys plus pinned plain forms (EXPECTED_VARIANTS of test_conv_pinned_gpu.py) under the frozen epilogues.

Worst ratios over these tables on an MI355X, units of 2^-24 * S (bound): mean 2.74 (8.22: re-measured, see SCH_MEAN), invstd 2.86
(5.79), dx 160.3 (1514.6; masked elements of a wide layer, as in the BatchNorm pins), d_sc 9.5 (1514.6), dweight 0.59 (3.63), dbias
0.23 (3.81), the two-problem forward's projection sums 1.35 / 1.03 (C_MOMENTS = 16), grouped sums 0.008 / 0.12 (3.81 / 3.63), wgrad_multi 1.27 (8).
The two-launch path on the same inputs gives the same statistics figures (mean 2.74, invstd 2.86).
"""
import types

import pytest
import torch

import conv_fused_pinned_refs as R
from conv_fused_pinned_refs import (C_BF16, C_DB, C_DW, C_DX, C_STAT_INVSTD, C_STAT_MEAN, C_WGRAD, FWD_COMBOS, N_DX_ACC, N_INVSTD_ACC, N_MEAN_ACC,
                                    N_RUNNING, N_UNBIAS, Report, U, _check_bf16, _check_exact, _cv, _density, _key, _ref_dgrad, _ref_fwd,
                                    _ref_wgrad, _ternary, check_window, ref_bn_backward, ref_moments, ref_running, ref_unbias)
from test_bn_pinned_gpu import ratio_of
from test_conv_pinned_gpu import C_MOMENTS, _cl, _gauss, _seed

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SCH, SUM = "acc_f64sum", "f64sum"
# The mean of sums a CONVOLUTION epilogue took (fp32 within a row tile, around a non-integer shift; f64 across tiles) exceeds
# C_STAT_MEAN["acc_f64sum"] (measured on fp32 tensors summed in f64 throughout) in the fused AND in the two-launch form alike
# (2.74 / 2.74 units on fwd_bn t64h_cols_8x8): re-measured over this table, STAT_MEAN_MEASURED["conv_acc_f64sum"]
# beside the old figure in tests/test_bn_pinned_gpu.py.  Every other quantity stays inside the BatchNorm pins' own bounds.
SCH_MEAN = "conv_acc_f64sum"


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def _kernels(t):
    return sorted({r["kernel"] for r in t.records})


def _ints(shape, lo, hi, g, dev):
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev).to(BF16)


def _bn(dev, w, b, rm, rv, eps):
    return types.SimpleNamespace(weight=w.float().to(dev), bias=b.float().to(dev), running_mean=rm.float().to(dev).clone(),
                                 running_var=rv.float().to(dev).clone(), num_batches_tracked=torch.zeros((), dtype=torch.int64, device=dev),
                                 eps=eps)


def _bn_params(c, g, dev, exact):
    """weight (a zero and a negative entry), bias, running mean (nonzero: the shift; integers in the exact table), running variance."""
    w = torch.rand(c, generator=g, device=dev) + 0.5
    w[0], w[1] = 0.0, -1.25
    b = torch.randn(c, generator=g, device=dev)
    rm = torch.randint(-3, 4, (c,), generator=g, device=dev).float() if exact else torch.randn(c, generator=g, device=dev) * 0.3
    rm[2] = 2.0 if exact else 0.4
    rv = torch.rand(c, generator=g, device=dev) + 0.5
    return w.double(), b.float().double(), rm.double(), rv.float().double()


def _beta_ok(beta_p, mean_p, alpha_p, b):
    v, tie = R.fma32(-mean_p, alpha_p, b)
    return (beta_p == v) | (tie & ((beta_p - v).abs() <= R.ulp32(v)))


# ---------------------------------------------------------------------------------------------------------------- forward checks
def _check_stats(rep, name, st, tile, shift, w, b, eps, exact, m):
    """The published mean | invstd | alpha | beta [4, C] (float64 view) against the float64 moments of the stored tile."""
    mean_r, var_r = ref_moments(tile)
    is_r = 1.0 / torch.sqrt(var_r + eps)
    mean_p, is_p, alpha_p, beta_p = st[0], st[1], st[2], st[3]
    xmax = max(float(tile.abs().max()), 1e-30)
    if exact:
        if _pow2(m):
            bad = mean_p != mean_r.float().double()
            if bool(bad.any()):
                c = int(bad.nonzero()[0])
                rep.expect(False, f"{name}: mean is not fl(shift + sum / M) of the exact sum in {int(bad.sum())} channels; first channel {c}: "
                                  f"got {float(mean_p[c])!r}, exact {float(mean_r[c])!r} (shift {float(shift[c])!r})")
        em = float(((mean_p - mean_r).abs() / (U * xmax)).max())
        ei = float(((is_p - is_r).abs() / (U * is_r)).max())
        rep.expect(em <= N_MEAN_ACC, f"{name}: mean off float64 by {em:.2f} units of 2^-24 * max|x| > {N_MEAN_ACC}")
        rep.expect(ei <= N_INVSTD_ACC, f"{name}: invstd off float64 by {ei:.2f} units of 2^-24 > {N_INVSTD_ACC}")
        mean_tol, var_rel = N_MEAN_ACC * U * xmax, 2.0 * N_INVSTD_ACC * U
    else:
        scale = U * (mean_r.abs() + torch.sqrt(var_r))
        em = float(((mean_p - mean_r).abs() / scale.clamp_min(1e-300)).max())
        ei = float(((is_p - is_r).abs() / (U * is_r)).max())
        rep.figure(f"fused_stat_mean[{SCH_MEAN}]", em)
        rep.figure(f"fused_stat_invstd[{SCH}]", ei)
        rep.expect(em <= C_STAT_MEAN[SCH_MEAN], f"{name}: mean off float64 by {em:.2f} units of 2^-24 * (|mean| + std) > {C_STAT_MEAN[SCH_MEAN]:.2f}")
        rep.expect(ei <= C_STAT_INVSTD[SCH], f"{name}: invstd off float64 by {ei:.2f} units of 2^-24 > {C_STAT_INVSTD[SCH]:.2f}")
        mean_tol, var_rel = C_STAT_MEAN[SCH_MEAN] * scale, 2.0 * C_STAT_INVSTD[SCH] * U
    rep.expect(bool((alpha_p == (is_p * w).float().double()).all()), f"{name}: published alpha is not fl(invstd * w)")
    rep.expect(bool(_beta_ok(beta_p, mean_p, alpha_p, b).all()), f"{name}: published beta is not fma(-mean, alpha, b)")
    return mean_r, var_r, mean_tol, var_rel


def _check_running(rep, name, bn, rm0, rv0, mean_r, var_r, mean_tol, var_rel, mom, updates, m, eps):
    var_u = var_r * ref_unbias(m)
    mom = float(torch.tensor(mom, dtype=torch.float32))           # (the float the launch receives)
    rm_ref, rv_ref = ref_running(rm0, mean_r, mom, updates), ref_running(rv0, var_u, mom, updates)
    tol_rm = N_RUNNING * updates * U * (rm0.abs() + mean_r.abs()) + mean_tol
    tol_rv = (N_RUNNING * updates + N_UNBIAS) * U * (rv0.abs() + var_u) + var_rel * (var_u + eps * ref_unbias(m))
    erm, erv = (bn.running_mean.double() - rm_ref).abs(), (bn.running_var.double() - rv_ref).abs()
    rep.expect(bool((erm <= tol_rm).all()), f"{name}: running_mean off float64 ({updates} updates, momentum {mom}): worst {float(erm.max()):.3e}")
    rep.expect(bool((erv <= tol_rv).all()), f"{name}: running_var off float64 ({updates} updates, momentum {mom}): worst {float(erv.max()):.3e}")
    rep.expect(int(bn.num_batches_tracked) == updates, f"{name}: num_batches_tracked {int(bn.num_batches_tracked)} != {updates}")


def _check_act(rep, name, act, tile, st, res, sc, relu, nan_at=None):
    """Every element of y_act rounds from the float64 relu(raw * alpha + beta [+ res | + raw_sc * alpha2 + beta2]) of the PUBLISHED
    coefficients within 2^-23 of the terms' absolute sum (the fp32 roundings of the expression); sc = (raw_sc, stats_sc)."""
    val = tile * _cv(st[2]) + _cv(st[3])
    s = val.abs()
    if sc is not None:
        v2 = sc[0] * _cv(sc[1][2]) + _cv(sc[1][3])
        val, s = val + v2, s + v2.abs()
    elif res is not None:
        r = res.double()
        if nan_at is not None:
            r = r.clone()
            r[nan_at] = 0.0
        val, s = val + r, s + r.abs()
    tol = 2.0 * U * s
    lo, hi = val - tol, val + tol
    if relu:
        lo, hi = lo.clamp_min(0.0), hi.clamp_min(0.0)
    if nan_at is not None:
        rep.expect(bool(torch.isnan(act[nan_at].float())), f"{name}: the residual's NaN did not reach its element")
        act = act.clone()
        act[nan_at] = 0.0
        lo[nan_at], hi[nan_at] = -1.0, 1.0
    check_window(rep, name, act, lo, hi)


def _fwd_operands(case, exact, dev):
    g = torch.Generator(device=dev).manual_seed(_seed(tuple(case[:7]), 41 + exact))
    n, ci, co, h, k = case.n, case.ci, case.co, case.h, case.k
    if exact:
        p = _density(k * k * ci)
        x, w = _cl(_ternary((n, ci, h, h), p, g, dev)), _cl(_ternary((co, ci, k, k), p, g, dev))
        res = _cl(_ints((n, co, h, h), -3, 3, g, dev))
        xs, wsc = _cl(_ternary((n, ci, 2 * h, 2 * h), _density(ci), g, dev)), _cl(_ternary((co, ci, 1, 1), _density(ci), g, dev))
    else:
        x, w = _cl(_gauss((n, ci, h, h), 1.0, g, dev)), _cl(_gauss((co, ci, k, k), (k * k * ci) ** -0.5, g, dev))
        res = _cl(_gauss((n, co, h, h), 1.0, g, dev))
        xs, wsc = _cl(_gauss((n, ci, 2 * h, 2 * h), 1.0, g, dev)), _cl(_gauss((co, ci, 1, 1), ci ** -0.5, g, dev))
    return g, x, w, res, xs, wsc


def _two_launch_stats(ops, dev, rep, x, w, d, form, relu, mom, res, xs, wsc, bn, bsc):
    """The two-launch path on the same inputs (conv_fwd with sums + bn_train_forward[_dual]): its statistics against float64 of ITS tile,
    printed beside the fused form's — a bound both exceed was measured on too narrow a table, one only the fused form exceeds is a bug."""
    ops.acc_reset(dev)
    raw, sta = ops.conv_fwd(x, w, 1, stats_shift=bn.running_mean, want_stats=True, dilation=d)
    tiles = [(raw, bn.eps)]
    if form == "projection":
        rsc, stc = ops.conv_fwd(xs, wsc, 2, stats_shift=bsc.running_mean, want_stats=True)
        _, st, ssc = ops.bn_train_forward_dual(raw, bn, sta, mom, rsc, bsc, stc, 0.1)
        tiles.append((rsc, bsc.eps))
        sts = [st, ssc]
    else:
        _, st = ops.bn_train_forward(raw, bn.weight, bn.bias, res if form == "residual" else None, relu, bn.eps, mom, bn.running_mean,
                                     bn.running_var, bn.num_batches_tracked, sta)
        sts = [st]
    for (tile, eps), st in zip(tiles, sts):
        mean_r, var_r = ref_moments(tile.double())
        em = float(((st[0].double() - mean_r).abs() / (U * (mean_r.abs() + torch.sqrt(var_r))).clamp_min(1e-300)).max())
        ei = float(((st[1].double() - 1.0 / torch.sqrt(var_r + eps)).abs() * torch.sqrt(var_r + eps) / U).max())
        rep.figure(f"twolaunch_stat_mean[{SCH_MEAN}]", em)
        rep.figure(f"twolaunch_stat_invstd[{SCH}]", ei)


# (form, relu, momentum, running updates): ReLU on and off where ops allows it (the projection form has it on), momentum 1.0 twice
FORMS = [("plain", False, 1.0, 2), ("plain", True, 0.1, 1), ("residual", True, 0.1, 1), ("residual", False, 0.3, 2), ("projection", True, 0.3, 2)]


def _launch_fwd(ops, x, w, bn, mom, d, form, relu, res, xs, wsc, bsc, updates):
    """(trace, result, raw_sc): the projection's own convolution (a plain, pinned launch) stays outside the trace."""
    rsc = sc = None
    if form == "projection":
        rsc, stc = ops.conv_fwd(xs, wsc, 2, stats_shift=bsc.running_mean, want_stats=True)
        sc = (rsc, bsc, stc, 0.1)
    with ops.conv_trace() as t, ops.bn_running_updates(updates):
        r = ops.conv_fwd_bn(x, w, bn, mom, residual=res if form == "residual" else None, relu=relu, sc=sc, dilation=d)
    return t, r, rsc


@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: c.tag)
def test_conv_fwd_bn_pinned(pkg, gpu, case):
    ops = pkg.ops
    n, ci, co, h, k, d = case.n, case.ci, case.co, case.h, case.k, case.d
    m, eps = n * h * h, 1e-5
    want = R.kernel_name("fwd", case.form)
    rep = Report(f"fwd_bn {case.tag} on {want}")
    for exact in (True, False):
        g, x, w, res, xs, wsc = _fwd_operands(case, exact, gpu)
        ref, S = _ref_fwd(x, w, 1, d), _ref_fwd(x.abs(), w.abs(), 1, d)
        tab = "exact" if exact else "Gaussian"
        if exact:
            assert float(ref.abs().max()) <= 256 and float(S.max()) < 2.0 ** 24, f"{case.tag}: the exact operands are not exact"
        for form, relu, mom, updates in FORMS:
            what = f"{form}{' + relu' if relu else ''} {tab}"
            w1, b1, rm1, rv1 = _bn_params(co, g, gpu, exact)
            w2, b2, rm2, rv2 = _bn_params(co, g, gpu, exact)
            nan_at = None
            r_in = res
            if form == "residual" and relu and exact:
                nan_at = (n - 1, 5, h - 1, 2)
                r_in = res.clone()
                r_in[nan_at] = float("nan")
            outs = []
            for launch in range(2):
                ops.acc_reset(gpu)
                bn, bsc = _bn(gpu, w1, b1, rm1, rv1, eps), _bn(gpu, w2, b2, rm2, rv2, 1e-3)
                t, r, rsc = _launch_fwd(ops, x, w, bn, mom, d, form, relu, r_in, xs, wsc, bsc, updates)
                assert r is not None, f"{case.tag} {what}: the in-launch form declined the launch"
                assert _kernels(t) == [want], f"{case.tag} {what}: ran on {_kernels(t)}, the table expects {want}"
                outs.append([v.clone() for v in r])
            torch.cuda.synchronize()
            assert not ops.grid_barrier_error(gpu), f"{case.tag} {what}: a grid barrier gave up"
            if exact:
                rep.expect(all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))
                               for a, b in zip(*outs) if not torch.isnan(a.float()).any()),
                           f"{what}: the second launch in a row differs from the first")
            raw, act, st = outs[1][0], outs[1][1], outs[1][2].double()
            on = f"{what} on {want}"
            if exact:
                _check_exact(raw, ref, f"fwd_bn {case.tag} raw {on}")
            else:
                _check_bf16(raw, ref, S, f"fwd_bn {case.tag} raw {on}")
            tile = raw.double()
            mr, vr, mt, vrel = _check_stats(rep, f"{what} stats", st, tile, rm1, w1, b1, eps, exact, m)
            _check_running(rep, what, bn, rm1, rv1, mr, vr, mt, vrel, mom, updates, m, eps)
            sc = None
            if form == "projection":
                st2 = outs[1][3].double()
                if exact:
                    assert float(rsc.double().abs().max()) <= 256
                mr2, vr2, mt2, vrel2 = _check_stats(rep, f"{what} projection stats", st2, rsc.double(), rm2, w2, b2, 1e-3, exact, m)
                _check_running(rep, f"{what} projection", bsc, rm2, rv2, mr2, vr2, mt2, vrel2, 0.1, updates, m, 1e-3)
                sc = (rsc.double(), st2)
            _check_act(rep, f"{what} y_act", act, tile, st, r_in if form == "residual" else None, sc, relu, nan_at)
            if not exact:
                _two_launch_stats(ops, gpu, rep, x, w, d, form, relu, mom, res, xs, wsc, _bn(gpu, w1, b1, rm1, rv1, eps), _bn(gpu, w2, b2, rm2, rv2, 1e-3))
    rep.done()


@pytest.mark.parametrize("case", R.MULTI_FWD_CASES, ids=lambda c: c[0])
def test_conv_fwd_multi_bn_pinned(pkg, gpu, case):
    """A block's first 3x3 / 2 with its BatchNorm + ReLU in the launch, the 1x1 / 2 projection riding as problem 1: both raw tiles, problem
    0's BatchNorm, and the projection's accumulator sums against float64 sums of its raw tile."""
    ops = pkg.ops
    tag, n, ci, co, h, form = case
    rep = Report(f"fwd_multi_bn {tag}")
    ho, m, eps, mom = h // 2, n * (h // 2) ** 2, 1e-5, 0.1
    want = R.kernel_name("fwd", form)
    for exact in (True, False):
        g = torch.Generator(device=gpu).manual_seed(_seed(case[:5], 43 + exact))
        tab = "exact" if exact else "Gaussian"
        if exact:
            x = _cl(_ternary((n, ci, h, h), _density(9 * ci), g, gpu))
            w3, w1 = _cl(_ternary((co, ci, 3, 3), _density(9 * ci), g, gpu)), _cl(_ternary((co, ci, 1, 1), 0.5, g, gpu))
        else:
            x = _cl(_gauss((n, ci, h, h), 1.0, g, gpu))
            w3, w1 = _cl(_gauss((co, ci, 3, 3), (9 * ci) ** -0.5, g, gpu)), _cl(_gauss((co, ci, 1, 1), ci ** -0.5, g, gpu))
        refs = [(_ref_fwd(x, w_, 2, 1), _ref_fwd(x.abs(), w_.abs(), 2, 1)) for w_ in (w3, w1)]
        pw, pb, prm, prv = _bn_params(co, g, gpu, exact)
        _, _, srm, _ = _bn_params(co, g, gpu, exact)
        for launch in range(2):
            ops.acc_reset(gpu)
            bn = _bn(gpu, pw, pb, prm, prv, eps)
            shift_sc = srm.float()
            with ops.conv_trace() as t:
                r = ops.conv_fwd_multi_bn(x, [w3, w1], 2, [1, 1], [bn.running_mean, shift_sc], bn, mom)
            assert r is not None, f"{tag} {tab}: the in-launch form declined the launch"
            assert _kernels(t) == [want], f"{tag} {tab}: ran on {_kernels(t)}, the table expects {want}"
        torch.cuda.synchronize()
        assert not ops.grid_barrier_error(gpu)
        (raw0, raw1), (st0, st1), act, stats = r
        for i, (raw, (ref, S)) in enumerate(zip((raw0, raw1), refs)):
            if exact:
                assert float(ref.abs().max()) <= 256 and float(S.max()) < 2.0 ** 24
                _check_exact(raw, ref, f"fwd_multi_bn {tag} raw{i} exact on {want}")
            else:
                _check_bf16(raw, ref, S, f"fwd_multi_bn {tag} raw{i} Gaussian on {want}")
        st = stats.double()
        mr, vr, mt, vrel = _check_stats(rep, f"{tab} stats", st, raw0.double(), prm, pw, pb, eps, exact, m)
        _check_running(rep, tab, bn, prm, prv, mr, vr, mt, vrel, mom, 1, m, eps)
        _check_act(rep, f"{tab} y_act", act, raw0.double(), st, None, None, True)
        # the projection's sums: acc[slot][q][C] doubles, then its shift
        ns = R.acc_slots(co)
        a = st1.acc[:ns * 2 * co].view(ns, 2, co).sum(0)
        c_ = raw1.double() - _cv(shift_sc.double())
        m1, m2 = c_.sum((0, 2, 3)), (c_ * c_).sum((0, 2, 3))
        if exact:
            rep.expect(bool((a[0] == m1).all()) and bool((a[1] == m2).all()), f"{tab}: the projection's accumulator sums are not the float64 sums")
        else:
            e1 = float(((a[0] - m1).abs() / (U * c_.abs().sum((0, 2, 3)))).max())
            e2 = float(((a[1] - m2).abs() / (U * m2)).max())
            rep.figure("fused_multi_sum1", e1)
            rep.figure("fused_multi_sum2", e2)
            rep.expect(e1 <= C_MOMENTS and e2 <= C_MOMENTS, f"{tab}: the projection's sums off float64 by {e1:.2f} / {e2:.2f} units of 2^-24 * sum |.| > {C_MOMENTS}")
        sh = st1.acc[2 * ns * co:2 * ns * co + (co + 1) // 2].view(torch.float32)[:co]
        rep.expect(torch.equal(sh, shift_sc), f"{tab}: the projection's shift snapshot")
    rep.done()


# --------------------------------------------------------------------------------------------------------------- backward checks
def _dyadic_stats(c, g, dev):
    """mean | invstd | alpha | beta written by the test: integer means, powers of two (alpha with a zero and negative entries)."""
    mean = torch.randint(-1, 2, (c,), generator=g, device=dev).float()
    invstd = 2.0 ** torch.randint(-1, 2, (c,), generator=g, device=dev).float()
    alpha = 2.0 ** torch.randint(-2, 1, (c,), generator=g, device=dev).float() * (torch.randint(0, 2, (c,), generator=g, device=dev).float() * 2 - 1)
    alpha[0], alpha[1] = 0.0, -0.5
    beta = torch.randint(-2, 3, (c,), generator=g, device=dev).float()
    return torch.stack([mean, invstd, alpha, beta]).contiguous()


def _masked_window(rep, name, dres, gref, S, add, mask):
    """dres must be mask ? bf16(bf16(g') [+ addend]) : 0 for a g' within C_BF16 * 2^-24 * S of the float64 input gradient."""
    tol = C_BF16 * U * S

    def f(v):
        b = v.float().to(BF16)
        if add is not None:
            b = (b.float() + add.float()).to(BF16)
        return torch.where(mask, b, torch.zeros_like(b))

    lo, hi, gk = _key(f(gref - tol)), _key(f(gref + tol)), _key(dres)
    bad = (gk < torch.minimum(lo, hi)) | (gk > torch.maximum(lo, hi))
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {dres.numel()} elements are not the masked RNE bf16 of a value within {C_BF16} * 2^-24 * S of the float64 "
                          f"gradient; first at {i}: got {float(dres[i])}, float64 {float(gref[i])}")
    off = int((gk != _key(f(gref))).sum())
    rep.expect(off <= max(8, dres.numel() // 1000), f"{name}: {off} of {dres.numel()} elements off the RNE bf16 of the float64 gradient")


def _check_bn_bwd(rep, name, exact, m, gk, x, st, dx, dwb, start, which="dx"):
    """dx, dweight, dbias of the BatchNorm backward of the (already masked) gradient gk, from the statistics block st (float64)."""
    r = ref_bn_backward(gk, x, st[0], st[1], st[2], None)
    dw_ref, db_ref = r["dw"] + start[0], r["db"] + start[1]
    if exact:
        rep.expect(float(r["s_db"].max()) < 2.0 ** 24 and float((gk * (x - _cv(st[0]))).abs().sum((0, 2, 3)).max()) < 2.0 ** 24,
                   f"{name}: the exact operands' sums reach 2^24")
        rep.expect(bool((dwb[1].double() == db_ref).all()), f"{name}: dbias is not the integer sum"
                   f" (first channel {int((dwb[1].double() != db_ref).nonzero()[0]) if bool((dwb[1].double() != db_ref).any()) else -1})")
        rep.expect(R.is_f32(dw_ref) and bool((dwb[0].double() == dw_ref).all()), f"{name}: dweight is not invstd * the integer sum"
                   f" (first channel {int((dwb[0].double() != dw_ref).nonzero()[0]) if bool((dwb[0].double() != dw_ref).any()) else -1})")
        xm = x - _cv(st[0])
        inner = xm * _cv(-st[2] * st[1] * st[1] * r["sgx"] / m) + _cv(-st[2] * r["sg"] / m)
        if _pow2(m):
            # the dyadic statistics make every term of the fma chain an fp32 value: the bit-for-bit check below must be the one that runs
            rep.expect(R.is_f32(inner) and R.is_f32(r["dx"]), f"{name}: the exact table's {which} terms are not fp32 values: the check would only be a window")
        if _pow2(m) and R.is_f32(inner) and R.is_f32(r["dx"]):
            want = r["dx"].float().to(BF16)
            bad = _key(dx) != _key(want)
            # (+0 and -0 are one value: the fma chain's sign of an exact zero is not pinned)
            bad &= ~((dx.float() == 0) & (want.float() == 0))
            nb = int(bad.sum())
            if nb:
                i = tuple(bad.nonzero()[0].tolist())
                rep.expect(False, f"{name}: {nb} of {dx.numel()} elements of {which} are not the RNE bf16 of the float64 alpha * g + (x - mean) * k0 + k1; "
                                  f"first at {i}: got {float(dx[i])}, float64 {float(r['dx'][i])}")
        else:
            tol = N_DX_ACC * U * r["s_dx"]
            check_window(rep, f"{name} {which}", dx, r["dx"] - tol, r["dx"] + tol)
    else:
        edx = ratio_of(dx, r["dx"], U * r["s_dx"])
        edw = float(((dwb[0].double() - dw_ref).abs() / (U * (r["s_dw"] + start[0].abs())).clamp_min(1e-300)).max())
        edb = float(((dwb[1].double() - db_ref).abs() / (U * (r["s_db"] + start[1].abs())).clamp_min(1e-300)).max())
        for key, v, c in ((f"fused_{which}[{SUM}]", edx, C_DX[SUM]), (f"fused_dw[{SUM}]", edw, C_DW[SUM]), (f"fused_db[{SUM}]", edb, C_DB[SUM])):
            rep.figure(key, v)
            rep.expect(v <= c, f"{name}: {key} off float64 by {v:.2f} units of 2^-24 * S > {c:.2f}")


def _bwd_operands(case, exact, dev, pair=False):
    g = torch.Generator(device=dev).manual_seed(_seed(tuple(case[:5]), 47 + exact))
    n, ci, co, h, k = case.n, case.ci, case.co, case.h, case.k
    ho = h // 2 if pair else h
    if exact:
        p = _density(k * k * co)
        dy, w = _cl(_ternary((n, co, ho, ho), p, g, dev)), _cl(_ternary((co, ci, k, k), p, g, dev))
        add, res = _cl(_ternary((n, ci, h, h), 0.5, g, dev)), _cl(_ints((n, ci, h, h), -2, 2, g, dev))
        bn_x, sc_x = _cl(_ints((n, ci, h, h), -3, 3, g, dev)), _cl(_ints((n, ci, h, h), -3, 3, g, dev))
    else:
        dy, w = _cl(_gauss((n, co, ho, ho), 1.0, g, dev)), _cl(_gauss((co, ci, k, k), (k * k * co) ** -0.5, g, dev))
        add, res = _cl(_gauss((n, ci, h, h), 1.0, g, dev)), _cl(_gauss((n, ci, h, h), 1.0, g, dev))
        bn_x, sc_x = _cl(_gauss((n, ci, h, h), 1.0, g, dev) + 0.25), _cl(_gauss((n, ci, h, h), 1.5, g, dev))
    return g, dy, w, add, res, bn_x, sc_x


def _published_stats(ops, x, g, dev, res, relu):
    """Gaussian table: the statistics block (and stored output) a plain BatchNorm forward publishes (pinned by test_bn_pinned_gpu.py)."""
    c = x.shape[1]
    gamma, beta = torch.rand(c, generator=g, device=dev) + 0.5, torch.randn(c, generator=g, device=dev) * 0.3
    gamma[0], gamma[1] = 0.0, -1.25
    y, st = ops.bn_train_forward(x, gamma, beta, res, relu, 1e-5, 0.1, None, None, None)
    return y, st.contiguous()


def _block_output(x, st, res, exact):
    """Exact table: the stored block output relu(x * alpha + beta + res) (dyadic: exact in bf16), with a +0, a -0 and the smallest
    positive bf16 planted where the mask is decided by them."""
    y = (x.double() * _cv(st[2].double()) + _cv(st[3].double()) + res.double()).clamp_min(0.0)
    assert bool((y.float().to(BF16).double() == y).all())
    y = _cl(y.float().to(BF16))
    flat = y.view(torch.int16)
    flat[0, 3, 0, 0], flat[0, 4, 0, 1], flat[0, 5, 1, 0] = 0, -32768, 1          # +0, -0, 2^-133
    return y


BWD_FORMS = ["bn1", "block_output", "block_output_sc"]


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: c.tag)
def test_conv_dgrad_bn_pinned(pkg, gpu, case):
    ops = pkg.ops
    n, ci, co, h, k, d = case.n, case.ci, case.co, case.h, case.k, case.d
    m = n * h * h
    want = R.kernel_name("dgrad", case.form)
    rep = Report(f"dgrad_bn {case.tag} on {want}")
    sc_form = case.form[7] > 0          # the projection BatchNorm's backward: halo forms only (the per-tap forms' LDS has no room for its tile)
    assert (R.dispatch_bnf(n, h, h, co, ci, k, d, bsc=True) is not None) == sc_form
    for exact in (True, False):
        tab = "exact" if exact else "Gaussian"
        g, dy, w, add, res, bn_x, sc_x = _bwd_operands(case, exact, gpu)
        wt = _cl(w.permute(1, 0, 2, 3))
        gref, S = _ref_dgrad(dy, w, (n, ci, h, h), 1, d), _ref_dgrad(dy.abs(), w.abs(), (n, ci, h, h), 1, d)
        if exact:
            assert float((gref.abs() + 1).max()) <= 256 and float(S.max()) < 2.0 ** 24, f"{case.tag}: the exact operands are not exact"
        x64 = bn_x.double()
        for form in BWD_FORMS:
            what = f"{form} {tab}"
            block = form != "bn1"
            if exact:
                stats, st_sc = _dyadic_stats(ci, g, gpu), _dyadic_stats(ci, g, gpu)
                bn_y = _block_output(bn_x, stats, res, True) if block else None
            else:
                _, st_sc = _published_stats(ops, sc_x, g, gpu, None, False)
                bn_y, stats = _published_stats(ops, bn_x, g, gpu, res if block else None, True)
                bn_y = bn_y if block else None
            st = stats.double()
            start = (torch.randint(-8, 9, (2, ci), generator=g, device=gpu).float() if exact else torch.randn(2, ci, generator=g, device=gpu))
            dwb, dws = torch.full((2, ci), 777.0, device=gpu), torch.full((2, ci), 777.0, device=gpu)
            d_sc = torch.empty_like(bn_x) if form == "block_output_sc" else None
            outs = []
            for launch in range(2):                     # written over garbage, then accumulated onto `start`
                ops.acc_reset(gpu)
                if launch == 1:
                    outs.append((r[0].clone(), r[1].clone(), dwb.clone(), dws.clone(), None if d_sc is None else d_sc.clone()))
                    dwb.copy_(start)
                    dws.copy_(start)
                with ops.conv_trace() as t:
                    r = ops.conv_dgrad_bn(dy, wt, (h, h), bn_x, stats, True, bn_y=bn_y, addend=add if block else None, want_dres=True,
                                          dweight=dwb[0], dbias=dwb[1], accumulate=launch == 1, dilation=d,
                                          sc=(sc_x, st_sc, d_sc, dws[0], dws[1]) if d_sc is not None else None)
                if form == "block_output_sc" and not sc_form:
                    break
                assert r is not None, f"{case.tag} {what}: the in-launch form declined the launch"
                assert _kernels(t) == [want], f"{case.tag} {what}: ran on {_kernels(t)}, the table expects {want}"
            if form == "block_output_sc" and not sc_form:
                assert r is None and not t.records, f"{case.tag} {what}: a form without the projection backward took the launch"
                continue
            outs.append((r[0], r[1], dwb, dws, d_sc))
            torch.cuda.synchronize()
            assert not ops.grid_barrier_error(gpu), f"{case.tag} {what}: a grid barrier gave up"
            mask = (bn_y.double() > 0) if block else (x64 * _cv(st[2]) + _cv(st[3]) > 0)
            zero = torch.zeros(2, ci, dtype=torch.float64, device=gpu)
            for launch, (dx, dres, dwb_l, dws_l, dsc_l) in enumerate(outs):
                nm = f"{what} launch {launch} on {want}"
                base = start.double() if launch == 1 else zero
                if exact:
                    gfull = gref + (add.double() if block else 0.0)
                    _check_exact(dres, torch.where(mask, gfull, torch.zeros_like(gfull)), f"dgrad_bn {case.tag} dres (mask, masked gradient) {nm}")
                else:
                    _masked_window(rep, f"{nm} dres", dres, gref, S, add if block else None, mask)
                gk = dres.double()
                _check_bn_bwd(rep, nm, exact, m, gk, x64, st, dx, dwb_l, base)
                if dsc_l is not None:
                    _check_bn_bwd(rep, nm + " projection", exact, m, gk, sc_x.double(), st_sc.double(), dsc_l, dws_l, base, which="d_sc")
            if exact and form == "bn1":                 # without the second output: the same dx
                ops.acc_reset(gpu)
                r2 = ops.conv_dgrad_bn(dy, wt, (h, h), bn_x, stats, True, dilation=d)
                assert r2 is not None and r2[1] is None
                rep.expect(torch.equal(r2[0].view(torch.int16), outs[0][0].view(torch.int16)), f"{what}: dx differs without want_dres")
    rep.done()


@pytest.mark.parametrize("case", R.PAIR_BWD_CASES, ids=lambda c: c[0])
def test_conv_dgrad_bn_pair_pinned(pkg, gpu, case):
    """The stride-2 pair form (a block's first 3x3 / 2 and its 1x1 / 2 projection, four output-parity classes, one set of sums)."""
    ops = pkg.ops
    tag, n, ci, co, h, form = case
    rep = Report(f"dgrad_bn_pair {tag}")
    c = R.Case(tag, n, ci, co, h, 3, 1, form)
    want = R.kernel_name("dgrad", form)
    m = n * h * h
    for exact in (True, False):
        tab = "exact" if exact else "Gaussian"
        g, _, w3, _, res, bn_x, _ = _bwd_operands(c, exact, gpu, pair=True)
        ho = h // 2
        if exact:
            both = _cl(_ternary((2 * n, co, ho, ho), _density(10 * co), g, gpu))
            w1 = _ternary((co, ci, 1, 1), 0.5, g, gpu)
        else:
            both = _cl(_gauss((2 * n, co, ho, ho), 1.0, g, gpu))
            w1 = _gauss((co, ci, 1, 1), co ** -0.5, g, gpu)
        dy, dy_sc = both[:n], both[n:]
        wt10 = torch.cat([w3.permute(1, 2, 3, 0).reshape(ci, 9, co), w1.permute(1, 2, 3, 0).reshape(ci, 1, co)], dim=1).contiguous()
        shape = (n, ci, h, h)
        gref = _ref_dgrad(dy, w3, shape, 2, 1) + torch.nn.grad.conv2d_input(shape, w1.double(), dy_sc.double(), 2, 0)
        S = _ref_dgrad(dy.abs(), w3.abs(), shape, 2, 1) + torch.nn.grad.conv2d_input(shape, w1.double().abs(), dy_sc.double().abs(), 2, 0)
        if exact:
            assert float(gref.abs().max()) <= 256 and float(S.max()) < 2.0 ** 24
            stats = _dyadic_stats(ci, g, gpu)
            bn_y = _block_output(bn_x, stats, res, True)
        else:
            bn_y, stats = _published_stats(ops, bn_x, g, gpu, res, True)
        st = stats.double()
        start = torch.randint(-8, 9, (2, ci), generator=g, device=gpu).float() if exact else torch.randn(2, ci, generator=g, device=gpu)
        dwb = torch.full((2, ci), 777.0, device=gpu)
        outs = []
        for launch in range(2):
            ops.acc_reset(gpu)
            if launch == 1:
                outs.append((r[0].clone(), r[1].clone(), dwb.clone()))
                dwb.copy_(start)
            with ops.conv_trace() as t:
                r = ops.conv_dgrad_bn(dy, None, (h, h), bn_x, stats, True, bn_y=bn_y, want_dres=True, dweight=dwb[0], dbias=dwb[1],
                                      accumulate=launch == 1, pair=(dy_sc, wt10))
            assert r is not None, f"{tag} {tab}: the in-launch form declined the launch"
            assert _kernels(t) == [want], f"{tag} {tab}: ran on {_kernels(t)}, the table expects {want}"
        outs.append((r[0], r[1], dwb))
        torch.cuda.synchronize()
        assert not ops.grid_barrier_error(gpu)
        mask = bn_y.double() > 0
        for launch, (dx, dres, dwb_l) in enumerate(outs):
            nm = f"{tab} launch {launch} on {want}"
            if exact:
                _check_exact(dres, torch.where(mask, gref, torch.zeros_like(gref)), f"dgrad_bn_pair {tag} dres {nm}")
            else:
                _masked_window(rep, f"{nm} dres", dres, gref, S, None, mask)
            base = start.double() if launch == 1 else torch.zeros(2, ci, dtype=torch.float64, device=gpu)
            _check_bn_bwd(rep, nm, exact, m, dres.double(), bn_x.double(), st, dx, dwb_l, base)
    rep.done()


# ----------------------------------------------------------------------------------------------------------- frozen BatchNorm forms
def _rne(v):
    return v.float().to(BF16)


def _affine_window(rep, name, got, ref, S, fn):
    """got must be fn(r) for a bf16 tile value r = RNE(conv') with conv' within C_BF16 * 2^-24 * S of the float64 convolution; fn is
    monotone in r per element (an affine map with a ReLU or a mask), so the keys of fn at both ends bound got's."""
    tol = C_BF16 * U * S
    a, b, gk = _key(fn(_rne(ref - tol))), _key(fn(_rne(ref + tol))), _key(got)
    bad = (gk < torch.minimum(a, b)) | (gk > torch.maximum(a, b))
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements outside the window; first at {i}: got {float(got[i])}, float64 convolution {float(ref[i])}")
    off = int((gk != _key(fn(_rne(ref)))).sum())
    rep.expect(off <= max(8, got.numel() // 1000), f"{name}: {off} of {got.numel()} elements off the value of the RNE tile")


@pytest.mark.parametrize("case", R.FROZEN_CASES, ids=lambda c: c[0])
def test_frozen_batchnorm_epilogues_pinned(pkg, gpu, case):
    """conv_fwd_affine over FWD_COMBOS, conv_dgrad_affine, conv_dgrad_dual with and without addend.  The epilogues round the bf16 tile
    once more: y = bf16(fl32(expression of the bf16 tile)); in the exact table the expression is exact (dyadic coefficients) and the
    outputs are the RNE bf16 of float64 bit for bit."""
    ops = pkg.ops
    tag, n, ci, co, h, w_, k, s, d = case
    rep = Report(f"frozen {tag}")
    ho, wo = (h - 1) // s + 1, (w_ - 1) // s + 1
    kern = set()
    for exact in (True, False):
        tab = "exact" if exact else "Gaussian"
        g = torch.Generator(device=gpu).manual_seed(_seed(case, 53 + exact))
        if exact:
            x, w = _cl(_ternary((n, ci, h, w_), _density(k * k * ci), g, gpu)), _cl(_ternary((co, ci, k, k), _density(k * k * ci), g, gpu))
            dy, wb = _cl(_ternary((n, co, ho, wo), _density(k * k * co), g, gpu)), _cl(_ternary((co, ci, k, k), _density(k * k * co), g, gpu))
            res, add = _cl(_ints((n, co, ho, wo), -3, 3, g, gpu)), _cl(_ternary((n, ci, h, w_), 0.5, g, gpu))
            kf, kb = _dyadic_stats(co, g, gpu), _dyadic_stats(ci, g, gpu)
            act = _cl(_ints((n, ci, h, w_), -1, 2, g, gpu).clamp_min(0))
        else:
            x, w = _cl(_gauss((n, ci, h, w_), 1.0, g, gpu)), _cl(_gauss((co, ci, k, k), (k * k * ci) ** -0.5, g, gpu))
            dy, wb = _cl(_gauss((n, co, ho, wo), 1.0, g, gpu)), _cl(_gauss((co, ci, k, k), (k * k * co) ** -0.5, g, gpu))
            res, add = _cl(_gauss((n, co, ho, wo), 1.0, g, gpu)), _cl(_gauss((n, ci, h, w_), 1.0, g, gpu))
            mk = lambda c: ops.affine_coefs(torch.randn(c, generator=g, device=gpu), torch.rand(c, generator=g, device=gpu) + 0.5,
                                            torch.randn(c, generator=g, device=gpu), torch.randn(c, generator=g, device=gpu))
            kf, kb = mk(co), mk(ci)
            act = _cl(torch.relu(_gauss((n, ci, h, w_), 1.0, g, gpu)))
        act.view(torch.int16)[0, 3, 0, 0], act.view(torch.int16)[0, 4, 0, 1], act.view(torch.int16)[0, 5, 1, 0] = 0, -32768, 1
        al, be = kf[2].view(1, -1, 1, 1), kf[3].view(1, -1, 1, 1)
        ref, S = _ref_fwd(x, w, s, d), _ref_fwd(x.abs(), w.abs(), s, d)
        for res_on, relu in FWD_COMBOS:
            with ops.conv_trace() as t:
                y = ops.conv_fwd_affine(x, w, s, kf, res if res_on else None, relu, dilation=d)
            assert y is not None, f"{tag}: conv_fwd_affine declined a tiled shape"
            kern |= set(_kernels(t))
            nm = f"fwd_affine res{res_on} relu{relu} {tab} on {_kernels(t)}"
            if exact:
                assert float(ref.abs().max()) <= 256 and float(S.max()) < 2.0 ** 24
                v64 = ref * al.double() + be.double() + (res.double() if res_on else 0.0)
                assert R.is_f32(v64)
                want = _rne(v64.clamp_min(0.0) if relu else v64)
                ok = (_key(y) == _key(want)) | ((y.float() == 0) & (want.float() == 0))
                rep.expect(bool(ok.all()), f"{nm}: {int((~ok).sum())} elements are not the RNE bf16 of the float64 value"
                           + (f"; first at {tuple((~ok).nonzero()[0].tolist())}" if not bool(ok.all()) else ""))
            else:
                # fl32(fma(r, alpha, beta) [+ res]) -> bf16: the fp32 roundings move a value by 2^-23 relative at most, far inside a
                # bf16 ulp; hold y to the window of the RNE tile's float64 value +- those roundings
                lo_hi = []
                for r_ in (_rne(ref - C_BF16 * U * S), _rne(ref + C_BF16 * U * S)):
                    v = r_.double() * al.double() + be.double()
                    sc_ = v.abs() + (res.double().abs() if res_on else 0.0)
                    v = v + (res.double() if res_on else 0.0)
                    lo_hi += [v - 2.0 * U * sc_, v + 2.0 * U * sc_]
                lo, hi = torch.stack(lo_hi).min(0).values, torch.stack(lo_hi).max(0).values
                if relu:
                    lo, hi = lo.clamp_min(0.0), hi.clamp_min(0.0)
                check_window(rep, nm, y, lo, hi)
        # input gradients: dx = bf16((act > 0 ? bf16(dgrad) : 0) * alpha); dual: dres = act > 0 ? bf16(bf16(dgrad) + addend) : 0, d3 = bf16(dres * alpha)
        wt = _cl(wb.permute(1, 0, 2, 3))
        shape = (n, ci, h, w_)
        gref, gS = _ref_dgrad(dy, wb, shape, s, d), _ref_dgrad(dy.abs(), wb.abs(), shape, s, d)
        alb = kb[2].contiguous()
        mask = act.double() > 0
        mul = lambda r: (torch.where(mask, r.float(), torch.zeros_like(r.float())) * alb.view(1, -1, 1, 1)).to(BF16)
        with ops.conv_trace() as t:
            dx = ops.conv_dgrad_affine(dy, wt, (h, w_), s, alb, act, dilation=d)
        assert dx is not None, f"{tag}: conv_dgrad_affine declined a tiled shape"
        kern |= set(_kernels(t))
        nm = f"dgrad_affine {tab} on {_kernels(t)}"
        if exact:
            assert float((gref.abs() + 1).max()) <= 256 and float(gS.max()) < 2.0 ** 24
            want = mul(_rne(gref))
            ok = (_key(dx) == _key(want)) | ((dx.float() == 0) & (want.float() == 0))
            rep.expect(bool(ok.all()), f"{nm}: {int((~ok).sum())} elements are not bf16(masked gradient * alpha)")
        else:
            _affine_window(rep, nm, dx, gref, gS, mul)
        if d == 1:
            for with_add in (False, True):
                with ops.conv_trace() as t:
                    r = ops.conv_dgrad_dual(dy, wt, (h, w_), s, add if with_add else None, alb, act)
                assert r is not None, f"{tag}: conv_dgrad_dual declined a tiled shape"
                kern |= set(_kernels(t))
                d3, dres = r
                nm = f"dgrad_dual addend{int(with_add)} {tab} on {_kernels(t)}"
                if exact:
                    gfull = gref + (add.double() if with_add else 0.0)
                    _check_exact(dres, torch.where(mask, gfull, torch.zeros_like(gfull)), f"frozen {tag} {nm} dres")
                else:
                    _masked_window(rep, f"{nm} dres", dres, gref, gS, add if with_add else None, mask)
                want = (dres.float() * alb.view(1, -1, 1, 1)).to(BF16)         # both outputs: d3 is the rounded product of the stored dres
                ok = (_key(d3) == _key(want)) | ((d3.float() == 0) & (want.float() == 0))
                rep.expect(bool(ok.all()), f"{nm}: {int((~ok).sum())} elements of d3 are not bf16(dres * alpha)")
    assert kern <= R.EXPECTED_VARIANTS, f"{tag}: the frozen epilogues ran on instantiations no plain pin reaches: {sorted(kern - R.EXPECTED_VARIANTS)}"
    rep.done()


@pytest.mark.parametrize("shape", [(2, 64, 128, 14, 10), (3, 128, 256, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_conv_dgrad_with_fused_projection_pinned(pkg, gpu, shape):
    """conv_dgrad(..., sc=...): the 3x3 / 2 and the 1x1 / 2 projection's input gradients as one accumulation, rounded once."""
    ops = pkg.ops
    n, ci, co, h, w_ = shape
    ho, wo = h // 2, w_ // 2
    for exact in (True, False):
        g = torch.Generator(device=gpu).manual_seed(_seed(shape, 59 + exact))
        if exact:
            both, w3, w1 = _cl(_ternary((2 * n, co, ho, wo), _density(10 * co), g, gpu)), _ternary((co, ci, 3, 3), _density(10 * co), g, gpu), _ternary((co, ci, 1, 1), 0.5, g, gpu)
        else:
            both, w3, w1 = _cl(_gauss((2 * n, co, ho, wo), 1.0, g, gpu)), _gauss((co, ci, 3, 3), (9 * co) ** -0.5, g, gpu), _gauss((co, ci, 1, 1), co ** -0.5, g, gpu)
        dy, dy_sc = both[:n], both[n:]
        wt10 = torch.cat([w3.permute(1, 2, 3, 0).reshape(ci, 9, co), w1.permute(1, 2, 3, 0).reshape(ci, 1, co)], dim=1).contiguous()
        sh = (n, ci, h, w_)
        ref = _ref_dgrad(dy, w3, sh, 2, 1) + torch.nn.grad.conv2d_input(sh, w1.double(), dy_sc.double(), 2, 0)
        S = _ref_dgrad(dy.abs(), w3.abs(), sh, 2, 1) + torch.nn.grad.conv2d_input(sh, w1.double().abs(), dy_sc.double().abs(), 2, 0)
        with ops.conv_trace() as t:
            dx = ops.conv_dgrad(dy, _cl(w3.permute(1, 0, 2, 3)), (h, w_), 2, sc=(dy_sc, wt10))
        what = f"dgrad sc= {shape} {'exact' if exact else 'Gaussian'} on {_kernels(t)}"
        assert set(_kernels(t)) <= R.EXPECTED_VARIANTS, what
        if exact:
            assert float(ref.abs().max()) <= 256 and float(S.max()) < 2.0 ** 24
            _check_exact(dx, ref, what)
        else:
            _check_bf16(dx, ref, S, what)


# ------------------------------------------------------------------------------------------- grouped input gradient, wgrad_multi
@pytest.mark.parametrize("case", R.GROUPED_CASES, ids=lambda c: c.tag)
def test_grouped_dgrad_sums_pinned(pkg, gpu, case):
    """conv_dgrad(groups=2, bn_bwd=...) with a half-batch that is not a whole number of row tiles (the straddling tile walks twice): dx
    and each half's two sums (sum g, sum g (x - mean) of ITS statistics block, recomputed mask) against separate float64 sums."""
    ops = pkg.ops
    rep = Report(f"grouped {case.tag}")
    n, ci, co, h, k = case.n, case.ci, case.co, case.h, case.k
    want = R.kernel_name("dgrad", case.form, gs=1, bf=0)
    ns, hb = R.acc_slots(ci), n // 2
    for exact in (True, False):
        tab = "exact" if exact else "Gaussian"
        g, dy, w, _, _, bn_x, _ = _bwd_operands(case, exact, gpu)
        wt = _cl(w.permute(1, 0, 2, 3))
        if exact:
            st2 = torch.stack([_dyadic_stats(ci, g, gpu), _dyadic_stats(ci, g, gpu)])
        else:
            st2 = torch.stack([_published_stats(ops, bn_x[i * hb:(i + 1) * hb], g, gpu, None, True)[1] for i in range(2)])
        ops.acc_reset(gpu)
        with ops.conv_trace() as t:
            dx, part = ops.conv_dgrad(dy, wt, (h, h), 1, bn_bwd=(bn_x, st2, True), groups=2)
        assert _kernels(t) == [want], f"{case.tag} {tab}: ran on {_kernels(t)}, the table expects {want}"
        gref, S = _ref_dgrad(dy, w, (n, ci, h, h), 1, 1), _ref_dgrad(dy.abs(), w.abs(), (n, ci, h, h), 1, 1)
        if exact:
            assert float(gref.abs().max()) <= 256 and float(S.max()) < 2.0 ** 24
            _check_exact(dx, gref, f"grouped {case.tag} dx exact on {want}")
        else:
            _check_bf16(dx, gref, S, f"grouped {case.tag} dx Gaussian on {want}")
        for i in range(2):
            sl = slice(i * hb, (i + 1) * hb)
            st = st2[i].double()
            xh, gh = bn_x[sl].double(), dx[sl].double()
            gm = torch.where(xh * _cv(st[2]) + _cv(st[3]) > 0, gh, torch.zeros_like(gh))
            xm = xh - _cv(st[0])
            s1, s2 = gm.sum((0, 2, 3)), (gm * xm).sum((0, 2, 3))
            a = part.group(i, ci).acc[:ns * 2 * ci].view(ns, 2, ci).sum(0)
            if exact:
                assert float(gm.abs().sum((0, 2, 3)).max()) < 2.0 ** 24 and float((gm * xm).abs().sum((0, 2, 3)).max()) < 2.0 ** 24
                rep.expect(bool((a[0] == s1).all()), f"{tab}: half {i}: sum g is not the float64 sum over that half")
                rep.expect(bool((a[1] == s2).all()), f"{tab}: half {i}: sum g (x - mean) is not the float64 sum over that half")
            else:
                e1 = float(((a[0] - s1).abs() / (U * gm.abs().sum((0, 2, 3))).clamp_min(1e-300)).max())
                e2 = float(((a[1] - s2).abs() / (U * (gm * xm).abs().sum((0, 2, 3))).clamp_min(1e-300)).max())
                rep.figure(f"grouped_db[{SUM}]", e1)
                rep.figure(f"grouped_dw[{SUM}]", e2)
                rep.expect(e1 <= C_DB[SUM], f"{tab}: half {i}: sum g off float64 by {e1:.2f} units > {C_DB[SUM]:.2f}")
                rep.expect(e2 <= C_DW[SUM], f"{tab}: half {i}: sum g (x - mean) off float64 by {e2:.2f} units > {C_DW[SUM]:.2f}")
    rep.done()


@pytest.mark.parametrize("name", sorted(R.WGRAD_MULTI_CASES))
def test_conv_wgrad_multi_pinned(pkg, gpu, name):
    """Several layers' weight gradients in one launch, added into their gradient tensors (ops.conv_wgrad_multi always accumulates: the
    multi launch has no overwriting form through ops): bit for bit onto integers in the exact table, C_WGRAD in the Gaussian one."""
    ops = pkg.ops
    shapes = R.WGRAD_MULTI_CASES[name]
    for exact in (True, False):
        g = torch.Generator(device=gpu).manual_seed(_seed((name,), 61 + exact))
        items, refs = [], []
        for (n, ci, co, h, k, s, d) in shapes:
            if exact:
                p = _density(n * h * h, target=4096.0)
                x, dy = _cl(_ternary((n, ci, h, h), p, g, gpu)), _cl(_ternary((n, co, h, h), p, g, gpu))
                start = _cl(torch.randint(-64, 65, (co, ci, k, k), generator=g, device=gpu).float())
            else:
                x, dy = _cl(_gauss((n, ci, h, h), 1.0, g, gpu)), _cl(_gauss((n, co, h, h), 1.0, g, gpu))
                start = _cl(torch.randn((co, ci, k, k), generator=g, device=gpu))
            items.append((x, dy, k, s, d, start.clone()))
            refs.append((_ref_wgrad(x, dy, (co, ci, k, k), s, d), _ref_wgrad(x.abs(), dy.abs(), (co, ci, k, k), s, d), start.double()))
        codes = {ops.conv_wgrad_plan(x, dy, k, s) for (x, dy, k, s, _, _) in items}
        assert len(codes) == 1 and 0 not in codes, f"{name}: the layers do not share one plan: {codes}"
        with ops.conv_trace() as t:
            ops.conv_wgrad_multi(items)
        assert _kernels(t) == [name], f"{name}: ran on {_kernels(t)}"
        for i, (it, (ref, S, start)) in enumerate(zip(items, refs)):
            what = f"{name} layer {i} {shapes[i]} {'exact' if exact else 'Gaussian'}"
            if exact:
                assert float((S + 64).max()) < 2.0 ** 24
                _check_exact(it[5], ref + start, what)
            else:
                err = (it[5].double() - (ref + start)).abs()
                ratio = float(((err - 2.0 ** -23 * (ref.abs() + start.abs())).clamp_min(0.0) / (U * S + 1e-300)).max())
                print(f"BNPIN fused_wgrad_multi {ratio:.4f} {what}")
                assert ratio <= C_WGRAD, f"{what}: |g - g64| = {ratio:.2f} * 2^-24 * S > {C_WGRAD}"


# ------------------------------------------------------------------------------------------------------------------------ coverage
def _z(shape, dev, dt=BF16):
    return _cl(torch.zeros(shape, dtype=dt, device=dev)) if len(shape) == 4 else torch.zeros(shape, dtype=dt, device=dev)


def test_tables_reach_exactly_the_fused_instantiations(pkg, gpu):
    """Every launch form of the tables above on zero operands (the trace is what matters): the fused kernels traced are exactly
    FUSED_ALLOWLIST's keys; whatever else runs (the frozen epilogues' and the fused projection gradient's kernels) is a pinned plain form."""
    if R._tuned():
        pytest.skip(f"kernel tuning variables set ({R._tuned()}): dispatch is not the default one")
    ops = pkg.ops
    first = {}

    def note(t, row):
        for r in t.records:
            first.setdefault(r["kernel"], row)

    one = lambda c: torch.ones(c, device=gpu)
    for c in R.FWD_CASES:
        x, w = _z((c.n, c.ci, c.h, c.h), gpu), _z((c.co, c.ci, c.k, c.k), gpu)
        ops.acc_reset(gpu)
        with ops.conv_trace() as t:
            r = ops.conv_fwd_bn(x, w, _bn(gpu, one(c.co), one(c.co), one(c.co), one(c.co), 1e-5), 0.1, dilation=c.d)
        assert r is not None, c.tag
        note(t, "fwd " + c.tag)
    for c in R.BWD_CASES:
        dy, wt, bx = _z((c.n, c.co, c.h, c.h), gpu), _z((c.ci, c.co, c.k, c.k), gpu), _z((c.n, c.ci, c.h, c.h), gpu)
        ops.acc_reset(gpu)
        with ops.conv_trace() as t:
            r = ops.conv_dgrad_bn(dy, wt, (c.h, c.h), bx, torch.ones(4, c.ci, device=gpu), True, dilation=c.d)
        assert r is not None, c.tag
        note(t, "bwd " + c.tag)
    for tag, n, ci, co, h, _ in R.MULTI_FWD_CASES:
        ops.acc_reset(gpu)
        bn = _bn(gpu, one(co), one(co), one(co), one(co), 1e-5)
        with ops.conv_trace() as t:
            r = ops.conv_fwd_multi_bn(_z((n, ci, h, h), gpu), [_z((co, ci, 3, 3), gpu), _z((co, ci, 1, 1), gpu)], 2, [1, 1],
                                      [bn.running_mean, one(co)], bn, 0.1)
        assert r is not None, tag
        note(t, tag)
    for tag, n, ci, co, h, _ in R.PAIR_BWD_CASES:
        both = _z((2 * n, co, h // 2, h // 2), gpu)
        bx = _z((n, ci, h, h), gpu)
        ops.acc_reset(gpu)
        with ops.conv_trace() as t:
            r = ops.conv_dgrad_bn(both[:n], None, (h, h), bx, torch.ones(4, ci, device=gpu), True, bn_y=bx, pair=(both[n:], torch.zeros(ci * 10 * co, dtype=BF16, device=gpu)))
        assert r is not None, tag
        note(t, tag)
    for c in R.GROUPED_CASES:
        ops.acc_reset(gpu)
        with ops.conv_trace() as t:
            ops.conv_dgrad(_z((c.n, c.co, c.h, c.h), gpu), _z((c.ci, c.co, c.k, c.k), gpu), (c.h, c.h), 1,
                           bn_bwd=(_z((c.n, c.ci, c.h, c.h), gpu), torch.ones(2, 4, c.ci, device=gpu), True), groups=2)
        note(t, c.tag)
    for name, shapes in R.WGRAD_MULTI_CASES.items():
        items = [(_z((n, ci, h, h), gpu), _z((n, co, h, h), gpu), k, s, d, _cl(torch.zeros(co, ci, k, k, device=gpu))) for (n, ci, co, h, k, s, d) in shapes]
        with ops.conv_trace() as t:
            ops.conv_wgrad_multi(items)
        note(t, name)
    for tag, n, ci, co, h, w_, k, s, d in R.FROZEN_CASES:
        ho, wo = (h - 1) // s + 1, (w_ - 1) // s + 1
        x, w, dy, wt = _z((n, ci, h, w_), gpu), _z((co, ci, k, k), gpu), _z((n, co, ho, wo), gpu), _z((ci, co, k, k), gpu)
        with ops.conv_trace() as t:
            assert ops.conv_fwd_affine(x, w, s, torch.zeros(4, co, device=gpu), _z((n, co, ho, wo), gpu), True, dilation=d) is not None
            assert ops.conv_dgrad_affine(dy, wt, (h, w_), s, one(ci), x, dilation=d) is not None
            if d == 1:
                assert ops.conv_dgrad_dual(dy, wt, (h, w_), s, x, one(ci), x) is not None
        note(t, tag)
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)
    got, want = set(first), set(R.FUSED_ALLOWLIST)
    extra = got - want - R.EXPECTED_VARIANTS             # the frozen epilogues run on plain forms: pinned ones
    assert not extra and want <= got, (f"the tables reach {sorted(extra)} beyond FUSED_ALLOWLIST and the pinned plain forms (rows: "
                                       f"{[first[v] for v in sorted(extra)]}), miss {sorted(want - got)}")
    fused_rows = {first[v] for v in got - want}
    assert fused_rows <= {c[0] for c in R.FROZEN_CASES}, f"a fused table ran a plain form: {sorted(fused_rows)}"
