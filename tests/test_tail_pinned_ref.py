"""The float64 references of tests/tail_pinned_refs.py (what tests/test_tail_pinned_gpu.py holds the mixing, head and loss kernels to)
checked on the CPU: against torch in float64 (var / mean, F.linear + adaptive_avg_pool2d and F.cross_entropy with autograd), against
torch.lerp in fp32 and exact rationals for the lerp bits, against the project's fp32 C oracle for mix_feature and the lerp points; the
dispatch predicates restated from the sources with their constants; the coverage of the GPU tables; and the tables' own condition
that the references alone could pass the bf16 midpoint rule."""
import fractions
import re

import numpy as np
import pytest
import torch

import tail_pinned_refs as R
import test_tail_pinned_gpu as G
from conftest import ROOT, ptr

U = R.U
F = np.float32


def _src(name):
    with open(f"{ROOT}/cv_a-fan_amd/csrc/{name}") as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------------- mix_feature
@pytest.mark.parametrize("c,hw", [(2, 5), (19, 7), (512, 3)])
def test_mix_feature_reference_matches_torch_and_the_c_oracle(c_oracle, orc, c, hw):
    gen = torch.Generator().manual_seed(c)
    n = 2
    clean = (torch.randn((n, c, hw, 1), generator=gen) * 1.5 + 0.5)
    adv = (torch.randn((n, c, hw, 1), generator=gen) * 0.7 - 0.25)
    rows = lambda t: R.rows_of(t.double(), False)
    ref, s = R.mix_feature(rows(clean), rows(adv), 1e-5, 64)
    want = rows(orc.mix_feature(clean.double(), adv.double(), 1e-5))
    assert float((ref - want).abs().max()) <= 1e-12 * float(s.max())
    mu, var = R.moments(rows(clean))
    assert torch.allclose(mu[:, 0], rows(clean).mean(1), rtol=0, atol=1e-14) and torch.allclose(var[:, 0], rows(clean).var(1), rtol=1e-13, atol=0)
    assert torch.equal(R.rows_back(rows(clean), clean.shape), clean.double())
    assert bool((s >= ref.abs()).all())
    # the fp32 C oracle: double statistics rounded to fp32, then the four fp32 operations: every rounding is a term of S
    out = np.zeros((n, c, hw), F)
    cn, an = clean.numpy().reshape(n, c, hw), adv.numpy().reshape(n, c, hw)
    c_oracle.oracle_mix_feature(ptr(cn), ptr(an), ptr(out), n, c, hw, F(1e-5))
    got = rows(torch.from_numpy(out).reshape(n, c, hw, 1))
    assert bool(((got - ref).abs() <= 1.5 * U * s).all()), float(((got - ref).abs() / (U * s)).max())


@pytest.mark.filterwarnings("ignore:var")
def test_mix_feature_of_one_channel_is_nan():
    x = torch.randn((4, 1), dtype=torch.float64)
    ref, s = R.mix_feature(x, x + 1, 1e-5, 64)
    assert bool(torch.isnan(ref).all())
    assert bool(torch.isnan(torch.randn(4, 1).var(1)).all())


def test_mix_sensitivity_contains_the_ill_conditioned_row_of_an_fp32_emulation():
    """The channels-last kernel's arithmetic in fp32 on the CPU (a lane's shifted sums, the butterfly of Chan merges) on
    1e3 + 1e-2 N(0, 1): the variance is off float64 by some 1e-4 relative; the M2 sensitivity of the reference holds that."""
    gen = torch.Generator().manual_seed(5)
    c = 512
    x = (1e3 + 1e-2 * torch.randn(c, generator=gen, dtype=torch.float64)).float().numpy()
    parts = []
    for lane in range(64):
        v = x[lane::64]
        sh = v[0]
        s = q = F(0)
        for e in v:
            d = F(e - sh)
            s = F(s + d)
            q = F(q + F(d * d))
        dm = F(s / F(len(v)))
        parts.append((F(len(v)), F(sh + dm), max(F(q - F(s * dm)), F(0))))

    def merge(a, b):
        n = F(a[0] + b[0])
        d, f = F(b[1] - a[1]), F(b[0] / n)
        return n, F(a[1] + F(d * f)), F(F(a[2] + b[2]) + F(F(F(d * d) * a[0]) * f))
    o = 32
    while o:
        parts = [merge(parts[i], parts[i ^ o]) if (i & o) == 0 else merge(parts[i ^ o], parts[i]) for i in range(64)]
        o >>= 1
    x64 = torch.from_numpy(x).double()[None]
    mu, var = R.moments(x64)
    s_mu, s_m2 = R._sens(x64, mu, 64)
    m2 = float(var) * (c - 1)
    rel = abs(float(parts[0][2]) - m2) / m2
    assert rel > 1e-5, "the row is meant to show the loss of accuracy"
    assert abs(float(parts[0][2]) - m2) <= U * float(s_m2) and abs(float(parts[0][1]) - float(mu)) <= U * float(s_mu)
    assert all(p == parts[0] for p in parts), "the lane-symmetric merge order leaves every lane with the same bits"


# ----------------------------------------------------------------------------------------------------------------------- lerp, mix_w
def test_round_sum_has_no_double_rounding():
    # 1 + 2^-24 + 2^-60: above the fp32 midpoint; the float64 sum rounds onto the midpoint, which RNE would take down to 1
    p, q = np.array([2.0 ** -24 + 2.0 ** -60, 2.0 ** -24 - 2.0 ** -60, 2.0 ** -24]), np.array([1.0, 1.0, 1.0])
    assert (p + q).astype(F).tolist() == [1.0, 1.0, 1.0]
    assert R.round_sum_f32(p, q).tolist() == [float(F(1) + F(2.0 ** -23)), 1.0, 1.0]


@pytest.mark.parametrize("n_points", [3, 4, 5])
def test_lerp_reference_matches_torch_the_c_oracle_and_exact_rationals(c_oracle, n_points):
    gen = torch.Generator().manual_seed(n_points)
    n = 4096
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3
    ws = R.sample_weights(n_points)
    out = np.zeros((len(ws), n), F)
    c_oracle.oracle_lerp_points(ptr(a.numpy()), ptr(b.numpy()), ptr(out), n, ptr(np.array(ws, F)), len(ws))
    for k, w in enumerate(ws):
        got = R.lerp_f32(a.numpy(), b.numpy(), w)
        assert np.array_equal(got.view(np.int32), torch.lerp(a, b, float(w)).numpy().view(np.int32)), f"torch.lerp, w = {w}"
        assert np.array_equal(got.view(np.int32), out[k].view(np.int32)), f"C oracle, w = {w}"
        small = abs(w) < 0.5
        coeff = fractions.Fraction(float(w if small else F(w - F(1))))
        for i in range(0, n, 97):
            d = fractions.Fraction(float(F(b[i].item()) - F(a[i].item())))
            exact = coeff * d + fractions.Fraction(float((a if small else b)[i]))
            lo, hi = sorted((float(got[i]), float(np.nextafter(got[i], F(np.inf) if exact > fractions.Fraction(float(got[i])) else F(-np.inf)))))
            assert abs(exact - fractions.Fraction(float(got[i]))) * 2 <= fractions.Fraction(hi) - fractions.Fraction(lo), (i, w)


def test_mix_w_reference_matches_torch():
    gen = torch.Generator().manual_seed(1)
    c, a = torch.randn(1000, generator=gen), torch.randn(1000, generator=gen)
    w = torch.tensor(0.3137)
    assert np.array_equal(R.mix_w_f32(c.numpy(), a.numpy(), 0.3137).view(np.int32), (c + w * (a - c)).numpy().view(np.int32))
    wd = torch.tensor(0.3137, dtype=torch.float64, requires_grad=True)
    g = torch.randn(1000, generator=gen, dtype=torch.float64)
    ((c.double() + wd * (a.double() - c.double())) * g).sum().backward()
    dw, s = R.mix_w_grad(g, c, a)
    assert abs(dw - float(wd.grad)) <= 1e-13 * s


# ------------------------------------------------------------------------------------------------------------------- head and loss
def test_head_reference_matches_torch_autograd():
    gen = torch.Generator().manual_seed(2)
    b, hw, c, k = 5, 6, 20, 7
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    x, w, bias, dl = rn(b, hw, c).requires_grad_(True), rn(k, c).requires_grad_(True), rn(k).requires_grad_(True), rn(b, k)
    x4 = x.permute(0, 2, 1).reshape(b, c, 2, 3)
    pooled_t = torch.nn.functional.adaptive_avg_pool2d(x4, 1).flatten(1)
    logits_t = torch.nn.functional.linear(pooled_t, w, bias)
    (logits_t * dl).sum().backward()
    pooled, sp, logits, sl = R.head_forward(x.detach(), w.detach(), bias.detach())
    assert float((pooled - pooled_t.detach()).abs().max()) <= 1e-14 and float((logits - logits_t.detach()).abs().max()) <= 1e-13
    assert bool((sp >= pooled.abs()).all()) and bool((sl >= logits.abs() - 1e-13).all())
    dx, sdx, dw, sdw, db, sdb = R.head_backward(dl, w.detach(), pooled, hw)
    assert float((dx[:, None, :] - x.grad).abs().max()) <= 1e-14
    assert float((dw - w.grad).abs().max()) <= 1e-13 and float((db - bias.grad).abs().max()) <= 1e-13
    assert torch.equal(R.head_forward(x.detach(), w.detach(), None)[2], pooled @ w.detach().t())


@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (17, 64), (20, 1000)])
def test_cross_entropy_reference_matches_torch_autograd(n, k):
    gen = torch.Generator().manual_seed(n + k)
    for scale in (3.0, 80.0, 1e4):
        l = (torch.randn((n, k), generator=gen, dtype=torch.float64) * scale).requires_grad_(True)
        t = torch.randint(0, k, (n,), generator=gen)
        loss = torch.nn.functional.cross_entropy(l, t)
        loss.backward()
        ref = R.cross_entropy(l.detach(), t)
        assert abs(ref["loss"] - loss.item()) <= 2.0 ** -40 * ref["s_loss"]
        assert bool(((ref["d"] - l.grad).abs() <= 2.0 ** -40 * ref["s_d"]).all())
        assert bool((ref["s_d"] >= ref["d"].abs()).all())


def test_cross_entropy_reference_edges():
    l = torch.tensor([[1.25, 1.25, 1.25], [0.5, float("-inf"), 2.0], [1.0, 2.0, 3.0]], dtype=torch.float64)
    ref = R.cross_entropy(l, torch.tensor([1, 2, 0]))
    assert torch.allclose(ref["d"][0], torch.tensor([1 / 9, 1 / 9 - 1 / 3, 1 / 9], dtype=torch.float64), atol=1e-16)
    assert float(ref["d"][1, 1]) == 0.0 and float(ref["s_d"][1, 1]) == 0.0 and np.isfinite(ref["loss"])
    bad = R.cross_entropy(l, torch.tensor([1, 3, 0]))
    assert np.isnan(bad["loss"]) and bool(torch.isnan(bad["d"][1]).all()) and bool(torch.isfinite(bad["d"][[0, 2]]).all())
    assert torch.equal(bad["d"][[0, 2]], ref["d"][[0, 2]])


def test_perturb_norms_reference(c_oracle):
    gen = torch.Generator().manual_seed(4)
    xc = torch.randn((3, 1000), generator=gen)
    xa = xc + 0.03 * torch.randn((3, 1000), generator=gen)
    linf, l2, ss = R.perturb_norms(xa.numpy(), xc.numpy())
    o2, oi = np.zeros(3, F), np.zeros(3, F)
    c_oracle.oracle_perturb_norms(ptr(xa.numpy()), ptr(xc.numpy()), 3, 1000, ptr(o2), ptr(oi))
    assert np.array_equal(oi, linf) and np.allclose(o2, l2, rtol=3e-7, atol=0)


# ------------------------------------------------------------------------------------------------------------------------- dispatch
def _const(src, name):
    m = re.search(rf"constexpr int {name} = ([^;]+);", src)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}, {"AFAN_WAVE": 64}))


def test_restated_constants_are_those_of_the_sources():
    mix, head, pgd = _src("afan_mix.hip"), _src("afan_head.hip"), _src("afan_pgd.hip")
    assert _const(mix, "BLOCK") == R.BLOCK == _const(head, "BLOCK") and _const(mix, "MAX_LDS_BYTES") == R.MAX_LDS_BYTES
    assert _const(mix, "LM_MAX") == R.LM_MAX and _const(mix, "MIXW_MAX_BLOCKS") == R.MIXW_MAX_BLOCKS
    assert _const(head, "MAXK") == R.MAXK and _const(head, "DW_SLICES") == R.DW_SLICES
    assert _const(head, "CEW_WAVES") == R.CEW_WAVES and _const(head, "CE_BLOCK") == R.CE_BLOCK
    assert _const(pgd, "NORM_CHUNK") == R.NORM_CHUNK
    assert "> 64 * 1024) pix >>= 1" in mix and R.LDS_DEFAULT == 64 * 1024
    assert mix.count("BLOCK, 8192)") == 2 and R.NHWC_GRID_CAP == 8192              # the channels-last grids of mix and lerp_mix
    assert "n * k > (1 << 16)" in head and R.CE_MAX_ELEMS == 1 << 16
    assert "if (k >= 64) ce_fwd_wide_kernel" in head and R.CE_WIDE_K == 64
    assert "c <= 64 * 8" in mix and (R.KEEP_SMALL, R.KEEP_LARGE) == (8, 20) and "mix_feature_nhwc_kernel<T, 20>" in mix


def test_mix_tile_choice():
    want = {19: (64, True), 304: (32, True), 512: (16, True), 1024: (8, True), 2048: (8, True), 6000: (64, False), 232: (64, True)}
    for c, (pix, stage) in want.items():
        assert R._tile(c) == (pix, stage), c
    p = R.mix_plan(2048, 9)
    assert (p["lds"], p["optin"], p["tiles"]) == (71680, True, 2)
    assert R.mix_plan(6000, 6) == dict(pix=8, stage=False, lds=6144, optin=False, tiles=1, tiny=True, groups=32)
    assert R.mix_plan(19, 5)["pix"] == 8 and R.mix_plan(19, 33)["pix"] == 64 and R.mix_plan(19, 32)["pix"] == 32
    # the fused kernel's own opt-in: the tile of mix_feature, five sets of partial moments
    assert not R.mix_plan(232, 72)["optin"] and R.lerp_mix_plan(232, 72)["optin"] and R.lerp_mix_plan(232, 72)["lds"] == 74752
    assert R.mix_plan(232, 72)["pix"] == R.lerp_mix_plan(232, 72)["pix"] == 64
    for c in range(1, 8193):
        for hw in (2, 9, 77):
            a, b = R.mix_plan(c, hw), R.lerp_mix_plan(c, hw)
            assert (a["pix"], a["stage"], a["tiles"]) == (b["pix"], b["stage"], b["tiles"]), (c, hw)
            assert b["lds"] <= 160 * 1024 and a["lds"] <= R.MAX_LDS_BYTES


def test_lerp_mix_never_needed_its_156_kb_guard():
    """afan_lerp_mix used to drop staging when its launch would pass 156 KB.  Staging is only chosen when the clean column and two
    sets of partial moments fit 128 KB, so the fused launch stays at or below 124 928 + 15 360 = 140 288 B: no channel count
    reaches the guard, and the line is gone from the source."""
    assert not any(R.lerp_mix_dead_branch(c) for c in range(1, 8193))
    assert max(R.lerp_mix_bytes(c, *R._tile(c)) for c in range(1, 8193) if R._tile(c)[1]) <= 140288
    assert "156 * 1024" not in _src("afan_mix.hip")


def test_other_dispatch_predicates():
    assert R.nhwc_grid(9) == 3 and R.nhwc_grid(32768) == 8192 and R.nhwc_grid(32769) == 8192
    assert R.mix_w_dot_grid(262144) == 1024 and R.mix_w_dot_grid(262149) == 1024 and R.mix_w_dot_grid(4099) == 17 and R.mix_w_dot_grid(0) == 1
    assert [R.head_fwd_form(True, c, True) for c in (8, 64, 512, 2048, 24, 20, 2056)] == ["vec"] * 4 + ["scalar"] * 3
    assert R.head_fwd_form(True, 64, False) == "scalar" and R.head_fwd_form(False, 64, True) == "scalar"
    assert [R.head_vec_groups(c) for c in (8, 64, 512, 2048)] == [256, 32, 4, 1]
    assert [R.ce_form(n, k) for n, k in ((17, 63), (17, 64), (1024, 64), (65537, 1), (1025, 64))] == ["row", "wide", "wide", None, None]


# ------------------------------------------------------------------------------------------------------------------------- coverage
def test_tables_reach_every_variant():
    """The restated predicates map the GPU tables onto exactly EXPECTED_VARIANTS: every instantiation and inner path of the mixing,
    head and loss kernels."""
    got = G.table_variants()
    assert sorted(got) == G.EXPECTED_VARIANTS, f"missing {sorted(set(G.EXPECTED_VARIANTS) - got)}, unexpected {sorted(got - set(G.EXPECTED_VARIANTS))}"
    assert {(c.n_points, m) for c in G.LERP_CASES for m in G.lerp_masks(c.n_points)} >= {(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (3, 3), (5, 0b1010), (5, 0b0101)}
    assert G.HW_EXACT.keys() == {c.hw for c in G.HEAD_FWD_CASES} and set(G.HW_EXACT.values()) == {1, 4, 16, 64}


BF16_MIX = [c for c in G.MIX_CASES if c.dt == G.BF16 and c.kind != "c1" and c.n * c.hw * c.c <= 1 << 17]


@pytest.mark.parametrize("case", BF16_MIX, ids=G.mix_id)
def test_bf16_midpoint_share_of_the_mix_reference_is_under_half_its_cap(case):
    """A bf16 output may be the other neighbour only where float64 lies within the window of a rounding midpoint, for at most 1 %
    of a case's elements: the share of elements whose window holds a midpoint at all stays under half of that."""
    clean, adv = G.mix_rows(case)
    ref, s = R.mix_feature(clean.reshape(-1, case.c), adv.reshape(-1, case.c), G.EPS, G.mix_lanes(case))
    share = R.midpoint_share(ref, G.mix_measured(case) * U * s)
    assert share <= G.BF16_SHARE_CAP / 2, share


@pytest.mark.parametrize("case", G.HEAD_BWD_CASES, ids=G.head_bwd_id)
def test_bf16_midpoint_share_of_the_head_dx_reference_is_under_half_its_cap(case):
    dl, w, pooled = G.head_bwd_gauss(case)[:3]
    dx, sdx = R.head_backward(dl, w, pooled, case.hw)[:2]
    assert R.midpoint_share(dx, G.c_dx(case.k) * U * sdx) <= G.BF16_SHARE_CAP / 2
