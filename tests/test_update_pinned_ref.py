"""The np.float32 references of tests/update_pinned_refs.py (what tests/test_update_pinned_gpu.py holds the PGD-step, SGD and weight-
transpose kernels to, bit for bit) checked on the CPU: against the project's C oracle bit for bit on the tables' special values,
against torch on the CPU (torch.sign, the attack's masked clamp, .to(torch.bfloat16), three steps of torch.optim.SGD), the permutation
reference against itself; the constants and dispatch predicates restated from the sources; and the coverage of the GPU tables."""
import re

import numpy as np
import pytest
import torch

import test_update_pinned_gpu as G
import update_pinned_refs as R
from conftest import ROOT, ptr

F = np.float32


def _src(name):
    with open(f"{ROOT}/cv_a-fan_amd/csrc/{name}") as f:
        return f.read()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ against the C oracle
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("eps", [G.EPS, F(0)])
def test_pgd_step_reference_equals_the_c_oracle(c_oracle, clip, eps):
    for gdt in (G.F32, G.BF16):
        xa, g, _, xc = G.step_inputs(G.N_RAGGED, gdt)
        assert np.isnan(xa).sum() == 2 and np.isnan(g).sum() == 2 and (g == 0).sum() >= 18 and np.isinf(g).sum() == 4
        got = R.pgd_step(xa, g, xc, G.GAMMA, eps, clip)
        want = xa.copy()
        c_oracle.oracle_pgd_step(ptr(want), ptr(g.copy()), ptr(xc.copy()), xa.size, G.GAMMA, eps, clip)
        assert R.same_f32(got, want) is None
        assert np.array_equal(np.isnan(got), np.isnan(xa) | np.isnan(g)), "NaN in, NaN out, and nowhere else"


def test_axpy_noise_reference_equals_the_c_oracle(c_oracle):
    xa, u = G.noise_inputs(G.N_RAGGED)
    assert u.min() == 0 and u.max() < 1 and (u == np.nextafter(F(1), F(0))).sum() == 2
    want = xa.copy()
    c_oracle.oracle_axpy_noise(ptr(want), ptr(u.copy()), xa.size, G.EPS)
    got = R.axpy_noise(xa, u, G.EPS)
    assert np.array_equal(_bits(got), _bits(want))
    assert float(got[0]) == float(F(0.5) - G.EPS) and float(got[1]) == 0.5               # u = 0 -> -eps, u = 0.5 -> 0


@pytest.mark.parametrize("mom,wd,gscale", [(0.9, 5e-4, 1.0), (0.9, 5e-4, 1.0 / 256), (0.9, 5e-4, 0.0), (0.0, 5e-4, 1.0), (0.9, 0.0, 1.0)])
def test_sgd_reference_equals_the_c_oracle(c_oracle, mom, wd, gscale):
    p, g, m = G.sgd_inputs(G.N_RAGGED)
    wp, wm = p.copy(), m.copy()
    rp, rm = p, m
    for lr in G.LRS:
        c_oracle.oracle_sgd_step(ptr(wp), ptr(g.copy()), ptr(wm), p.size, F(lr), F(mom), F(wd), F(gscale))
        rp, rm = R.sgd_step(rp, g, rm, lr, mom, wd, gscale, False)
        assert np.array_equal(_bits(rp), _bits(wp)) and np.array_equal(_bits(rm), _bits(wm))
    # the first step: momentum = the decayed gradient whatever the buffer held; a zero buffer on the later-step form gives the same values
    fp, fm = R.sgd_step(p, g, np.full_like(m, np.nan), 0.1, mom, wd, gscale, True)
    lp, lm = R.sgd_step(p, g, np.zeros_like(m), 0.1, mom, wd, gscale, False)
    assert np.isfinite(fp).all() and np.array_equal(fp, lp) and np.array_equal(fm, lm)


# ------------------------------------------------------------------------------------------------------------- against torch (CPU)
def _attack_clamp(t, lo, hi):
    """The attack's in-place masked clamp, restated with torch."""
    t = t.clone()
    low = t < lo
    t[low] = lo[low]
    high = t > hi
    t[high] = hi[high]
    return t


def test_sign_step_and_clamp_references_equal_torch():
    xa, g, _, xc = G.step_inputs(G.N_RAGGED, G.F32)
    tg = torch.from_numpy(g.copy())
    # a NaN gradient: the kernels, the C oracle and this reference propagate it (sign(NaN) = NaN, the contract the GPU tables hold);
    # torch.sign on the CPU computes (0 < g) - (g < 0), which is 0 there, so those elements are compared apart
    gn = np.isnan(g)
    s = R.sign(g)
    assert gn.sum() == 2 and R.same_f32(s[~gn], torch.sign(tg).numpy()[~gn]) is None
    assert not np.signbit(s[g == 0]).any() and np.isnan(s[gn]).all()
    for clip in (0, 1):
        t = torch.from_numpy(xa.copy())
        t.add_(float(G.GAMMA) * torch.sign(tg))
        if clip:
            c = torch.from_numpy(xc.copy())
            t = _attack_clamp(t, c - float(G.EPS), c + float(G.EPS))
        got = R.pgd_step(xa, g, xc, G.GAMMA, G.EPS, clip)
        assert R.same_f32(got[~gn], t.numpy()[~gn]) is None and np.isnan(got[gn]).all()
    t, lo, hi = G.clamp_inputs(G.N_RAGGED)
    got = R.clamp(t, lo, hi)
    assert R.same_f32(got, _attack_clamp(*(torch.from_numpy(a.copy()) for a in (t, lo, hi))).numpy()) is None
    # lo = 1 > hi = -1: whatever t was, the second `if` has the last word; NaN bounds leave t alone
    assert got[:3].tolist() == [-1.0, -1.0, -1.0] and np.isnan(got[3]) and got[4:8].tolist() == [-3.0, 1.0, 3.0, -1.0]


def test_bf16_reference_equals_torch_and_the_table():
    x = G.cast_inputs(G.N_RAGGED)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_bits(x)
    assert R.same_bf16(got, want) is None
    tab = np.array([a for a, _ in G.CAST_TABLE], np.uint32).view(F)
    assert R.same_bf16(R.bf16_bits(tab), np.array([b for _, b in G.CAST_TABLE], np.uint16)) is None
    assert R.bf16_is_nan(R.bf16_bits(tab)).sum() == 3
    # no subnormal operand in the tables, and widening undoes the rounding of a bf16 value
    fin = np.isfinite(x) & (x != 0)
    assert (np.abs(x[fin]) >= F(2.0 ** -126)).all()
    keep = ~R.bf16_is_nan(got)
    assert np.array_equal(R.bf16_bits(R.bf16_widen(got))[keep], got[keep])


def test_sgd_reference_matches_torch_optim_sgd():
    p0, _, _ = G.sgd_inputs(G.N_RAGGED)
    rng = np.random.default_rng(3)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([pt], 0.1, momentum=G.MOM, weight_decay=G.WD)
    rp, rm = p0, np.zeros_like(p0)
    for it, lr in enumerate(G.LRS):
        g = rng.standard_normal(p0.size).astype(F)
        for grp in opt.param_groups:
            grp["lr"] = lr
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        rp, rm = R.sgd_step(rp, g, rm, lr, G.MOM, G.WD, 1.0, it == 0)
        # torch's CPU kernels may fuse: a few fp32 ulps (the tolerance of test_sgd_vs_c_oracle_and_torch)
        np.testing.assert_allclose(rp, pt.detach().numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(rm, opt.state[pt]["momentum_buffer"].numpy(), rtol=1e-6, atol=1e-7)


# --------------------------------------------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("k,rs,c", [(8, 1, 8), (80, 9, 48), (72, 1, 40)])
def test_permutation_reference_applied_twice_returns_the_source(k, rs, c):
    n = k * rs * c
    src = (np.arange(n) * 7 + 1 & 0xffff).astype(np.uint16)
    d1, _ = R.make_descs([(0, 0, k, rs, c, rs, 0)])
    mid = R.transpose_weights(src, np.full(n, 0xa5a5, np.uint16), d1)
    assert mid.reshape(c, rs, k)[3, rs - 1, 5] == src.reshape(k, rs, c)[5, rs - 1, 3]
    d2, _ = R.make_descs([(0, 0, c, rs, k, rs, 0)])                      # the roles of K and C swapped
    back = R.transpose_weights(mid, np.full(n, 0xa5a5, np.uint16), d2)
    assert np.array_equal(back, src) and (rs * c == 1 or not np.array_equal(mid, src))


def test_permutation_reference_leaves_what_no_descriptor_owns():
    rows = G._six()
    descs, tiles = R.make_descs(rows)
    assert tiles == sum(R.transpose_tiles(r[2], r[3], r[4]) for r in rows) and descs[:, 5].tolist() == sorted(descs[:, 5].tolist())
    n_src, n_dst = G.transpose_extent(rows)
    src = (np.arange(n_src) & 0xffff).astype(np.uint16)
    dst = R.transpose_weights(src, np.full(n_dst, 0xa5a5, np.uint16), descs)
    owned = sum(r[2] * r[3] * r[4] for r in rows)
    assert n_dst - owned > 0 and (dst != 0xa5a5).sum() >= owned - 2 and (dst == 0xa5a5).sum() >= n_dst - owned
    # source tensors and destination operands do not overlap, every offset keeps 16-byte alignment
    spans = sorted((r[0], r[0] + r[2] * r[3] * r[4]) for r in rows)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    ops = sorted({(r[1], r[1] + r[4] * r[5] * r[2]) for r in rows})
    assert all(a[1] <= b[0] for a, b in zip(ops, ops[1:])) and len(ops) == 4
    for rows in G.TRANSPOSE_CASES:
        assert all(r[0] % 8 == 0 and r[1] % 8 == 0 and r[2] % 8 == 0 and r[4] % 8 == 0 and r[6] + r[3] <= r[5] for r in rows)


# ------------------------------------------------------------------------------------------------------------------------- dispatch
def _const(src, name):
    m = re.search(rf"constexpr int {name} = ([^;]+);", src)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}, {"AFAN_WAVE": 64}))


def test_restated_constants_are_those_of_the_sources():
    pgd, sgd, conv, common = _src("afan_pgd.hip"), _src("afan_sgd.hip"), _src("afan_conv.hip"), _src("afan_common.h")
    assert _const(pgd, "BLOCK") == _const(sgd, "BLOCK") == R.BLOCK and _const(pgd, "NORM_CHUNK") == R.NORM_CHUNK
    assert "#define AFAN_WAVE 64" in common and R.WAVE == 64 and "s += AFAN_WAVE" in pgd
    assert "int max_blocks = 256 * 8" in common and R.GRID_CAP == 256 * 8
    assert pgd.count("batch > 65535") == 2 and R.MAX_BATCH == 65535
    assert "tile[64][64 + 8]" in conv and "(Cc + 63) / 64" in conv and R.TILE == 64
    # the alignment rules that choose the vector kernels
    assert ("aligned(x_adv, 16) && aligned(grad, 4 * sizeof(G)) &&\n                     (!CLIP || aligned(x_clean, 16)) && "
            "(!SHADOW || aligned(shadow, 8))") in pgd
    assert ("(per_sample % 4 == 0) && aligned(x_adv, 16) && aligned(x_clean, 16) &&\n                     "
            "(!STEP || aligned(grad, 4 * sizeof(G))) && (!SHADOW || aligned(shadow, 8))") in pgd
    assert "aligned(x_adv, 16) && aligned(u, 16) && (!shadow_bf16 || aligned(shadow_bf16, 8))" in pgd
    assert "const int vec = aligned(src, 16) && aligned(dst, 16);" in pgd
    assert "aligned(x, 16) && aligned(x_adv, 16) && (!x32 || aligned(x32, 16)) && (!shadow || aligned(shadow, 16))" in pgd
    assert ("aligned(param, 16) && aligned(grad, 16) && aligned(momentum_buf, 16) &&\n                    "
            "(!shadow_bf16 || aligned(shadow_bf16, 8))") in sgd
    assert pgd.count("grid_for(vec ? (n + 3) / 4 : n, BLOCK)") == 2 and pgd.count("grid_for(vec ? (n + 7) / 8 : n, BLOCK)") == 2
    assert "grid_for(vec ? (n + 3) / 4 : n, BLOCK)" in sgd and "grid_for(n16, BLOCK)" in sgd
    codes = _src("../../include/afan_hip.h")
    for name in ("OK", "EDTYPE", "EALIGN", "ESHAPE", "ENULL"):
        assert re.search(rf"AFAN_{name} = (-?\d+)", codes).group(1) == str(getattr(R, "AFAN_" + name))


def test_sizes_are_the_smallest_with_a_second_trip():
    assert (R.T4, R.T8, R.T1) == (4 * 2048 * 256 + 4 * 256 * 3 + 3, 8 * 2048 * 256 + 8 * 100 + 5, 2048 * 256 + 777)
    assert R.grid_for(1) == 1 and R.grid_for(0) == 1 and R.grid_for(257) == 2 and R.grid_for(1 << 30) == 2048
    full = R.GRID_CAP * R.BLOCK
    for width, t in ((4, R.T4), (8, R.T8)):
        assert R.loop_trips(width * full + width - 1, True, width) == 1 and R.loop_trips(width * full + width, True, width) == 2
        assert R.loop_trips(t, True, width) == 2 and t % width and t // width - full < full    # some threads two trips, some one
    assert R.loop_trips(full, False, 1) == 1 and R.loop_trips(full + 1, False, 1) == 2 and R.loop_trips(R.T1, False, 1) == 2
    assert R.loop_trips(1 << 20, True, 4) == 1 and R.loop_trips(100003, False, 1) == 1       # the largest cases of the older tests
    assert R.norm_slices(G.P_FIN_V) == 66 and R.norm_slices(64 * R.NORM_CHUNK) == 64 and R.norms_workspace_floats(3, 4097) == 12
    assert R.transpose_tiles(80, 9, 48) == 18 and R.transpose_tiles(256, 9, 304) == 4 * 9 * 5 and R.transpose_tiles(8, 1, 8) == 1


def test_alignment_predicates():
    assert R.step_scalar_terms(4, 1, 1, (0, 0, 0, 0)) == [] and R.step_scalar_terms(2, 1, 1, (0, 8, 0, 8)) == []
    assert R.step_scalar_terms(4, 1, 1, (4, 4, 4, 2)) == ["x_adv", "grad", "x_clean", "shadow"]
    assert R.step_scalar_terms(2, 0, 0, (0, 2, 4, 2)) == ["grad"] and R.step_scalar_terms(2, 1, 1, (0, 4, 0, 4)) == ["grad", "shadow"]
    assert R.step_norms_scalar_terms(4, 0, 4097, (0, 0, 0, 2)) == ["per%4"] and R.step_norms_scalar_terms(4, 0, 8, (0, 0, 4, 0)) == ["x_clean"]
    assert R.noise_vec(0, (0, 0, 2)) and not R.noise_vec(1, (0, 0, 2)) and R.noise_vec(1, (0, 0, 8)) and not R.noise_vec(0, (0, 4, 0))
    assert R.sgd_vec(1, (0, 0, 0, 8)) and not R.sgd_vec(1, (0, 0, 0, 4)) and not R.sgd_vec(0, (0, 0, 4, 0))
    assert R.cast_vec((0, 0)) and not R.cast_vec((0, 8))
    assert R.init_scalar_terms(1, 1, (0, 0, 0, 8)) == ["shadow"] and R.init_scalar_terms(0, 0, (0, 4, 0, 8)) == []


# ------------------------------------------------------------------------------------------------------------------------- coverage
def test_tables_reach_every_variant():
    """The restated predicates map the GPU tables onto exactly EXPECTED_VARIANTS: every instantiation and inner path of the PGD-step,
    SGD and weight-transpose kernels."""
    got = G.table_variants()
    assert sorted(got) == G.EXPECTED_VARIANTS, f"missing {sorted(set(G.EXPECTED_VARIANTS) - got)}, unexpected {sorted(got - set(G.EXPECTED_VARIANTS))}"
    for name in ("trip2", "ragged_tail", "finalize_trip2", "partial_k_tile", "partial_c_tile", "multi_desc"):
        assert any(name in t for t in got), name
    small = set(R.SMALL_N)
    assert small <= {c.n for c in G.STEP_CASES} and small <= {c.n for c in G.NOISE_CASES} and small <= {c.n for c in G.SGD_CASES}
    assert small <= {n for n, _ in G.CAST_CASES} and small <= {c.n for c in G.INIT_CASES}
    assert {(c.batch, c.per) for c in G.NORM_CASES} >= {(R.MAX_BATCH, 1), (R.MAX_BATCH, 4), (2, G.P_FIN_V), (2, G.P_FIN_S)}
    assert {c.per for c in G.NORM_CASES} >= {1, 7, 4096, 4097, 4100}
    assert max(c.n for c in G.STEP_CASES + G.SGD_CASES) == R.T4 and max(n for n, _ in G.CAST_CASES) == R.T8 and 4 * R.T8 < 17.5e6
