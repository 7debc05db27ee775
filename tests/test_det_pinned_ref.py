"""The float64 references of tests/det_pinned_refs.py (what tests/test_det_pinned_gpu.py holds the ROIAlign and linear-pair kernels
to) checked on the CPU: against the fp32 C oracle (oracle_roi_align, itself pinned bit for bit to the reference's CPU kernel) within
the rounding bound counted from the oracle's expression, against the torch restatement in float64, bit for bit on the exact table,
and the tables' own conditions (exactness, samples on the validity edges, the share of bf16 rounding midpoints)."""
import numpy as np
import pytest
import torch

import det_pinned_refs as R
from conftest import oracle_roi

U = R.U
N, H, W = 2, 13, 18
SCALE = 1 / 16
# oracle_roi_align: acc += w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4 per sample (weight product, tap product, three inner adds, the add
# into acc), acc / count: 5 + (samples of the bin) + 1 roundings on the longest path; backward: g * w / count added in index
# order: weight product, product, division, one add per arriving term
C_ORACLE_FWD_FIXED, C_ORACLE_BWD_FIXED = 6, 3


def _data(shape, gen, exact, bf16=False):
    if exact:
        return R.ints(shape, 8, gen)
    t = torch.randn(shape, generator=gen)
    return (t.bfloat16() if bf16 else t).double()


CASES = [(7, 7, 0, 60), (7, 5, 2, 40), (14, 14, 0, 30), (16, 16, 4, 24), (17, 17, 0, 12), (7, 7, 4, 1300)]


@pytest.mark.parametrize("ph,pw,sr,r", CASES, ids=lambda v: str(v))
def test_gaussian_table_matches_the_fp32_oracle_within_the_counted_bound(c_oracle, ph, pw, sr, r):
    c = 3
    gen = torch.Generator().manual_seed(ph * 100 + sr)
    rois = R.gauss_rois(r, N, H, W, ph, pw, seed=ph + sr)
    g = R.roi_geom(rois, SCALE, ph, pw, H, W, sr)
    ov = R.overlaps(g)
    assert 0.3 * r <= ov.sum() < r, "ROIs on the map and ROIs outside it"
    assert (rois[:, 3] < rois[:, 1]).any() and (rois[:, 4] < rois[:, 2]).any(), "malformed ROIs"
    x, dy = _data((N, c, H, W), gen, False), _data((r, c, ph, pw), gen, False)
    y, s, k = R.roi_align_fwd(x, g)
    got = torch.from_numpy(oracle_roi(c_oracle, x.float().numpy(), rois, ph, pw, SCALE, sr)).double()
    x32 = x.float().double()
    y32, s32, _ = R.roi_align_fwd(x32, g)
    bound = (C_ORACLE_FWD_FIXED + k[:, None].double()) * U * s32
    assert bool(((got - y32).abs() <= bound).all()), float(((got - y32).abs() / bound.clamp_min(1e-300)).max())
    assert bool((s >= y.abs() - 1e-12).all())
    dy32 = dy.float().double()
    dx, sb, ks, kg = R.roi_align_bwd(dy32, g, N)
    gotb = torch.from_numpy(oracle_roi(c_oracle, x.float().numpy(), rois, ph, pw, SCALE, sr, mode=1, dy=dy32.float().numpy())).double()
    boundb = (C_ORACLE_BWD_FIXED + ks[:, None].double()) * U * sb
    assert bool(((gotb - dx).abs() <= boundb).all()), float(((gotb - dx).abs() / boundb.clamp_min(1e-300)).max())
    assert bool((kg <= ks).all()) and bool((sb.sum(1)[ks == 0] == 0).all())
    # the adjoint identity of the reference itself, in float64
    lhs, rhs = float((dx * x32).sum()), float((dy32 * y32).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((dy32.abs() * s32).sum())


def test_gaussian_table_matches_the_torch_restatement_in_float64(orc):
    """oracle.roi_align_torch takes its coordinates in another association (start + (p + (i + .5) / grid) * bin): a sample moves by a
    few fp32 ulps of a coordinate below 32 cells, a weight by as much; the forward and the autograd gradient agree to that times the
    plain sum of the taps' absolute values."""
    ph, pw, c, r = 7, 5, 2, 36
    gen = torch.Generator().manual_seed(7)
    for sr in (0, 2):
        rois = R.gauss_rois(r, N, H, W, ph, pw, seed=70 + sr)
        g = R.roi_geom(rois, SCALE, ph, pw, H, W, sr)
        x = _data((N, c, H, W), gen, False).requires_grad_(True)
        dy = _data((r, c, ph, pw), gen, False)
        want = orc.roi_align_torch(x, torch.from_numpy(rois), (ph, pw), SCALE, sr)
        want.backward(dy)
        y, s, _ = R.roi_align_fwd(x.detach(), g)
        tol = 8 * 2.0 ** -23 * 32
        ny, nx = torch.from_numpy((g.y.A != 0) * 1.0), torch.from_numpy((g.x.A != 0) * 1.0)
        cnt = torch.from_numpy(g.count).view(-1, 1, 1, 1)
        taps = torch.stack([torch.einsum("ph,chw,qw->cpq", ny[i], x.detach()[int(g.batch[i])].abs(), nx[i]) for i in range(r)]) / cnt
        assert bool(((y - want.detach()).abs() <= tol * 2 * taps + 1e-15).all())
        dx, sb, _, _ = R.roi_align_bwd(dy, g, N)
        tb = torch.zeros_like(dx)
        for i in range(r):
            tb[int(g.batch[i])] += torch.einsum("ph,cpq,qw->chw", ny[i], dy[i].abs() / g.count[i], nx[i])
        assert bool(((dx - x.grad).abs() <= tol * 2 * tb + 1e-15).all())


EXACT = [(7, 7, 0, 60), (7, 5, 2, 40), (14, 14, 0, 24), (16, 16, 4, 24), (17, 17, 0, 12), (7, 7, 0, 1300)]


@pytest.mark.parametrize("ph,pw,sr,r", EXACT, ids=lambda v: str(v))
def test_exact_table_is_exact_and_agrees_bit_for_bit(c_oracle, orc, ph, pw, sr, r):
    c = 3
    gen = torch.Generator().manual_seed(ph + sr + r)
    rois = R.exact_rois(r, N, H, W, ph, pw, seed=ph * 10 + sr, sampling_ratio=sr)
    g = R.roi_geom(rois, SCALE, ph, pw, H, W, sr)
    # the table's own conditions
    assert set(np.unique(g.batch)) == {0, 1}
    assert R.overlaps(g).sum() * 2 >= r, "at least half of the ROIs overlap the map"
    assert set(np.unique(g.count)) <= {1.0, 2.0, 4.0, 8.0, 16.0}
    for a, size in ((g.y, H), (g.x, W)):
        lo_edge, hi_edge = R.edge_samples(a, size)
        assert lo_edge > 0 and hi_edge > 0, "samples exactly at -1 and exactly at the size"
    x, dy = _data((N, c, H, W), gen, True), _data((r, c, ph, pw), gen, True)
    assert float(x.abs().max()) <= 8 and float(dy.abs().max()) <= 8
    y, s, _ = R.roi_align_fwd(x, g)
    dx, sb, _, _ = R.roi_align_bwd(dy, g, N)
    ok, k = R.exact_range_ok(g, max(float(s.max()), float(sb.max())))
    assert ok, (k, float(s.max()), float(sb.max()))
    got = oracle_roi(c_oracle, x.float().numpy(), rois, ph, pw, SCALE, sr)
    assert np.array_equal(got.astype(np.float64), y.numpy())
    gotb = oracle_roi(c_oracle, x.float().numpy(), rois, ph, pw, SCALE, sr, mode=1, dy=dy.float().numpy())
    assert np.array_equal(gotb.astype(np.float64), dx.numpy())
    # the float64 C oracle too (its geometry is float64: the same numbers on this table)
    assert np.array_equal(oracle_roi(c_oracle, x.numpy(), rois, ph, pw, SCALE, sr), y.numpy())
    if r <= 60:                                            # the torch restatement loops over the ROIs
        xt = x.clone().requires_grad_(True)
        want = orc.roi_align_torch(xt, torch.from_numpy(rois), (ph, pw), SCALE, sr)
        want.backward(dy)
        assert torch.equal(want.detach(), y) and torch.equal(xt.grad, dx)
        assert np.array_equal(want.detach().float().numpy(), got)


def test_malformed_rois_are_inexact():
    """end < start gives an extent of 1 and bin = 1 / P: not dyadic for P = 7, which is why such ROIs belong to the Gaussian table."""
    rois = np.array([[0, 64, 64, 32, 32]], np.float32)
    g = R.roi_geom(rois, SCALE, 7, 7, H, W, 0)
    assert R.dyadic_bits(g.y.A) > 14 and not R.exact_range_ok(g, 8.0)[0]


def test_gather_path_census():
    """Bins of at least one cell meet a row in at most 3 bins; bins below one cell in more."""
    big = np.array([[0, 16, 16, 16 + 7 * 32, 16 + 7 * 32]], np.float32)          # 2-cell bins
    small = np.array([[0, 16, 16, 16 + 7 * 4, 16 + 7 * 4]], np.float32)          # quarter-cell bins
    assert R.gather_paths(R.roi_geom(big, SCALE, 7, 7, H, W, 0))[1] == 0
    s, l = R.gather_paths(R.roi_geom(small, SCALE, 7, 7, H, W, 0))
    assert l > 0


@pytest.mark.parametrize("ph,c_fixed", [(7, 6), (14, 6)])
def test_bf16_midpoint_share_of_the_reference_is_under_its_cap(ph, c_fixed):
    """A bf16 output may be the other neighbour only where float64 lies within the fp32 noise of a rounding midpoint; at most 1 % of a
    case's elements may use that: the share of elements whose window holds a midpoint at all stays under it."""
    gen = torch.Generator().manual_seed(3)
    for sr in (0, 2):
        rois = R.gauss_rois(48, N, H, W, ph, ph, seed=5 + sr)
        g = R.roi_geom(rois, SCALE, ph, ph, H, W, sr)
        x = _data((N, 8, H, W), gen, False, bf16=True)
        y, s, k = R.roi_align_fwd(x, g)
        share = R.midpoint_share(y, (c_fixed + 1 + k[:, None].double()) * U * s)
        assert share <= 0.01, share


def test_rne_bf16_decides_on_the_float64_value():
    one, ulp = 1.0, 2.0 ** -7                                                   # bf16 neighbours of 1.0: 1 and 1 + 2^-7
    mid = one + ulp / 2
    ref = torch.tensor([mid, mid + 2.0 ** -40, mid - 2.0 ** -40, one + ulp + ulp / 2, -mid - 2.0 ** -40, 0.0, 3.0], dtype=torch.float64)
    want = torch.tensor([one, one + ulp, one, one + 2 * ulp, -(one + ulp), 0.0, 3.0]).bfloat16()
    assert torch.equal(R.rne_bf16(ref), want)
    lo, hi = R.bf16_edges(want)
    assert bool((lo <= ref).all()) and bool((ref <= hi).all())


def test_linear_pair_reference_matches_torch():
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((33, 68), generator=gen, dtype=torch.float64, requires_grad=True)
    w1 = torch.randn((31, 68), generator=gen, dtype=torch.float64, requires_grad=True)
    w2 = torch.randn((2, 68), generator=gen, dtype=torch.float64, requires_grad=True)
    b1 = torch.randn(31, generator=gen, dtype=torch.float64, requires_grad=True)
    b2 = torch.randn(2, generator=gen, dtype=torch.float64, requires_grad=True)
    g1, g2 = torch.randn((33, 31), generator=gen, dtype=torch.float64), torch.randn((33, 2), generator=gen, dtype=torch.float64)
    r1, r2 = torch.nn.functional.linear(x, w1, b1), torch.nn.functional.linear(x, w2, b2)
    ((r1 * g1).sum() + (r2 * g2).sum()).backward()
    y1, s1, y2, s2 = R.linear_pair(x.detach(), w1.detach(), b1.detach(), w2.detach(), b2.detach())
    assert float((y1 - r1.detach()).abs().max()) <= 1e-12 and float((y2 - r2.detach()).abs().max()) <= 1e-12
    assert bool((s1 >= y1.abs() - 1e-12).all()) and bool((s2 >= y2.abs() - 1e-12).all())
    gx, sx, ((gw1, sw1, gb1, sb1), (gw2, sw2, gb2, sb2)) = R.linear_pair_grads(g1, g2, x.detach(), w1.detach(), w2.detach())
    assert float((gx - x.grad).abs().max()) <= 1e-12 and float((gw1 - w1.grad).abs().max()) <= 1e-12
    assert float((gw2 - w2.grad).abs().max()) <= 1e-12 and float((gb1 - b1.grad).abs().max()) <= 1e-12
    assert float((gb2 - b2.grad).abs().max()) <= 1e-12 and bool((sx >= gx.abs() - 1e-12).all()) and bool((sw1 >= gw1.abs() - 1e-12).all())
    nb = R.linear_pair(x.detach(), w1.detach(), None, w2.detach(), None)
    assert torch.equal(nb[0], x.detach() @ w1.detach().t())
