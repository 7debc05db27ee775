"""The float64 references of tests/seg_pinned_refs.py (what tests/test_seg_pinned_gpu.py holds the DeepLab layer kernels to) checked on
the CPU against torch in float64, and the operands of the exact checks checked for exactness.  torch evaluates the resize's source
index in fp32 with its own association, so weights may differ by a few ulps of the source coordinate: 4e-7 * max(h, w) per weight,
as the existing suite allows; everything else is float64 against float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_pinned_refs as R

RESIZES = [((1, 1), (4, 3)), ((5, 9), (5, 9)), ((5, 9), (20, 18)), ((9, 9), (33, 33)), ((17, 23), (40, 31)), ((40, 31), (17, 23)),
           ((33, 33), (129, 129)), ((3, 4), (12, 16))]


@pytest.mark.parametrize("src,dst", RESIZES, ids=lambda v: "x".join(map(str, v)))
def test_resize_and_adjoint_match_torch(src, dst):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((3, 2) + src, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((3, 2) + dst, generator=g, dtype=torch.float64)
    y = F.interpolate(x, size=dst, mode="bilinear", align_corners=False)
    y.backward(dy)
    tol = 4e-7 * max(src + dst)
    got, s, taps = R.resize_fwd(x.detach(), *dst)
    assert float(((got - y.detach()).abs() - tol * 2 * taps).max()) <= 0, "forward"
    dx, sb = R.resize_bwd(dy, *src)
    # every weight of the column is off by at most tol: |dx - torch| <= tol * (number of terms) * max |dy| ... bounded by the plain tap sum
    ny = torch.from_numpy((R.axis_matrix(src[0], dst[0]) != 0).astype(np.float64))
    nx = torch.from_numpy((R.axis_matrix(src[1], dst[1]) != 0).astype(np.float64))
    tb = torch.einsum("oi,ncop,pj->ncij", ny, dy.abs(), nx)
    assert float(((dx - x.grad).abs() - tol * 2 * tb).max()) <= 0, "adjoint"
    assert bool((s >= got.abs() - 1e-12).all()) and bool((sb >= dx.abs() - 1e-12).all())
    # rows of each axis matrix sum to 1 within one fp32 rounding; at most two taps per output
    for a, b in zip(src, dst):
        w = R.axis_matrix(a, b)
        assert np.abs(w.sum(1) - 1.0).max() <= 2.0 ** -23 and ((w != 0).sum(1) <= 2).all() and (w >= 0).all()


@pytest.mark.parametrize("a,b", [(1, 1), (1, 2), (1, 4), (5, 5), (5, 10), (5, 20), (9, 18), (33, 132), (65, 65), (3, 12)])
def test_dyadic_weights_are_multiples_of_an_eighth(a, b):
    assert R.dyadic(a, b)
    w = R.axis_matrix(a, b)
    assert (w * 8 == np.round(w * 8)).all() and (w.sum(1) == 1.0).all()
    i0, i1, l0, l1, src = R.axis_table(a, b)
    assert ((src * 8) == np.round(src * 8)).all() and (l0.astype(np.float64) + l1 == 1.0).all()


def test_exact_resize_operands_are_exact():
    """|x| <= 64 and weights in eighths: every product of two weights and a value is a multiple of 1/64 below 2^7, every partial sum
    of the k x k terms (k counted here: the border inputs of a ratio of 4 feed 8 outputs per axis) stays below 2^24 / 64: exact in fp32
    in any order."""
    for a, b in [(1, 4), (5, 20), (9, 18), (7, 7)]:
        k = R.resize_terms(a, b)
        assert k <= 8
        assert 64 * 64 * k * k < 2 ** 24


@pytest.mark.parametrize("ignore", [255, -100])
def test_cross_entropy_matches_torch(ignore):
    g = torch.Generator().manual_seed(2)
    x = (torch.randn((2, 5, 4, 6), generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    t = torch.randint(0, 5, (2, 4, 6), generator=g)
    t[torch.rand((2, 4, 6), generator=g) < 0.3] = ignore
    loss = torch.nn.CrossEntropyLoss(ignore_index=ignore)(x, t)
    loss.backward()
    got, grad, count = R.ce2d(x.detach(), t, ignore, 0.7)
    assert count == int((t != ignore).sum())
    assert abs(float(got - loss.detach())) <= 1e-13 * max(1.0, abs(float(loss)))
    assert float((grad - 0.7 * x.grad).abs().max()) <= 1e-14
    # no live pixel: NaN loss, zero gradient; logits of +-80 stay finite
    got, grad, count = R.ce2d(x.detach(), torch.full_like(t, ignore), ignore, 1.0)
    assert count == 0 and bool(torch.isnan(got)) and float(grad.abs().max()) == 0.0
    big = torch.where(torch.rand((2, 5, 4, 6), generator=g) < 0.5, 80.0, -80.0).double()
    got, grad, _ = R.ce2d(big, t, ignore, 1.0)
    assert bool(torch.isfinite(got)) and bool(torch.isfinite(grad).all())


def pool_input(shape, gen, special=True):
    """Post-ReLU values (ties at 0), one plane of -inf, NaNs at the first, a middle and the last position of a window."""
    x = torch.randn(shape, generator=gen).clamp_min(0.0).to(torch.bfloat16).double().numpy()
    if special and shape[1] > 1:
        x[0, 1] = -np.inf
    if special and shape[2] >= 3 and shape[3] >= 3:
        x[0, 0, 0, 0] = np.nan
        x[-1, 0, shape[2] // 2, shape[3] // 2] = np.nan
        x[-1, -1, -1, -1] = np.nan
        x[-1, 0, 1, 1] = np.nan
    return x


@pytest.mark.parametrize("k,s,p,hw", [(3, 2, 1, (9, 11)), (2, 2, 0, (8, 6)), (7, 1, 0, (7, 7)), (5, 3, 2, (11, 9)), (15, 1, 7, (9, 9)),
                                      (3, 2, 1, (1, 1)), (15, 2, 0, (17, 16))])
def test_maxpool_matches_torch(k, s, p, hw):
    g = torch.Generator().manual_seed(3)
    x = pool_input((2, 3) + hw, g)
    y, idx = R.maxpool_fwd(x, k, s, p)
    ty, ti = F.max_pool2d(torch.from_numpy(x), k, s, p, return_indices=True)
    assert np.array_equal(y, ty.numpy(), equal_nan=True)
    ho, wo = y.shape[2:]
    oy, ox = np.meshgrid(np.arange(ho), np.arange(wo), indexing="ij")
    flat = (oy * s - p + idx.astype(np.int64) // k) * hw[1] + (ox * s - p + idx.astype(np.int64) % k)
    assert np.array_equal(flat, ti.numpy()), "winner positions (ties, NaN, -inf windows)"
    dy = R.ints(y.shape, 3, g).numpy()
    dx, sa, terms = R.maxpool_bwd(dy, idx, hw[0], hw[1], k, s, p)
    ref = torch.zeros(2 * 3, hw[0] * hw[1], dtype=torch.float64).scatter_add_(1, ti.reshape(6, -1), torch.from_numpy(dy).reshape(6, -1))
    assert np.array_equal(dx.reshape(6, -1), ref.numpy()) and terms <= (-(-k // s)) ** 2 and (sa >= np.abs(dx)).all()


def test_avgpool_pointwise_linear_match_torch():
    g = torch.Generator().manual_seed(4)
    x = torch.randn((3, 8, 17), generator=g, dtype=torch.float64)
    y, s = R.avgpool_fwd(x)
    assert float((y - x.mean(2)).abs().max()) <= 1e-15 and bool((s >= y.abs()).all())
    for bias in (True, False):
        x = torch.randn((65, 16), generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn((5, 16), generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(5, generator=g, dtype=torch.float64, requires_grad=True) if bias else None
        dy = torch.randn((65, 5), generator=g, dtype=torch.float64)
        if bias:        # the classifier: F.conv2d on [1, ci, m, 1]
            ref = F.conv2d(x.t().reshape(1, 16, 65, 1), w.reshape(5, 16, 1, 1), b).reshape(5, 65).t()
        else:
            ref = F.linear(x, w)
        ref.backward(dy)
        y, s = R.pointwise_fwd(x.detach(), w.detach(), None if b is None else b.detach())
        dx, sdx, dw, sdw, db, sdb = R.pointwise_bwd(dy, x.detach(), w.detach())
        assert float((y - ref.detach()).abs().max()) <= 1e-13 and float((dx - x.grad).abs().max()) <= 1e-13
        assert float((dw - w.grad).abs().max()) <= 1e-12 and (b is None or float((db - b.grad).abs().max()) <= 1e-12)
        assert bool((s >= y.abs() - 1e-12).all()) and bool((sdx >= dx.abs() - 1e-12).all()) and bool((sdw >= dw.abs() - 1e-12).all())


def test_ternary_operands_are_exact():
    g = torch.Generator().manual_seed(5)
    for m, ci, co in [(65536 + 64 + 5, 8, 32), (65, 512, 32), (16, 2048, 256)]:
        x, w, dy = R.ternary((m, ci), g), R.ternary((co, ci), g), R.ternary((m, co), g)
        assert R.products_exact(x, w.t()) and R.products_exact(dy, w) and R.products_exact(dy.t(), x)
        assert m < 2 ** 24 and ci < 2 ** 24


def test_dropout_reference():
    x = torch.randn(1000, generator=torch.Generator().manual_seed(6))
    mask = (torch.arange(1000) % 3 != 0).to(torch.uint8)
    y = R.dropout(x, 0.5, mask)
    assert torch.equal(y, torch.where(mask != 0, x * 2.0, torch.zeros(()))) and y.dtype == torch.float32
    assert torch.equal(R.dropout(x, 0.0, torch.ones(1000, dtype=torch.uint8)), x)
    ref = F.dropout(torch.ones(1000, dtype=torch.float64), 0.1, True)
    assert abs(float(R.dropout(torch.ones(1000), 0.1, mask).max()) - float(ref.max())) <= 2.0 ** -23 * 1.2


# windows of the fused resize + cross-entropy kernel (source rows a 16-row output tile reads), from the fp32 index rule
WINDOWS = {(1, 4): 2, (33, 129): 6, (129, 513): 6, (9, 33): 6, (5, 7): 6, (13, 41): 7, (7, 7): 8, (20, 48): 8, (17, 40): 8,
           (33, 65): 10, (65, 129): 10, (40, 64): 12, (16, 16): 17, (33, 33): 17}


def up_window(h, ho):
    i0, i1, _, _, _ = R.axis_table(h, ho)
    return max(int(i0[min(y0 + 16, ho) - 1]) + 1 - int(i0[y0]) + 1 for y0 in range(0, ho, 16))


def test_fused_ce_window_table_and_query(pkg):
    """The source window from the reference's own index table, and the host query of the library (no GPU: it launches nothing)."""
    lib = pkg._lib.load()
    for (h, ho), win in WINDOWS.items():
        assert up_window(h, ho) == win, (h, ho)
        assert lib.afan_ce2d_upsampled_supported(21, h, h, ho, ho) == int(win <= 8), (h, ho)
        assert lib.afan_ce2d_upsampled_supported(21, 1, h, 4, ho) == int(win <= 8)          # each axis is checked on its own
    assert lib.afan_ce2d_upsampled_supported(33, 33, 33, 129, 129) == 0 and lib.afan_ce2d_upsampled_supported(0, 33, 33, 129, 129) == 0
    assert lib.afan_ce2d_upsampled_supported(21, 40, 31, 17, 23) == 0                       # down-scaling
