"""The float64 references of tests/conv_f32_pinned_refs.py (what tests/test_conv_f32_pinned_gpu.py holds the general fp32 convolution
kernels to) checked on the CPU against torch's convolution and autograd in float64, on every row of the table; the wgrad_plan
restatement against values computed by hand; the exact operands checked for exactness; the table's coverage of EXPECTED_VARIANTS."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_f32_pinned_refs as R

IDX = list(range(len(R.CASES)))
ids = lambda i: R.case_id(R.CASES[i])


def _rel(got, ref):
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-300)


def _torch(x, w, b, dy, c):
    x, w = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    y = F.conv2d(x, w, None if b is None else torch.from_numpy(b), c.stride, c.pad, c.dil)
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), x.grad.numpy(), w.grad.numpy()


@pytest.mark.parametrize("idx", IDX, ids=ids)
@pytest.mark.parametrize("kind", ["gauss32", "gauss16"])
def test_references_and_scales_match_torch_float64(idx, kind):
    p, c = R.problem(idx, kind), R.CASES[idx]
    assert p.y.shape == (c.n, c.co) + R.out_hw(c)
    y, dx, dw = _torch(p.x, p.w, p.b, p.dy, c)
    assert _rel(p.y, y) <= 1e-12 and _rel(p.dx, dx) <= 1e-12 and _rel(p.dw, dw) <= 1e-12
    # the scales: the same operation on absolute values, plus |b|
    ys, dxs, dws = _torch(np.abs(p.x), np.abs(p.w), None if p.b is None else np.abs(p.b), np.abs(p.dy), c)
    assert _rel(p.y_s, ys) <= 1e-12 and _rel(p.dx_s, dxs) <= 1e-12 and _rel(p.dw_s, dws) <= 1e-12
    assert (p.y_s >= np.abs(p.y) - 1e-12 * p.y_s).all() and (p.dx_s >= np.abs(p.dx) - 1e-12 * p.dx_s).all() and (p.dw_s >= np.abs(p.dw) - 1e-12 * p.dw_s).all()
    # the product counts: the same operation on ones
    one = lambda a: np.ones_like(a)
    yc, dxc, dwc = _torch(one(p.x), one(p.w), None, one(p.dy), c)
    assert (yc == p.y_cnt[None, None]).all() and (dxc == p.dx_cnt[None, None]).all() and (dwc == p.dw_cnt[None, None]).all()
    # every operand is a value of its storage type
    for a in (p.x, p.w, p.dy):
        assert (a.astype(np.float32).astype(np.float64) == a).all()
        if kind == "gauss16":
            assert (R._bf16_round(a) == a).all() and (torch.from_numpy(a).to(torch.bfloat16).double().numpy() == a).all()
    assert (p.b is None) == (kind == "gauss16")


@pytest.mark.parametrize("idx", IDX, ids=ids)
def test_exact_operands_are_exact_in_fp32_in_any_order(idx):
    p, c = R.problem(idx, "exact"), R.CASES[idx]
    y, dx, dw = _torch(p.x, p.w, p.b, p.dy, c)
    assert (p.y == y).all() and (p.dx == dx).all() and (p.dw == dw).all()
    for a in (p.x, p.w, p.dy):
        assert (a == np.round(a)).all() and np.abs(a).max() <= 2 and (a == 0).mean() > 0.4
    assert (p.b == np.round(p.b)).all() and np.abs(p.b).max() <= 4 and (p.g0 == np.round(p.g0)).all() and np.abs(p.g0).max() <= 4
    # sum |a * b| < 2^24: every partial sum of integers is exact whatever the order, the slices and the accumulate included
    assert p.y_s.max() < 2 ** 24 and p.dx_s.max() < 2 ** 24 and (p.dw_s + np.abs(p.g0)).max() < 2 ** 24
    # |result| <= 256 wherever a bf16 output is compared: integers up to 256 are bf16 values
    assert np.abs(p.y).max() <= 256 and np.abs(p.dx).max() <= 256
    # the operations are not trivial on these operands
    assert np.count_nonzero(p.y) and np.count_nonzero(p.dw) and np.count_nonzero(p.dx)


def test_wgrad_plan_matches_hand_computed_values():
    c = R.CASES[R.PLAN_ROW]
    assert tuple(c) == (2, 33, 35, 4, 16, 3, 1, 1, 1) and R.out_hw(c) == (33, 35)
    # P = 2 * 33 * 35 = 2310 pixels = 144 full K-steps + one of 6 pixels; one 32 x 128 tile (co 16, 36 columns): 1024 slices wanted,
    # 145 / 8 = 18 allowed, 9 steps each -> 17 slices, the last of 145 - 16 * 9 = 1 step
    assert R.wgrad_plan(2310, 16, 36) == (32, 17, 9)
    assert 2310 - 144 * R.BK == 6 and 145 - 16 * 9 == 1
    assert R.workspace_floats(c) == 17 * 16 * 36
    # the stem row: P = 70, 5 steps: one slice.  The linear layer as a weight gradient: P = 300, 19 steps, 19 / 8 = 2 slices of 10 and 9
    # steps, the last step of 300 - 288 = 12 pixels.  The cap: P = 32768, 2048 steps, 2048 / 8 = 256 slices of 8.
    assert R.wgrad_plan(70, 16, 27) == (32, 1, 5)
    assert R.wgrad_plan(300, 21, 5) == (32, 2, 10)
    assert R.wgrad_plan(32768, 16, 27) == (32, 256, 8)
    # past the cap: 4096 steps -> 256 slices of 16; more tiles than the target: 136 x 1152 = 2 x 9 tiles, 1024 / 18 -> 57 wanted
    assert R.wgrad_plan(65536, 16, 27) == (32, 256, 16)
    assert R.wgrad_plan(16 * 8 * 57, 136, 1152) == (128, 57, 8)
    assert R.wgrad_plan(16 * 800, 136, 1152) == (128, 54, 15)          # 800 steps: ceil(800 / 57) = 15 per slice, ceil(800 / 15) = 54 slices
    assert R.wgrad_plan(40, 40, 72) == (64, 1, 3)
    # every row of the table: one slice, a last slice shorter than the others, a last step with fewer than 16 pixels, 256 slices and
    # both loops of the reduction (eight slices at a time, then one at a time) are all present
    plans = {}
    for c in R.CASES:
        ho, wo = R.out_hw(c)
        plans[c] = (c.n * ho * wo,) + R.wgrad_plan(c.n * ho * wo, c.co, c.k * c.k * c.ci)
    assert any(sl == 1 for _, _, sl, _ in plans.values())
    assert any(sl == R.WG_MAX_SLICES for _, _, sl, _ in plans.values())
    assert any(sl > 1 and -(-P // R.BK) % sps for P, _, sl, sps in plans.values())
    assert any(P % R.BK for P, _, _, _ in plans.values())
    assert any(sl >= 8 and sl % 8 for _, _, sl, _ in plans.values())
    assert {bm for _, bm, _, _ in plans.values()} == {32, 64, 128}


def test_dispatch_restatement_on_known_calls():
    stem, lin = R.CASES[0], R.CASES[9]
    # 3 channels: nothing is a vector in any layout
    assert R.variant_of(stem, "fwd", R.F32, R.NHWC, R.NHWC, 0) == {"conv_f32_kernel<f32,32,A scalar,B scalar>", "conv_f32_kernel<f32>|a_rows=0",
                                                                 "conv_f32_kernel<f32,32>|b_rows=0"}
    # the stem's input gradient in bf16: dy has 16 channels (vectors), the output tile is ci = 3 wide
    assert R.variant_of(stem, "dgrad", R.BF16, R.NHWC, R.NHWC, 0) == {"conv_f32_kernel<bf16,32,A vec,B scalar>", "conv_f32_kernel<bf16,32>|b_rows=1"}
    assert "conv_f32_kernel<bf16>|a_rows=1" in R.variant_of(stem, "dgrad", R.BF16, R.NCHW, R.NHWC, 0)
    # a 1x1 in KCRS memory is KRSC memory: B stays a vector; a 1-pixel NCHW map has unit channel stride but sH = 1: A is scalar
    assert R.variant_of(lin, "fwd", R.F32, R.NHWC, R.NCHW, 0) == {"conv_f32_kernel<f32,32,A vec,B vec>"}
    assert "conv_f32_kernel<f32,32,A scalar,B vec>" in R.variant_of(lin, "fwd", R.F32, R.NCHW, R.NCHW, 0)
    assert "conv_f32_kernel<f32,64,A vec,B scalar>" in R.variant_of(R.CASES[1], "fwd", R.F32, R.NHWC, R.NCHW, 0)
    # one element late: no vectors
    assert "conv_f32_kernel<f32,64,A scalar,B vec>" in R.variant_of(R.CASES[1], "fwd", R.F32, R.NHWC, R.NHWC, 1)
    assert R.variant_of(R.CASES[2], "wgrad", R.BF16, R.NHWC, R.NHWC, 2, 1) == {"wgrad_f32_kernel<bf16,128,A scalar,B vec>", "wgrad_f32_kernel<bf16,128>|a_k=0",
                                                                             "wgrad_f32_reduce_kernel|accumulate=1"}


def test_table_reaches_every_instantiation():
    """Pure Python: every call the GPU test makes mapped to the kernels it launches by the restated dispatch.  The set must be exactly
    EXPECTED_VARIANTS: the 24 forward / input-gradient and the 24 weight-gradient instantiations, each scalar staging mode under both
    values of its lane flag, the reduction with accumulate 0 and 1."""
    got = R.table_variants()
    assert len(R.EXPECTED_VARIANTS) == 24 + 4 + 12 + 24 + 12 + 4 + 2
    assert sorted(got) == R.EXPECTED_VARIANTS, f"missing {sorted(set(R.EXPECTED_VARIANTS) - got)}, unexpected {sorted(got - set(R.EXPECTED_VARIANTS))}"
    assert max(c.k * c.k for c in R.CASES) == R.MAXT
