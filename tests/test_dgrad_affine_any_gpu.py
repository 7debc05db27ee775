"""The frozen BatchNorm (+ ReLU) backward epilogue on the small-channel and 64 -> 64 weights-in-registers input-gradient kernels
(afan_conv_dgrad_affine_nhwc_bf16 with any_family = 1, ops.conv_dgrad_affine(any_kernel=True)): bit for bit afan_conv_dgrad_nhwc_bf16 followed by
afan_affine_relu_bwd, on an instantiation of its own.  afan_conv_dgrad_affine_nhwc_bf16 keeps to the tiled kernel's shapes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _case(gpu, n, ci, co, h, w, k, st, seed):
    """Operands of the input gradient of a ci -> co convolution (k x k, stride st) on an [n, ci, h, w] input."""
    g = torch.Generator().manual_seed(seed)
    ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
    dy = torch.randn(n, co, ho, wo, generator=g).to(gpu).bfloat16().contiguous(memory_format=CL)
    wt = (torch.randn(ci, co, k, k, generator=g) / (co * k * k) ** 0.5).to(gpu).bfloat16().contiguous(memory_format=CL)
    act = torch.relu(torch.randn(n, ci, h, w, generator=g)).to(gpu).bfloat16().contiguous(memory_format=CL)      # ~half zeros
    coefs = torch.empty(4, ci).uniform_(0.5, 1.5, generator=g).to(gpu)       # alpha = row 2 of a coefficient block, as infer.py passes it
    return dy, wt, act, coefs[2]


def _check(pkg, dy, wt, act, alpha, hw, st, mask, kernel):
    raw = pkg.ops.conv_dgrad(dy, wt, hw, st)
    want, _ = pkg.ops.affine_relu_backward(raw, act if mask else None, alpha, mask)
    with pkg.ops.conv_trace() as tr:
        got = pkg.ops.conv_dgrad_affine(dy, wt, hw, st, alpha, act if mask else None, any_kernel=True)
    assert got is not None and got.stride() == want.stride()
    assert [t["kernel"] for t in tr.records] == [kernel] and tr.records[0]["op"] == "dgrad"
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), float((got.float() - want.float()).abs().max())


# (n, ci, co, h, w, k, stride) of the convolution whose input gradient is taken; the kernel's KK = co / 16 (its reduction)
SMALL = [(2, 16, 16, 32, 32, 3, 1), (2, 32, 32, 16, 16, 3, 1), (2, 16, 32, 32, 32, 3, 2), (3, 32, 64, 16, 16, 3, 2),
         (1, 16, 16, 7, 9, 3, 1), (1, 16, 32, 7, 9, 3, 2), (5, 32, 16, 9, 7, 1, 1)]


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("mask", [True, False])
def test_small_channel_dgrad_affine_epilogue(pkg, gpu, shape, mask):
    n, ci, co, h, w, k, st = shape
    dy, wt, act, alpha = _case(gpu, n, ci, co, h, w, k, st, ci + 3 * co + n + st)
    _check(pkg, dy, wt, act, alpha, (h, w), st, mask, "small_dgrad_aff<%d>" % {16: 1, 32: 2, 64: 4}[co])


@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 16, 8), (3, 16, 16)])
@pytest.mark.parametrize("mask", [True, False])
def test_c64_dgrad_affine_epilogue(pkg, gpu, shape, mask):
    n, h, w = shape
    dy, wt, act, alpha = _case(gpu, n, 64, 64, h, w, 3, 1, 64 + n + h)
    _check(pkg, dy, wt, act, alpha, (h, w), 1, mask, "c64_dgrad_aff")


@pytest.mark.parametrize("shape", [(2, 64, 64, 8, 8, 3, 1), (1, 64, 64, 7, 9, 3, 1), (2, 128, 128, 16, 16, 3, 1)])
def test_tiled_shapes_through_the_any_family_entry_equal_the_existing_export(pkg, gpu, shape):
    """64 -> 64 at 8 x 8 (ResNet-20s' last stage) and at a ragged 7 x 9 are the tiled kernel's, like 128 -> 128 at 16 x 16: the two
    entry points run the same launch, which also equals the two-launch form; without a mask the tiled kernel declines."""
    n, ci, co, h, w, k, st = shape
    dy, wt, act, alpha = _case(gpu, n, ci, co, h, w, k, st, 7 + h)
    raw = pkg.ops.conv_dgrad(dy, wt, (h, w), st)
    want, _ = pkg.ops.affine_relu_backward(raw, act, alpha, True)
    with pkg.ops.conv_trace() as t0:
        old = pkg.ops.conv_dgrad_affine(dy, wt, (h, w), st, alpha, act)
    with pkg.ops.conv_trace() as t1:
        new = pkg.ops.conv_dgrad_affine(dy, wt, (h, w), st, alpha, act, any_kernel=True)
    assert old is not None and new is not None
    assert [t["kernel"] for t in t0.records] == [t["kernel"] for t in t1.records] and len(t1.records) == 1
    assert torch.equal(new.view(torch.int16), old.view(torch.int16)) and torch.equal(new.view(torch.int16), want.view(torch.int16))
    with pkg.ops.conv_trace() as t2:
        assert pkg.ops.conv_dgrad_affine(dy, wt, (h, w), st, alpha, None, any_kernel=True) is None
    assert t2.records == []


@pytest.mark.parametrize("shape", [(2, 16, 16, 32, 32, 3, 1), (2, 16, 32, 32, 32, 3, 2), (2, 64, 64, 32, 32, 3, 1)])
def test_tiled_only_entry_point_still_declines_the_other_kernels(pkg, gpu, shape):
    n, ci, co, h, w, k, st = shape
    dy, wt, act, alpha = _case(gpu, n, ci, co, h, w, k, st, 21)
    with pkg.ops.conv_trace() as tr:
        assert pkg.ops.conv_dgrad_affine(dy, wt, (h, w), st, alpha, act) is None
    assert tr.records == []                                              # nothing launched
    assert pkg.ops.conv_dgrad_affine(dy, wt, (h, w), st, alpha, act, any_kernel=True) is not None
    with pytest.raises(ValueError):
        pkg.ops.conv_dgrad_affine(dy, wt, (h, w), st, alpha, None)


def test_block_output_form_still_declines_the_other_kernels(pkg, gpu):
    """afan_conv_dgrad_dual_nhwc_bf16 is unchanged: the small-channel and 64 -> 64 shapes have no such form."""
    for shape in [(2, 16, 16, 32, 32, 3, 1), (2, 64, 64, 32, 32, 3, 1)]:
        n, ci, co, h, w, k, st = shape
        dy, wt, act, alpha = _case(gpu, n, ci, co, h, w, k, st, 5)
        assert pkg.ops.conv_dgrad_dual(dy, wt, (h, w), st, None, alpha, act) is None
