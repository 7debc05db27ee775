"""Implicit-GEMM MFMA convolutions (afan_conv_*_nhwc_bf16) against torch's convolution on the same bf16 values."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [  # n, ci, co, h, k, stride
    (4, 64, 64, 32, 3, 1), (3, 64, 128, 32, 3, 2), (2, 128, 128, 16, 3, 1), (2, 64, 128, 32, 1, 2),
    (5, 128, 256, 16, 3, 2), (2, 256, 256, 8, 3, 1), (2, 256, 512, 8, 3, 2), (3, 512, 512, 4, 3, 1),
    (2, 256, 512, 8, 1, 2), (1, 64, 64, 7, 3, 1), (2, 64, 64, 9, 3, 2), (1, 128, 64, 5, 1, 1), (64, 128, 128, 16, 3, 1),
    # the weights-in-registers kernel (afan_conv_c64.hip): W in {32, 16, 8, 4}, one and several tiles per workgroup
    (1, 64, 64, 32, 3, 1), (3, 64, 64, 16, 3, 1), (5, 64, 64, 8, 3, 1), (32, 64, 64, 4, 3, 1), (160, 64, 64, 32, 3, 1),
    # the launches of the training step itself: the 256-row producer-wave tile (16x16 stage), the deep 128- and 64-row
    # pipelines (8x8, 4x4 stages), one and several images per tile
    (256, 128, 128, 16, 3, 1), (256, 256, 256, 8, 3, 1), (256, 512, 512, 4, 3, 1), (8, 128, 256, 16, 3, 1), (6, 256, 128, 8, 3, 1),
    # the small-channel kernel (afan_conv_small.hip): the reference's 16-32-64-channel CIFAR ResNets
    (4, 16, 16, 32, 3, 1), (3, 16, 32, 32, 3, 2), (5, 32, 32, 16, 3, 1), (2, 32, 64, 16, 3, 2), (1, 16, 16, 7, 3, 1),
    (2, 32, 64, 9, 3, 2), (130, 16, 16, 32, 3, 1), (2, 64, 32, 8, 3, 1), (2, 16, 32, 8, 1, 2),
]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("n,ci,co,h,k,stride", CASES)
def test_conv_fwd_and_dgrad_match_torch(pkg, gpu, n, ci, co, h, k, stride):
    torch.manual_seed(n * 1000 + ci + co + h + k + stride)
    x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    w = _cl((torch.randn(co, ci, k, k, device=gpu) / (ci * k * k) ** 0.5).bfloat16())
    assert pkg.ops.conv_supported(ci, co, k, stride)
    y = pkg.ops.conv_fwd(x, w, stride)
    ref = F.conv2d(x.float(), w.float(), None, stride, k // 2)          # fp32 reference on the same bf16 values
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    # one bf16 rounding of an fp32-accumulated sum: |err| <= 2^-8 |ref| + accumulation noise
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.cpu().numpy(), rtol=1e-2, atol=1e-2)
    dy = _cl(torch.randn_like(ref).bfloat16())
    wt = _cl(w.permute(1, 0, 2, 3))
    dx = pkg.ops.conv_dgrad(dy, wt, (h, h), stride)
    dref = torch.ops.aten.convolution_backward(dy.float(), x.float(), w.float(), None, (stride, stride), (k // 2, k // 2),
                                               (1, 1), False, (0, 0), 1, [True, False, False])[0]
    assert dx.shape == dref.shape
    scale = float(dref.abs().max())
    np.testing.assert_allclose(dx.float().cpu().numpy(), dref.cpu().numpy(), rtol=1e-2, atol=1e-2 * max(scale, 1.0))


def test_conv_identity_kernel_is_exact(pkg, gpu):
    """A = I check with an asymmetric pattern: a centre-tap identity 3x3 kernel must return the input bit for bit,
    and a one-pixel-shift kernel the shifted input with zero padding (catches row/col or tap-order swaps)."""
    x = _cl(torch.randn(2, 64, 6, 6, device=gpu).bfloat16())
    w = torch.zeros(64, 64, 3, 3, device=gpu)
    w[torch.arange(64), torch.arange(64), 1, 1] = 1.0
    y = pkg.ops.conv_fwd(x, _cl(w.bfloat16()), 1)
    assert torch.equal(y, x)
    w = torch.zeros(64, 64, 3, 3, device=gpu)
    w[torch.arange(64), (torch.arange(64) + 1) % 64, 0, 2] = 1.0     # out c <- in c+1 at (h-1, w+1)
    y = pkg.ops.conv_fwd(x, _cl(w.bfloat16()), 1)
    ref = torch.zeros_like(x)
    ref[:, :, 1:, :-1] = x[:, :, :-1, 1:].roll(-1, dims=1)
    assert torch.equal(y, ref)


def test_conv_rejects_unsupported(pkg, gpu):
    assert not pkg.ops.conv_supported(3, 48, 3, 1) and not pkg.ops.conv_supported(3, 64, 3, 2)
    assert not pkg.ops.conv_supported(24, 64, 3, 1)
    x = _cl(torch.randn(1, 3, 8, 8, device=gpu).bfloat16())        # stem kernel: image width must be a multiple of 32
    w = _cl(torch.randn(64, 3, 3, 3, device=gpu).bfloat16())
    with pytest.raises(pkg.AfanLibraryError):
        pkg.ops.conv_fwd(x, w, 1)
    x = _cl(torch.randn(1, 24, 8, 8, device=gpu).bfloat16())
    w = _cl(torch.randn(64, 24, 3, 3, device=gpu).bfloat16())
    with pytest.raises(pkg.AfanLibraryError):
        pkg.ops.conv_fwd(x, w, 1)


STEM = [  # n, co, h, w   (afan_conv_stem.hip: 3 image channels, 3x3, stride 1)
    (4, 64, 32, 32), (3, 16, 32, 32), (5, 32, 8, 64), (1, 64, 1, 32), (2, 64, 5, 96), (256, 64, 32, 32), (130, 16, 32, 32),
]


@pytest.mark.parametrize("n,co,h,w", STEM)
def test_stem_forward_moments_and_wgrad(pkg, gpu, bn_mode, n, co, h, w):
    torch.manual_seed(n + co + h + w)
    assert pkg.ops.conv_supported(3, co, 3, 1) and pkg.ops.conv_wgrad_supported(3, co, 3, 1, (n, h, w))
    x = _cl(torch.randn(n, 3, h, w, device=gpu).bfloat16())
    wt = _cl((torch.randn(co, 3, 3, 3, device=gpu) / 27 ** 0.5).bfloat16())
    y = pkg.ops.conv_fwd(x, wt, 1)
    ref = F.conv2d(x.float(), wt.float(), None, 1, 1)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    # 27 products of bf16 values summed in fp32, one bf16 rounding (an ulp where the fp32 sums straddle a tie)
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.cpu().numpy(), rtol=1e-2, atol=1e-3)
    # moments for the following train-mode BatchNorm (accumulator form; the slab mode lets BatchNorm reduce itself)
    shift = torch.randn(co, device=gpu) * 0.1
    y2, st = pkg.ops.conv_fwd(x, wt, 1, stats_shift=shift, want_stats=True)
    assert torch.equal(y2, y)
    if bn_mode == "acc":
        assert st is not None and st.acc is not None
        gamma, beta = torch.rand(co, device=gpu) + 0.5, torch.randn(co, device=gpu)
        outs = []
        for cs in (None, st):
            rm, rv = shift.clone(), torch.ones(co, device=gpu)
            nbt = torch.zeros((), dtype=torch.int64, device=gpu)
            o, stats = pkg.ops.bn_train_forward(y, gamma, beta, None, True, 1e-5, 0.1, rm, rv, nbt, cs)
            outs.append((o.float().cpu().numpy(), stats.cpu().numpy(), rm.cpu().numpy(), rv.cpu().numpy()))
        a, b = outs
        np.testing.assert_allclose(b[1][:2], a[1][:2], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(b[2], a[2], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(b[3], a[3], rtol=2e-5)
        np.testing.assert_allclose(b[0], a[0], rtol=1e-2, atol=1e-2)
    else:
        assert st is None
    # weight gradient
    dy = _cl((torch.randn(n, co, h, w, device=gpu) / (n * h * w) ** 0.5).bfloat16())
    gref = torch.ops.aten.convolution_backward(dy.float(), x.float(), torch.zeros(co, 3, 3, 3, device=gpu), None, (1, 1),
                                               (1, 1), (1, 1), False, (0, 0), 1, [False, True, False])[1]
    g = pkg.ops.conv_wgrad(x, dy, 3, 1)
    assert g.shape == gref.shape and g.dtype == torch.float32
    scale = float(gref.abs().max())
    np.testing.assert_allclose(g.cpu().numpy(), gref.cpu().numpy(), rtol=2e-3, atol=2e-3 * scale)
    acc = torch.ones((co, 3, 3, 3), device=gpu).contiguous(memory_format=torch.channels_last)
    pkg.ops.conv_wgrad(x, dy, 3, 1, acc, accumulate=True)
    pkg.ops.conv_wgrad(x, dy, 3, 1, acc, accumulate=True)
    np.testing.assert_allclose(acc.cpu().numpy(), 1 + 2 * gref.cpu().numpy(), rtol=2e-3, atol=4e-3 * scale)
    assert torch.equal(pkg.ops.conv_wgrad(x, dy, 3, 1), g)          # fixed summation order


def test_stem_shift_kernel_is_exact(pkg, gpu):
    """Tap / channel order: a kernel that copies input channel c of the pixel at (h-1, w+1) into output channel c."""
    x = _cl(torch.randn(2, 3, 4, 32, device=gpu).bfloat16())
    w = torch.zeros(16, 3, 3, 3, device=gpu)
    w[torch.arange(3), torch.arange(3), 0, 2] = 1.0
    y = pkg.ops.conv_fwd(x, _cl(w.bfloat16()), 1)
    ref = torch.zeros(2, 16, 4, 32, device=gpu, dtype=torch.bfloat16)
    ref[:, :3, 1:, :-1] = x[:, :, :-1, 1:]
    assert torch.equal(y, _cl(ref))


@pytest.mark.parametrize("n,ci,co,h,k,stride", [(4, 64, 64, 32, 3, 1), (3, 64, 128, 32, 3, 2), (2, 256, 512, 8, 1, 2),
                                                 (64, 128, 128, 16, 3, 1), (1, 64, 64, 7, 3, 1),
                                                 (256, 256, 256, 8, 3, 1), (256, 512, 512, 4, 3, 1),    # deep-pipeline launches
                                                 (256, 128, 128, 16, 3, 1)])
def test_conv_epilogue_moments_feed_batchnorm(pkg, gpu, bn_mode, n, ci, co, h, k, stride):
    """conv (+ epilogue moment partials) -> BN(train) must equal conv -> stand-alone BN on the stored bf16 tensor."""
    torch.manual_seed(ci + co + h)
    x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    w = _cl((torch.randn(co, ci, k, k, device=gpu) / (ci * k * k) ** 0.5).bfloat16())
    shift = torch.randn(co, device=gpu) * 0.1
    y, st = pkg.ops.conv_fwd(x, w, stride, stats_shift=shift, want_stats=True)
    y_plain = pkg.ops.conv_fwd(x, w, stride)
    assert torch.equal(y, y_plain) and ((st.acc is not None) if bn_mode == "acc" else st.g >= 1)
    gamma, beta = torch.rand(co, device=gpu) + 0.5, torch.randn(co, device=gpu)
    outs = []
    for cs in (None, st):
        rm, rv = shift.clone(), torch.ones(co, device=gpu)
        nbt = torch.zeros((), dtype=torch.int64, device=gpu)
        o, stats = pkg.ops.bn_train_forward(y, gamma, beta, None, True, 1e-5, 0.1, rm, rv, nbt, cs)
        outs.append((o.float().cpu().numpy(), stats.cpu().numpy(), rm.cpu().numpy(), rv.cpu().numpy(), int(nbt)))
    a, b = outs
    np.testing.assert_allclose(b[1][:2], a[1][:2], rtol=2e-5, atol=2e-6)     # mean, invstd
    np.testing.assert_allclose(b[2], a[2], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(b[3], a[3], rtol=2e-5)
    np.testing.assert_allclose(b[0], a[0], rtol=1e-2, atol=1e-2)
    assert a[4] == b[4] == 1


SMALL_WGRAD = [  # afan_wgrad_small.hip: every 16/32-channel 3x3 layer of ResNet-20s / 56s, and more tile geometries
    (128, 16, 16, 32, 3, 1), (128, 16, 32, 32, 3, 2), (128, 32, 32, 16, 3, 1), (128, 32, 64, 16, 3, 2), (3, 32, 32, 8, 3, 1),
    (2, 16, 16, 64, 3, 1), (1, 32, 16, 16, 3, 1), (5, 16, 64, 32, 3, 2), (300, 16, 16, 32, 3, 1),
]


def test_small_wgrad_cases_are_taken_by_the_library(pkg, gpu):
    for n, ci, co, h, k, stride in SMALL_WGRAD:
        assert pkg.ops.conv_wgrad_supported(ci, co, k, stride, (n, h, h)), (n, ci, co, h, k, stride)
    assert not pkg.ops.conv_wgrad_supported(16, 16, 3, 1, (2, 7, 7)) and not pkg.ops.conv_wgrad_supported(16, 32, 1, 2, (2, 8, 8))
    assert not pkg.ops.conv_wgrad_supported(16, 16, 3, 1)          # no spatial size given: only the 64-multiple rule


@pytest.mark.parametrize("n,ci,co,h,k,stride", CASES + [(256, 128, 128, 16, 3, 1), (7, 64, 64, 5, 3, 1)] + SMALL_WGRAD)
def test_conv_wgrad_matches_torch(pkg, gpu, n, ci, co, h, k, stride):
    torch.manual_seed(n + ci + co + h + k + stride)
    x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    ho = (h + 2 * (k // 2) - k) // stride + 1
    dy = _cl((torch.randn(n, co, ho, ho, device=gpu) / (n * ho * ho) ** 0.5).bfloat16())
    w = torch.zeros(co, ci, k, k, device=gpu)
    ref = torch.ops.aten.convolution_backward(dy.float(), x.float(), w, None, (stride, stride), (k // 2, k // 2), (1, 1),
                                              False, (0, 0), 1, [False, True, False])[1]
    if not pkg.ops.conv_wgrad_supported(ci, co, k, stride, (n, h, h)):   # odd sizes / 1x1 of the small-channel layers: vendor library
        with pytest.raises(pkg.AfanLibraryError):
            pkg.ops.conv_wgrad(x, dy, k, stride)
        return
    g = pkg.ops.conv_wgrad(x, dy, k, stride)
    assert g.shape == ref.shape and g.dtype == torch.float32
    scale = float(ref.abs().max())
    np.testing.assert_allclose(g.cpu().numpy(), ref.cpu().numpy(), rtol=2e-3, atol=2e-3 * scale)   # fp32 accumulation both sides
    # accumulate into an existing KRSC buffer (the arena's gradient view), twice: the two branches of the joint loss
    acc = torch.ones((co, ci, k, k), device=gpu).contiguous(memory_format=torch.channels_last)
    pkg.ops.conv_wgrad(x, dy, k, stride, acc, accumulate=True)
    pkg.ops.conv_wgrad(x, dy, k, stride, acc, accumulate=True)
    np.testing.assert_allclose(acc.cpu().numpy(), 1 + 2 * ref.cpu().numpy(), rtol=2e-3, atol=4e-3 * scale)
    # bitwise reproducible (deterministic slice order, no atomics)
    assert torch.equal(pkg.ops.conv_wgrad(x, dy, k, stride), g)


@pytest.mark.parametrize("n,ci,co,h,k,stride", [(4, 64, 64, 32, 3, 1), (3, 64, 128, 32, 3, 2), (2, 128, 256, 16, 1, 2),
                                                 (64, 128, 128, 16, 3, 1), (3, 256, 512, 9, 3, 2),
                                                 (256, 128, 128, 16, 3, 1), (128, 256, 256, 8, 3, 1)])     # 256-row / deep-pipeline launches
def test_dgrad_epilogue_fusions(pkg, gpu, bn_mode, n, ci, co, h, k, stride):
    """dgrad + addend == dgrad then add; dgrad's fused BN-backward partials == the stand-alone reduction pass."""
    torch.manual_seed(ci + co + h + k)
    ho = (h + 2 * (k // 2) - k) // stride + 1
    dy = _cl(torch.randn(n, co, ho, ho, device=gpu).bfloat16())
    w = _cl((torch.randn(co, ci, k, k, device=gpu) / (co * k * k) ** 0.5).bfloat16())
    wt = _cl(w.permute(1, 0, 2, 3))
    plain = pkg.ops.conv_dgrad(dy, wt, (h, h), stride)
    addend = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    fused = pkg.ops.conv_dgrad(dy, wt, (h, h), stride, addend=addend)
    assert torch.equal(fused, plain + addend)                       # same fp32 add + one bf16 rounding
    # a BN(+ReLU) whose input was bn_x; its backward receives `plain` as dy
    bn_x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    gamma, beta = torch.rand(ci, device=gpu) + 0.5, torch.randn(ci, device=gpu) * 0.3
    for relu in (True, False):
        y, stats = pkg.ops.bn_train_forward(bn_x, gamma, beta, None, relu, 1e-5, 0.1, None, None, None)
        dx2, st = pkg.ops.conv_dgrad(dy, wt, (h, h), stride, bn_bwd=(bn_x, stats, relu))
        assert torch.equal(dx2, plain)
        outs = []
        for partials in (None, st):
            dwb = torch.zeros(2, ci, device=gpu)
            dxb, _ = pkg.ops.bn_backward(plain, bn_x, None, stats, gamma, beta, relu, False, dwb[0], dwb[1], partials=partials)
            outs.append((dxb.float().cpu().numpy(), dwb.cpu().numpy()))
        scale = max(1.0, float(np.abs(outs[0][1]).max()))
        np.testing.assert_allclose(outs[1][1], outs[0][1], rtol=2e-4, atol=2e-4 * scale)      # dweight, dbias
        np.testing.assert_allclose(outs[1][0], outs[0][0], rtol=2e-2, atol=2e-3 * max(1.0, float(np.abs(outs[0][0]).max())))
    # a BN whose ReLU follows a residual add (a BasicBlock's bn2): the mask comes from the stored output, bn_y > 0
    res = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    y, stats = pkg.ops.bn_train_forward(bn_x, gamma, beta, res, True, 1e-5, 0.1, None, None, None)
    dx3, st = pkg.ops.conv_dgrad(dy, wt, (h, h), stride, addend=addend, bn_bwd=(bn_x, stats, True), bn_y=y)
    assert torch.equal(dx3, fused)
    outs = []
    for partials in (None, st):
        dwb = torch.zeros(2, ci, device=gpu)
        dxb, dres = pkg.ops.bn_backward(fused, bn_x, y, stats, gamma, beta, True, True, dwb[0], dwb[1], partials=partials)
        outs.append((dxb.float().cpu().numpy(), dwb.cpu().numpy(), dres.float().cpu().numpy()))
    scale = max(1.0, float(np.abs(outs[0][1]).max()))
    np.testing.assert_allclose(outs[1][1], outs[0][1], rtol=2e-4, atol=2e-4 * scale)
    np.testing.assert_allclose(outs[1][0], outs[0][0], rtol=2e-2, atol=2e-3 * max(1.0, float(np.abs(outs[0][0]).max())))
    np.testing.assert_array_equal(outs[1][2], outs[0][2])


@pytest.mark.parametrize("n,ci,co,h,w", [(2, 256, 256, 33, 33), (3, 128, 256, 19, 19), (5, 64, 128, 7, 7), (9, 128, 128, 4, 4),
                                         (2, 192, 128, 13, 29), (1, 64, 256, 5, 61), (64, 512, 512, 7, 7),
                                         # 385..768 workgroups of 128 rows: the 256-row halo tile (a whole 16x16 image per tile)
                                         (256, 128, 128, 16, 16), (100, 128, 256, 16, 16), (150, 64, 128, 8, 40), (37, 128, 128, 15, 17),
                                         # weight-heavy launches (Ci >= 256): 128-row x 64-channel and 256-row x 64-channel halo tiles
                                         (256, 512, 512, 4, 4), (256, 256, 256, 8, 8), (200, 512, 256, 8, 8), (30, 256, 192, 9, 11)])
def test_halo_form_equals_per_tap_form(pkg, gpu, n, ci, co, h, w):
    """The LDS-resident-halo form of the tiled kernel (launches of about one workgroup per CU: 3x3 / stride 1, whole
    64-channel chunks) against (a) torch on the same bf16 values and (b) the per-tap form bit for bit: the same images
    inside a batch repeated until the launch has more than 768 workgroups take the per-tap form, and both forms add an
    output's products in one order.  Odd widths, tiles that straddle image rows and images, ragged last tiles."""
    torch.manual_seed(n + ci + co + h + w)
    x = _cl(torch.randn(n, ci, h, w, device=gpu).bfloat16())
    wgt = _cl((torch.randn(co, ci, 3, 3, device=gpu) / (ci * 9) ** 0.5).bfloat16())
    y = pkg.ops.conv_fwd(x, wgt, 1)
    ref = F.conv2d(x.float(), wgt.float(), None, 1, 1)
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.cpu().numpy(), rtol=1e-2, atol=1e-2)
    rep = 1
    while ((n * rep * h * w + 127) // 128) * (co // 128) <= 768:
        rep += 1
    xb = _cl(x.repeat(rep, 1, 1, 1))
    yb = pkg.ops.conv_fwd(xb, wgt, 1)
    for r in (0, rep // 2, rep - 1):
        assert torch.equal(yb[r * n:(r + 1) * n], y)
    dy = _cl(torch.randn(n, co, h, w, device=gpu).bfloat16())
    wt = _cl(wgt.permute(1, 0, 2, 3))
    dx = pkg.ops.conv_dgrad(dy, wt, (h, w), 1)
    refd = torch.nn.grad.conv2d_input((n, ci, h, w), wgt.float(), dy.float(), padding=1)
    np.testing.assert_allclose(dx.float().cpu().numpy(), refd.cpu().numpy(), rtol=1e-2, atol=2e-2)
    if ci % 128 == 0:                                  # (the gradient's GEMM has ci output channels: tiled kernel, 128-wide)
        rep = 1
        while ((n * rep * h * w + 127) // 128) * (ci // 128) <= 768:
            rep += 1
        dxb = pkg.ops.conv_dgrad(_cl(dy.repeat(rep, 1, 1, 1)), wt, (h, w), 1)
        for r in (0, rep - 1):
            assert torch.equal(dxb[r * n:(r + 1) * n], dx)


@pytest.mark.parametrize("n,ci,co,h,k,stride", [(8, 64, 128, 16, 3, 2), (16, 128, 128, 8, 3, 1), (64, 256, 512, 4, 1, 2),
                                                 (32, 256, 256, 8, 3, 1), (64, 512, 512, 4, 3, 1), (256, 128, 128, 16, 3, 1),
                                                 # half-batches that are NOT a whole number of row tiles (DeepLab's 33 x 33 maps at
                                                 # 2 + 2 images, one image per half, a stride-2 launch's parity classes): the one
                                                 # tile that holds rows of both halves sums per row
                                                 (4, 256, 256, 33, 3, 1), (4, 1024, 256, 33, 1, 1), (2, 256, 1024, 33, 1, 1),
                                                 (6, 64, 128, 18, 3, 2), (2, 512, 512, 7, 3, 1)])
def test_grouped_statistics_equal_separate_launches(pkg, gpu, n, ci, co, h, k, stride):
    """groups = 2 (two concatenated half-batches, BatchNorm statistics per half): one launch over [a | b] must equal the
    two launches over a and over b — outputs bit for bit (row tiles are independent), sums to accumulation-order noise."""
    torch.manual_seed(n + ci + co + h)
    ops = pkg.ops
    x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    w = _cl((torch.randn(co, ci, k, k, device=gpu) / (ci * k * k) ** 0.5).bfloat16())
    shift = torch.randn(co, device=gpu) * 0.1
    gamma, beta = torch.rand(co, device=gpu) + 0.5, torch.randn(co, device=gpu) * 0.2
    hb = n // 2
    y, st = ops.conv_fwd(x, w, stride, stats_shift=shift, want_stats=True, groups=2)
    outs, stats = [], []
    for g in range(2):
        xs = x[g * hb:(g + 1) * hb]
        ys, sts = ops.conv_fwd(xs, w, stride, stats_shift=shift, want_stats=True)
        assert torch.equal(ys, y[g * hb:(g + 1) * hb])
        o_ref, s_ref = ops.bn_train_forward(ys, gamma, beta, None, True, 1e-5, 0.1, None, None, None, sts)
        o_grp, s_grp = ops.bn_train_forward(y[g * hb:(g + 1) * hb], gamma, beta, None, True, 1e-5, 0.1, None, None, None,
                                            st.group(g, co))
        np.testing.assert_allclose(s_grp.cpu().numpy(), s_ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
        assert_close = np.testing.assert_allclose
        assert_close(o_grp.float().cpu().numpy(), o_ref.float().cpu().numpy(), rtol=1e-2, atol=1e-2)
        outs.append(o_ref)
        stats.append(s_ref)
    # ONE BatchNorm launch over both halves (gridDim.y = groups): per-half statistics, running stats updated half by half
    rm1, rv1, nb1 = shift.clone(), torch.ones(co, device=gpu), torch.zeros((), dtype=torch.int64, device=gpu)
    o_all, s_all = ops.bn_train_forward(y, gamma, beta, None, True, 1e-5, 0.1, rm1, rv1, nb1, st, groups=2)
    rm2, rv2, nb2 = shift.clone(), torch.ones(co, device=gpu), torch.zeros((), dtype=torch.int64, device=gpu)
    for g in range(2):
        o_h, s_h = ops.bn_train_forward(y[g * hb:(g + 1) * hb], gamma, beta, None, True, 1e-5, 0.1, rm2, rv2, nb2,
                                        st.group(g, co))
        np.testing.assert_array_equal(s_all[g].cpu().numpy(), s_h.cpu().numpy())
        assert torch.equal(o_all[g * hb:(g + 1) * hb], o_h)
    np.testing.assert_allclose(rm1.cpu().numpy(), rm2.cpu().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(rv1.cpu().numpy(), rv2.cpu().numpy(), rtol=1e-6, atol=1e-7)
    assert int(nb1) == int(nb2) == 2
    # dgrad with the BN-backward sums of a BatchNorm over dx's tensor (ci channels), per group
    ho = y.shape[2]
    dy = _cl(torch.randn(n, co, ho, ho, device=gpu).bfloat16())
    wt = _cl(w.permute(1, 0, 2, 3))
    bn_x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    g2, b2 = torch.rand(ci, device=gpu) + 0.5, torch.randn(ci, device=gpu) * 0.2
    st2 = torch.stack([ops.bn_train_forward(bn_x[g * hb:(g + 1) * hb], g2, b2, None, True, 1e-5, 0.1, None, None, None)[1]
                       for g in range(2)])
    dx, part = ops.conv_dgrad(dy, wt, (h, h), stride, bn_bwd=(bn_x, st2, True), groups=2)
    for g in range(2):
        sl = slice(g * hb, (g + 1) * hb)
        dxs, parts = ops.conv_dgrad(dy[sl], wt, (h, h), stride, bn_bwd=(bn_x[sl], st2[g], True))
        assert torch.equal(dxs, dx[sl])
        res = []
        for p_ in (parts, part.group(g, ci)):
            dwb = torch.zeros(2, ci, device=gpu)
            d_, _ = ops.bn_backward(dxs, bn_x[sl], None, st2[g], g2, b2, True, False, dwb[0], dwb[1], partials=p_)
            res.append((d_.float().cpu().numpy(), dwb.cpu().numpy()))
        scale = max(1.0, float(np.abs(res[0][1]).max()))
        np.testing.assert_allclose(res[1][1], res[0][1], rtol=1e-5, atol=1e-5 * scale)
        np.testing.assert_allclose(res[1][0], res[0][0], rtol=1e-2, atol=1e-3 * max(1.0, float(np.abs(res[0][0]).max())))
    # one grouped BatchNorm-backward launch against the two per-half launches
    dwb_a, dwb_b = torch.zeros(2, ci, device=gpu), torch.zeros(2, ci, device=gpu)
    d_all, _ = ops.bn_backward(dx, bn_x, None, st2, g2, b2, True, False, dwb_a[0], dwb_a[1], True, partials=part, groups=2)
    for g in range(2):
        sl = slice(g * hb, (g + 1) * hb)
        d_h, _ = ops.bn_backward(dx[sl], bn_x[sl], None, st2[g], g2, b2, True, False, dwb_b[0], dwb_b[1], True,
                                 partials=part.group(g, ci))
        assert torch.equal(d_all[sl], d_h)
    np.testing.assert_allclose(dwb_a.cpu().numpy(), dwb_b.cpu().numpy(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n,ci,co,h,k,stride", [(8, 16, 16, 32, 3, 1), (6, 16, 32, 32, 3, 2), (8, 32, 32, 16, 3, 1),
                                                 (4, 32, 64, 16, 3, 2), (3, 16, 16, 9, 3, 1)])
def test_small_channel_epilogue_fusions(pkg, gpu, n, ci, co, h, k, stride):
    """afan_conv_small.hip: BN moments in the forward epilogue, addend / BN-backward sums (both mask forms) in the dgrad
    epilogue, and image groups — against the stand-alone kernels on the same tensors."""
    torch.manual_seed(n + ci + co + h)
    ops = pkg.ops
    x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    w = _cl((torch.randn(co, ci, k, k, device=gpu) / (ci * k * k) ** 0.5).bfloat16())
    shift = torch.randn(co, device=gpu) * 0.1
    gamma, beta = torch.rand(co, device=gpu) + 0.5, torch.randn(co, device=gpu) * 0.2
    y, st = ops.conv_fwd(x, w, stride, stats_shift=shift, want_stats=True)
    assert torch.equal(y, ops.conv_fwd(x, w, stride)) and st.acc is not None
    o1, s1 = ops.bn_train_forward(y, gamma, beta, None, True, 1e-5, 0.1, None, None, None, st)
    o0, s0 = ops.bn_train_forward(y, gamma, beta, None, True, 1e-5, 0.1, None, None, None)
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(o1.float().cpu().numpy(), o0.float().cpu().numpy(), rtol=1e-2, atol=1e-2)
    ho = y.shape[2]
    dy = _cl(torch.randn(n, co, ho, ho, device=gpu).bfloat16())
    wt = _cl(w.permute(1, 0, 2, 3))
    plain = ops.conv_dgrad(dy, wt, (h, h), stride)
    addend = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    assert torch.equal(ops.conv_dgrad(dy, wt, (h, h), stride, addend=addend), plain + addend)
    bn_x = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    g2, b2 = torch.rand(ci, device=gpu) + 0.5, torch.randn(ci, device=gpu) * 0.3
    res = _cl(torch.randn(n, ci, h, h, device=gpu).bfloat16())
    for mode in ("recompute", "stored"):
        yb, stats = ops.bn_train_forward(bn_x, g2, b2, res if mode == "stored" else None, True, 1e-5, 0.1, None, None, None)
        kw = dict(bn_y=yb) if mode == "stored" else {}
        dx2, part = ops.conv_dgrad(dy, wt, (h, h), stride, bn_bwd=(bn_x, stats, True), **kw)
        assert torch.equal(dx2, plain)
        outs = []
        for p_ in (None, part):
            dwb = torch.zeros(2, ci, device=gpu)
            d_, _ = ops.bn_backward(plain, bn_x, yb if mode == "stored" else None, stats, g2, b2, True, False, dwb[0],
                                    dwb[1], partials=p_)
            outs.append((d_.float().cpu().numpy(), dwb.cpu().numpy()))
        scale = max(1.0, float(np.abs(outs[0][1]).max()))
        np.testing.assert_allclose(outs[1][1], outs[0][1], rtol=2e-4, atol=2e-4 * scale)
        np.testing.assert_allclose(outs[1][0], outs[0][0], rtol=2e-2, atol=2e-3 * max(1.0, float(np.abs(outs[0][0]).max())))
    # image groups (half-batch statistics), where the half-batch is a whole number of 128-pixel tiles
    if (n // 2) * (ho * ho) % 128 == 0 and n % 2 == 0:
        yg, stg = ops.conv_fwd(x, w, stride, stats_shift=shift, want_stats=True, groups=2)
        assert torch.equal(yg, y)
        hb = n // 2
        for g in range(2):
            ys, sts = ops.conv_fwd(x[g * hb:(g + 1) * hb], w, stride, stats_shift=shift, want_stats=True)
            a = ops.bn_train_forward(ys, gamma, beta, None, True, 1e-5, 0.1, None, None, None, sts)[1]
            b = ops.bn_train_forward(ys, gamma, beta, None, True, 1e-5, 0.1, None, None, None, stg.group(g, co))[1]
            np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("n,n2,ci,co,h,k,stride", [(4, 4, 64, 64, 32, 3, 1), (8, 3, 128, 128, 16, 3, 1), (4, 4, 128, 256, 16, 3, 2),
                                                   (16, 16, 256, 512, 8, 1, 2), (16, 5, 512, 512, 4, 3, 1),
                                                   # the small-channel kernel (ResNet-20s / 56s layers)
                                                   (8, 8, 16, 16, 32, 3, 1), (8, 3, 16, 32, 32, 3, 2), (6, 6, 32, 32, 16, 3, 1),
                                                   (4, 7, 32, 64, 16, 3, 2)])
def test_wgrad_two_operand_pairs_in_one_launch(pkg, gpu, n, n2, ci, co, h, k, stride):
    """afan_conv_wgrad2: grad += wgrad(x, dy) + wgrad(x2, dy2) in one launch (a tail layer's clean and adversarial pass)
    equals the two separate launches; pairs of different batch sizes; first pair's pixel count % 64 == 0."""
    torch.manual_seed(n + n2 + ci + co + h + k)
    ho = (h + 2 * (k // 2) - k) // stride + 1
    mk = lambda b: (_cl(torch.randn(b, ci, h, h, device=gpu).bfloat16()),
                    _cl((torch.randn(b, co, ho, ho, device=gpu) / (b * ho * ho) ** 0.5).bfloat16()))
    (x, dy), (x2, dy2) = mk(n), mk(n2)
    assert pkg.ops.wgrad_pairable(x, dy, k, stride)
    ref = pkg.ops.conv_wgrad(x, dy, k, stride)
    pkg.ops.conv_wgrad(x2, dy2, k, stride, ref, accumulate=True)
    got = pkg.ops.conv_wgrad(x, dy, k, stride, second=(x2, dy2))
    scale = float(ref.abs().max())
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-5 * scale)
    acc = torch.ones_like(ref)
    pkg.ops.conv_wgrad(x, dy, k, stride, acc, accumulate=True, second=(x2, dy2))
    np.testing.assert_allclose(acc.cpu().numpy(), 1 + ref.cpu().numpy(), rtol=1e-4, atol=1e-5 * max(scale, 1.0))
    assert torch.equal(pkg.ops.conv_wgrad(x, dy, k, stride, second=(x2, dy2)), got)      # fixed summation order
    with pytest.raises(pkg.AfanLibraryError):                                            # 3 * 5 * 5 pixels: not a multiple of 64
        xs, dys = _cl(torch.randn(3, 64, 5, 5, device=gpu).bfloat16()), _cl(torch.randn(3, 64, 5, 5, device=gpu).bfloat16())
        pkg.ops.conv_wgrad(xs, dys, 3, 1, second=(xs, dys))


@pytest.mark.parametrize("n,ci,co,h,w", [(4, 64, 128, 32, 32), (2, 128, 256, 16, 16), (3, 256, 512, 8, 8), (2, 64, 128, 14, 10)])
def test_dgrad_with_fused_projection_equals_two_launches(pkg, gpu, n, ci, co, h, w):
    """afan_conv_dgrad_sc_nhwc_bf16: the input gradients of a BasicBlock's 3x3 / stride-2 convolution and of its 1x1 / stride-2
    projection (resnet_s.py:52-77) as ONE launch — the projection is a tenth tap of the even/even parity class, gathered from
    the second tensor of the pair buffer, its weights the tenth slot of the [Ci][10][Co] operand afan_transpose_weights
    builds.  Against the two launches + addend it replaces (same kernels: differences are one bf16 rounding of the
    intermediate sum) and against float64."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(2)
    cl = torch.channels_last
    w1 = (torch.randn(co, ci, 3, 3, generator=g) * 0.05).to(gpu).bfloat16().contiguous(memory_format=cl)
    wsc = (torch.randn(co, ci, 1, 1, generator=g) * 0.1).to(gpu).bfloat16().contiguous(memory_format=cl)
    ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    pair = (torch.randn(2 * n, co, ho, wo, generator=g) * 0.5).to(gpu).bfloat16().contiguous(memory_format=cl)
    dy, dy_sc = pair[:n], pair[n:]
    wt1 = w1.permute(1, 0, 2, 3).contiguous(memory_format=cl)          # [Ci, Co, 3, 3] CRSK memory
    wtsc = wsc.permute(1, 0, 2, 3).contiguous(memory_format=cl)
    # the combined operand, built by the library's transpose kernel from KRSC sources exactly as the arena does
    src = torch.cat([w1.permute(0, 2, 3, 1).reshape(-1), wsc.permute(0, 2, 3, 1).reshape(-1)]).contiguous()
    dst = torch.zeros(ci * 10 * co, dtype=torch.bfloat16, device=gpu)
    t1 = ((co + 63) // 64) * 9 * ((ci + 63) // 64)
    desc = torch.tensor([[0, 0, co, 9, ci, 0, 10, 0], [w1.numel(), 0, co, 1, ci, t1, 10, 9]], dtype=torch.int64, device=gpu)
    ops.transpose_weights(src, dst, desc, 2, t1 + ((co + 63) // 64) * ((ci + 63) // 64))
    ref10 = torch.cat([wt1.permute(0, 2, 3, 1).reshape(ci, 9, co), wtsc.permute(0, 2, 3, 1).reshape(ci, 1, co)], dim=1)
    assert torch.equal(dst.view(ci, 10, co), ref10)
    fused = ops.conv_dgrad(dy, wt1, (h, w), 2, sc=(dy_sc, dst))
    two = ops.conv_dgrad(dy, wt1, (h, w), 2, addend=ops.conv_dgrad(dy_sc, wtsc, (h, w), 2))
    x = torch.zeros(n, ci, h, w, dtype=torch.float64, device=gpu, requires_grad=True)
    y = F.conv2d(x, w1.double(), stride=2, padding=1)
    ysc = F.conv2d(x, wsc.double(), stride=2)
    (gx,) = torch.autograd.grad([y, ysc], x, [dy.double(), dy_sc.double()])
    e_f = float((fused.double() - gx).norm() / gx.norm())
    e_t = float((two.double() - gx).norm() / gx.norm())
    assert e_f < 4e-3 and e_f <= e_t * 1.05 + 1e-6, (e_f, e_t)       # one rounding instead of two
    assert fused.is_contiguous(memory_format=cl)


@pytest.mark.parametrize("n,ci,co,h", [(8, 64, 128, 32), (4, 128, 256, 16), (2, 256, 512, 8)])
def test_block_end_dual_batchnorm_equals_two_launches(pkg, gpu, n, ci, co, h):
    """afan_bn_train_forward_acc_dual: relu(bn_a(raw_a) + bn_b(raw_b)) with both BatchNorms' moments taken from convolution
    epilogues — one launch for the end of a projection block (resnet_s.py:72-77).  Against the two launches it replaces:
    statistics blocks and running buffers bit-identical, output equal up to the bf16 rounding of the intermediate tensor
    the fused kernel no longer stores (compared in fp32 against the unrounded formula)."""
    import torch.nn as nn
    ops = pkg.ops
    g = torch.Generator().manual_seed(4)
    cl = torch.channels_last
    x = torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16().contiguous(memory_format=cl)
    w1 = (torch.randn(co, ci, 3, 3, generator=g) * 0.05).to(gpu).bfloat16().contiguous(memory_format=cl)
    wsc = (torch.randn(co, ci, 1, 1, generator=g) * 0.1).to(gpu).bfloat16().contiguous(memory_format=cl)
    res = {}
    for mode in ("dual", "two"):
        bna, bnb = nn.BatchNorm2d(co).to(gpu), nn.BatchNorm2d(co).to(gpu)
        with torch.no_grad():
            for b_, s_ in ((bna, 1), (bnb, 2)):
                gg = torch.Generator().manual_seed(s_)
                b_.weight.copy_(1 + 0.2 * torch.randn(co, generator=gg))
                b_.bias.copy_(0.1 * torch.randn(co, generator=gg))
                b_.running_mean.copy_(0.05 * torch.randn(co, generator=gg))
        ops.acc_reset(gpu)
        (ra, rb), (sta, stb) = ops.conv_fwd_multi(x, [w1, wsc], 2, [1, 1], [bna.running_mean, bnb.running_mean])
        if mode == "dual":
            y, sa, sb = ops.bn_train_forward_dual(ra, bna, sta, 0.1, rb, bnb, stb, 0.1)
        else:
            r_, sb = ops.bn_train_forward(rb, bnb.weight, bnb.bias, None, False, bnb.eps, 0.1, bnb.running_mean, bnb.running_var,
                                          bnb.num_batches_tracked, stb)
            y, sa = ops.bn_train_forward(ra, bna.weight, bna.bias, r_, True, bna.eps, 0.1, bna.running_mean, bna.running_var,
                                         bna.num_batches_tracked, sta)
        res[mode] = (y.float(), sa.clone(), sb.clone(), {k: v.clone() for b_ in (bna, bnb) for k, v in b_.state_dict().items() if "running" in k or "num" in k},
                     ra.float(), rb.float())
    d, t = res["dual"], res["two"]
    assert torch.equal(d[1], t[1]) and torch.equal(d[2], t[2])
    for k in t[3]:
        assert torch.equal(d[3][k], t[3][k]), k
    exact = torch.relu(d[4] * d[1][2].view(1, -1, 1, 1) + d[1][3].view(1, -1, 1, 1) + d[5] * d[2][2].view(1, -1, 1, 1) + d[2][3].view(1, -1, 1, 1))
    e_dual = float((d[0] - exact).norm() / exact.norm())
    e_two = float((t[0] - exact).norm() / exact.norm())
    assert e_dual < 3e-3 and e_dual <= e_two, (e_dual, e_two)          # one bf16 rounding instead of two


@pytest.mark.parametrize("shapes", [
    [(2, 1024, 256, 33, 1, 1, 1), (2, 256, 256, 33, 3, 1, 1), (2, 256, 1024, 33, 1, 1, 1)],          # a layer3 bottleneck at 2 images
    [(2, 2048, 512, 33, 1, 1, 1), (2, 512, 512, 33, 3, 1, 2), (2, 512, 2048, 33, 1, 1, 1), (2, 2048, 256, 33, 1, 1, 1)],
    [(8, 128, 128, 16, 3, 1, 1), (8, 128, 128, 16, 3, 1, 1)]])
def test_wgrad_multi_equals_separate_launches(pkg, gpu, shapes):
    """afan_conv_wgrad_multi_nhwc_bf16: the weight gradients of several layers in one launch + one reduction launch, added
    into their fp32 gradient tensors — bit-identical to one launch per layer (same slices, same order)."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(6)
    cl = torch.channels_last
    items, refs = [], []
    for (n, ci, co, h, k, st, dil) in shapes:
        x = torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16().contiguous(memory_format=cl)
        dy = (torch.randn(n, co, h, h, generator=g) * 0.1).to(gpu).bfloat16().contiguous(memory_format=cl)
        g0 = torch.randn(co, ci, k, k, generator=g).to(gpu).contiguous(memory_format=cl)
        items.append((x, dy, k, st, dil, g0.clone()))
        refs.append(ops.conv_wgrad(x, dy, k, st, g0.clone(), accumulate=True, dilation=dil))
    codes = {ops.conv_wgrad_plan(x, dy, k, st) for (x, dy, k, st, _, _) in items}
    assert len(codes) == 1 and 0 not in codes
    ops.conv_wgrad_multi(items)
    for it, ref in zip(items, refs):
        assert torch.equal(it[5], ref)


@pytest.mark.parametrize("shape", [(1, 1024, 256, 38, 57, 1, 1), (1, 256, 256, 38, 57, 3, 1), (1, 256, 1024, 38, 57, 1, 1), (2, 512, 512, 30, 41, 3, 2),
                                   (1, 512, 2048, 38, 57, 1, 2), (128, 512, 512, 7, 7, 3, 1), (3, 64, 256, 20, 24, 1, 1)])
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (False, False)])
def test_conv_with_frozen_batchnorm_epilogue_equals_two_launches(pkg, gpu, shape, res, relu):
    """afan_conv_fwd_affine_nhwc_bf16, any_family = 0 (Detection's frozen bottlenecks: convolution + BatchNorm(eval) (+ residual) (+ ReLU) in one
    launch) against the convolution launch followed by afan_affine_apply: the same bits."""
    n, ci, co, h, w, k, st = shape
    g = torch.Generator().manual_seed(ci + co + k)
    cl = torch.channels_last
    x = torch.randn(n, ci, h, w, generator=g).to(gpu).bfloat16().contiguous(memory_format=cl)
    wt = (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5).to(gpu).bfloat16().contiguous(memory_format=cl)
    mean, var = torch.randn(co, generator=g).to(gpu), (torch.rand(co, generator=g) + 0.5).to(gpu)
    coefs = pkg.ops.affine_coefs(mean, torch.rsqrt(var + 1e-5), (torch.rand(co, generator=g) + 0.5).to(gpu), torch.randn(co, generator=g).to(gpu))
    raw = pkg.ops.conv_fwd(x, wt, st)
    r = torch.randn(raw.shape, generator=g).to(gpu).bfloat16().contiguous(memory_format=cl) if res else None
    want = pkg.ops.affine_apply(raw, coefs, r, relu)
    got = pkg.ops.conv_fwd_affine(x, wt, st, coefs, r, relu)
    assert got is not None and got.stride() == want.stride()
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())


def test_conv_with_frozen_batchnorm_epilogue_declines_other_kernels_shapes(pkg, gpu):
    cl = torch.channels_last
    x = torch.randn(2, 64, 32, 32, device=gpu).bfloat16().contiguous(memory_format=cl)
    w = torch.randn(64, 64, 3, 3, device=gpu).bfloat16().contiguous(memory_format=cl)
    coefs = pkg.ops.affine_coefs(torch.zeros(64, device=gpu), torch.ones(64, device=gpu), torch.ones(64, device=gpu), torch.zeros(64, device=gpu))
    assert pkg.ops.conv_fwd_affine(x, w, 1, coefs) is None            # the 64 -> 64 weights-in-registers kernel's shape


@pytest.mark.parametrize("shape", [(1, 256, 1024, 38, 57, 1, 1), (1, 256, 256, 38, 57, 3, 1), (2, 512, 512, 30, 41, 3, 2), (128, 512, 2048, 7, 7, 1, 1),
                                   (1, 128, 128, 75, 113, 3, 2), (3, 64, 256, 20, 24, 1, 1)])
def test_dgrad_with_frozen_batchnorm_backward_epilogue_equals_two_launches(pkg, gpu, shape):
    """afan_conv_dgrad_affine_nhwc_bf16, any_family = 0 (an input gradient + the backward of the frozen BatchNorm + ReLU in front of that convolution
    in one launch, stride 1 and the four parity classes of stride 2) against afan_conv_dgrad_nhwc_bf16 followed by
    afan_affine_relu_bwd: the same bits."""
    n, ci, co, h, w, k, st = shape
    g = torch.Generator().manual_seed(ci + co + k + st)
    cl = torch.channels_last
    ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
    dy = torch.randn(n, co, ho, wo, generator=g).to(gpu).bfloat16().contiguous(memory_format=cl)
    wt = (torch.randn(ci, co, k, k, generator=g) / (co * k * k) ** 0.5).to(gpu).bfloat16().contiguous(memory_format=cl)
    act = torch.relu(torch.randn(n, ci, h, w, generator=g)).to(gpu).bfloat16().contiguous(memory_format=cl)      # ~half zeros
    alpha = (torch.rand(ci, generator=g) + 0.5).to(gpu)
    raw = pkg.ops.conv_dgrad(dy, wt, (h, w), st)
    want, _ = pkg.ops.affine_relu_backward(raw, act, alpha, True)
    got = pkg.ops.conv_dgrad_affine(dy, wt, (h, w), st, alpha, act)
    assert got is not None and torch.equal(got, want), float((got.float() - want.float()).abs().max())


@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("shape", [(1, 1024, 256, 38, 57, 1, 1), (1, 256, 64, 150, 226, 1, 1), (2, 512, 128, 40, 56, 1, 1), (128, 2048, 512, 7, 7, 1, 1),
                                   (1, 256, 256, 38, 57, 3, 1)])
def test_dgrad_with_block_output_backward_epilogue_equals_two_launches(pkg, gpu, shape, with_addend):
    """afan_conv_dgrad_dual_nhwc_bf16 (the input gradient that arrives at a frozen-BatchNorm residual block's output, plus the other
    branch's share, masked by that output and leaving twice: as it is for the shortcut, times alpha for the last convolution)
    against afan_conv_dgrad_nhwc_bf16(addend) followed by afan_affine_relu_bwd with both outputs: the same bits."""
    n, ci, co, h, w, k, st = shape
    g = torch.Generator().manual_seed(ci + co + k + int(with_addend))
    cl = torch.channels_last
    dy = torch.randn(n, co, h, w, generator=g).to(gpu).bfloat16().contiguous(memory_format=cl)
    wt = (torch.randn(ci, co, k, k, generator=g) / (co * k * k) ** 0.5).to(gpu).bfloat16().contiguous(memory_format=cl)
    act = torch.relu(torch.randn(n, ci, h, w, generator=g)).to(gpu).bfloat16().contiguous(memory_format=cl)      # ~half zeros
    add = torch.randn(n, ci, h, w, generator=g).to(gpu).bfloat16().contiguous(memory_format=cl) if with_addend else None
    alpha = (torch.rand(ci, generator=g) + 0.5).to(gpu)
    raw = pkg.ops.conv_dgrad(dy, wt, (h, w), st, addend=add)
    want = pkg.ops.affine_relu_backward(raw, act, alpha, True, want_dx=True, want_dres=True)
    got = pkg.ops.conv_dgrad_dual(dy, wt, (h, w), st, add, alpha, act)
    assert got is not None
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _mk_bn(co, gpu, seed):
    import torch.nn as nn
    b = nn.BatchNorm2d(co).to(gpu)
    with torch.no_grad():
        gg = torch.Generator().manual_seed(seed)
        b.weight.copy_(1 + 0.2 * torch.randn(co, generator=gg))
        b.bias.copy_(0.1 * torch.randn(co, generator=gg))
        b.running_mean.copy_(0.05 * torch.randn(co, generator=gg))
        b.running_var.copy_(1 + 0.1 * torch.rand(co, generator=gg))
    return b


def _bn_state(b):
    return {k: v.clone() for k, v in b.state_dict().items() if "running" in k or "num" in k}


GRID_SHAPES = [  # n, ci, co, h, k, dilation: the training step's own launches (256-row, 256 x 64 and 128 x 64 halo tiles) and smaller
    # batches; k = 1: the bottleneck blocks' 1x1 convolutions on the per-tap variants (ResNet-50's layer3 / layer4 at 64 images: four-
    # stage 128- and 64-row tiles, two-stage tiles at two workgroups per CU; DeepLab's at two 513^2 images: 280 workgroups, beyond the
    # four-stage form's one per CU), a 3x3 whose halo does not fit (33 x 33 images) and DeepLab's atrous 3x3 (dilation 2)
    (256, 128, 128, 16, 3, 1), (256, 256, 256, 8, 3, 1), (256, 512, 512, 4, 3, 1), (64, 128, 128, 16, 3, 1), (32, 256, 256, 8, 3, 1),
    (100, 128, 256, 8, 3, 1), (64, 1024, 256, 14, 1, 1), (64, 512, 2048, 7, 1, 1), (32, 256, 1024, 14, 1, 1), (16, 2048, 512, 7, 1, 1),
    (2, 256, 256, 33, 3, 1), (2, 256, 1024, 33, 1, 1), (2, 512, 512, 33, 3, 2),
    (2, 1024, 256, 33, 1, 1), (3, 1024, 256, 33, 1, 1)]      # round 6: DeepLab's 70- / 104-workgroup launches on 64 x 64 tiles (dispatch_bnf's rule)


@pytest.mark.parametrize("n,ci,co,h,k,d", GRID_SHAPES)
@pytest.mark.parametrize("form", ["plain", "residual", "projection"])
def test_conv_with_in_launch_batchnorm_equals_two_launches(pkg, gpu, n, ci, co, h, form, k, d):
    """afan_conv_fwd_bn_nhwc_bf16 (sums -> grid barrier -> totals -> second pass, one launch) against afan_conv_fwd_nhwc_bf16 +
    afan_bn_train_forward_acc[_dual]: raw output, normalised output, statistics block, running buffers — every bit; twice in a row
    (the barrier words reset themselves) with two running-statistics updates per pass (the shared head pass's form)."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(n + ci + co + h)
    x = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    w = _cl((torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5).to(gpu).bfloat16())
    res = _cl(torch.randn(n, co, h, h, generator=g).to(gpu).bfloat16())
    xs = _cl(torch.randn(n, ci, 2 * h, 2 * h, generator=g).to(gpu).bfloat16())          # the projection's input (stride 2)
    wsc = _cl((torch.randn(co, ci, 1, 1, generator=g) * 0.1).to(gpu).bfloat16())
    out = {}
    for mode in ("two", "one"):
        bn, bsc = _mk_bn(co, gpu, 1), _mk_bn(co, gpu, 2)
        got = []
        for rep in range(2):
            ops.acc_reset(gpu)
            with ops.bn_running_updates(2):
                if form == "projection":
                    rsc, stc = ops.conv_fwd(xs, wsc, 2, stats_shift=bsc.running_mean, want_stats=True)
                    if mode == "one":
                        r = ops.conv_fwd_bn(x, w, bn, 0.1, relu=True, sc=(rsc, bsc, stc, 0.1), dilation=d)
                        assert r is not None, "the in-launch form declined a launch of the training step's kind"
                        raw, act, st, ssc = r
                    else:
                        raw, sta = ops.conv_fwd(x, w, 1, stats_shift=bn.running_mean, want_stats=True, dilation=d)
                        act, st, ssc = ops.bn_train_forward_dual(raw, bn, sta, 0.1, rsc, bsc, stc, 0.1)
                    got.append((raw.clone(), act.clone(), st.clone(), ssc.clone(), _bn_state(bn), _bn_state(bsc)))
                else:
                    rr = res if form == "residual" else None
                    if mode == "one":
                        r = ops.conv_fwd_bn(x, w, bn, 0.1, residual=rr, relu=True, dilation=d)
                        assert r is not None
                        raw, act, st = r
                    else:
                        raw, sta = ops.conv_fwd(x, w, 1, stats_shift=bn.running_mean, want_stats=True, dilation=d)
                        act, st = ops.bn_train_forward(raw, bn.weight, bn.bias, rr, True, bn.eps, 0.1, bn.running_mean, bn.running_var,
                                                       bn.num_batches_tracked, sta)
                    got.append((raw.clone(), act.clone(), st.clone(), _bn_state(bn)))
        out[mode] = got
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)
    for a, b in zip(out["one"], out["two"]):
        for p, q in zip(a, b):
            if isinstance(p, dict):
                for k in p:
                    assert torch.equal(p[k], q[k]), k
            else:
                assert torch.equal(p, q)
    assert int(out["one"][1][-1]["num_batches_tracked"]) == 4


@pytest.mark.parametrize("n,ci,co,h,k,d", GRID_SHAPES)
@pytest.mark.parametrize("form", ["bn1", "block_output"])
def test_dgrad_with_in_launch_batchnorm_backward_equals_two_launches(pkg, gpu, n, ci, co, h, form, k, d):
    """afan_conv_dgrad_bn_nhwc_bf16 against afan_conv_dgrad_nhwc_bf16 (BatchNorm-backward sums in its epilogue) +
    afan_bn_backward_acc: the gradient entering the BatchNorm's input, the masked gradient (block-output form: mask from the stored
    output, other branch's gradient added first) and the affine parameters' gradients (written, then accumulated) — every bit."""
    ops = pkg.ops
    if k == 1:
        ci, co = co, ci                # (the input gradient's GEMM writes ci channels: the listed launches' workgroup counts, mirrored)
    g = torch.Generator().manual_seed(3 * n + ci + co + h)
    dy = _cl(torch.randn(n, co, h, h, generator=g).to(gpu).bfloat16())
    w = _cl((torch.randn(co, ci, k, k, generator=g) / (co * k * k) ** 0.5).to(gpu).bfloat16())
    wt = _cl(w.permute(1, 0, 2, 3))
    bn_x = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    addend = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    res = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    gamma, beta = (torch.rand(ci, generator=g) + 0.5).to(gpu), (torch.randn(ci, generator=g) * 0.3).to(gpu)
    out_block = form == "block_output"
    y, stats = ops.bn_train_forward(bn_x, gamma, beta, res if out_block else None, True, 1e-5, 0.1, None, None, None)
    got = {}
    for mode in ("two", "one"):
        dwb = torch.zeros(2, ci, device=gpu)
        rs = []
        for rep in range(2):                               # second pass accumulates into dweight / dbias
            ops.acc_reset(gpu)
            if mode == "one":
                r = ops.conv_dgrad_bn(dy, wt, (h, h), bn_x, stats, True, bn_y=y if out_block else None,
                                      addend=addend if out_block else None, want_dres=out_block, dweight=dwb[0], dbias=dwb[1],
                                      accumulate=rep > 0, dilation=d)
                assert r is not None, "the in-launch form declined a launch of the training step's kind"
                dx, dres = r
            else:
                gsum, part = ops.conv_dgrad(dy, wt, (h, h), 1, addend=addend if out_block else None, bn_bwd=(bn_x, stats, True),
                                            bn_y=y if out_block else None, dilation=d)
                dx, dres = ops.bn_backward(gsum, bn_x, y if out_block else None, stats, gamma, beta, True, out_block, dwb[0], dwb[1],
                                           accumulate=rep > 0, partials=part)
            rs.append((dx.clone(), None if dres is None else dres.clone(), dwb.clone()))
        got[mode] = rs
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)
    for a, b in zip(got["one"], got["two"]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1])


def test_in_launch_batchnorm_declines_launches_it_cannot_take(pkg, gpu):
    """More workgroups than the chip holds at once (3x3 and 1x1), fewer than eight, the 64 -> 64 kernel's shape: None, and nothing ran."""
    ops = pkg.ops
    bn = _mk_bn(128, gpu, 1)
    before = dict(ops.CALLS)
    x = _cl(torch.randn(1024, 128, 16, 16, device=gpu).bfloat16())                 # 2 048 row tiles of 128
    w = _cl((torch.randn(128, 128, 3, 3, device=gpu) * 0.03).bfloat16())
    assert ops.conv_fwd_bn(x, w, bn, 0.1) is None
    assert ops.conv_fwd_bn(x, _cl((torch.randn(128, 128, 1, 1, device=gpu) * 0.1).bfloat16()), bn, 0.1) is None
    x1 = _cl(torch.randn(8, 128, 16, 16, device=gpu).bfloat16())
    xs = _cl(torch.randn(1, 128, 16, 16, device=gpu).bfloat16())                   # 2 row tiles: fewer than the barrier's 8 shards
    assert ops.conv_fwd_bn(xs, _cl((torch.randn(128, 128, 1, 1, device=gpu) * 0.1).bfloat16()), bn, 0.1) is None
    x64 = _cl(torch.randn(8, 64, 32, 32, device=gpu).bfloat16())
    assert ops.conv_fwd_bn(x64, _cl((torch.randn(64, 64, 3, 3, device=gpu) * 0.05).bfloat16()), _mk_bn(64, gpu, 2), 0.1) is None
    with ops.grid_bn(False):
        assert ops.conv_fwd_bn(x1, w, bn, 0.1) is None
    assert ops.CALLS["conv_fwd"] == before["conv_fwd"] and ops.CALLS["conv_bn_fused"] == before["conv_bn_fused"]
    assert int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("n,ci,co,h", [(256, 128, 256, 16), (256, 256, 512, 8), (64, 128, 256, 16), (32, 256, 512, 8)])
def test_stride2_pair_dgrad_with_in_launch_batchnorm_backward_equals_two_launches(pkg, gpu, n, ci, co, h):
    """afan_conv_dgrad_sc_bn_nhwc_bf16: the input gradient of a block's first 3x3 / 2 and its 1x1 / 2 projection (ONE launch, four
    output-parity classes) with the backward of the PREVIOUS block's last BatchNorm inside it — one set of sums over the four
    classes, then the grid barrier — against afan_conv_dgrad_sc_nhwc_bf16 (sums in its epilogue) + afan_bn_backward_acc: the
    gradient entering the BatchNorm's input, the masked gradient and the parameter gradients (written, then accumulated), bit for bit."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(7 * n + ci + co + h)
    both = _cl(torch.randn(2 * n, co, h // 2, h // 2, generator=g).to(gpu).bfloat16())
    dy, dy_sc = both[:n], both[n:]
    w1 = (torch.randn(co, ci, 3, 3, generator=g) / (co * 9) ** 0.5).to(gpu).bfloat16()
    wsc = (torch.randn(co, ci, 1, 1, generator=g) / co ** 0.5).to(gpu).bfloat16()
    wt10 = torch.cat([w1.permute(1, 2, 3, 0).reshape(ci, 9, co), wsc.permute(1, 2, 3, 0).reshape(ci, 1, co)], dim=1).contiguous()
    wt1 = _cl(w1.permute(1, 0, 2, 3))
    bn_x = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    res = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    gamma, beta = (torch.rand(ci, generator=g) + 0.5).to(gpu), (torch.randn(ci, generator=g) * 0.3).to(gpu)
    y, stats = ops.bn_train_forward(bn_x, gamma, beta, res, True, 1e-5, 0.1, None, None, None)
    got = {}
    for mode in ("two", "one"):
        dwb = torch.zeros(2, ci, device=gpu)
        rs = []
        for rep in range(2):
            ops.acc_reset(gpu)
            if mode == "one":
                r = ops.conv_dgrad_bn(dy, None, (h, h), bn_x, stats, True, bn_y=y, want_dres=True, dweight=dwb[0], dbias=dwb[1],
                                      accumulate=rep > 0, pair=(dy_sc, wt10))
                assert r is not None, "the in-launch form declined a launch of the training step's kind"
                dx, dres = r
            else:
                gsum, part = ops.conv_dgrad(dy, wt1, (h, h), 2, sc=(dy_sc, wt10), bn_bwd=(bn_x, stats, True), bn_y=y)
                dx, dres = ops.bn_backward(gsum, bn_x, y, stats, gamma, beta, True, True, dwb[0], dwb[1], accumulate=rep > 0, partials=part)
            rs.append((dx.clone(), dres.clone(), dwb.clone()))
        got[mode] = rs
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)
    for a, b in zip(got["one"], got["two"]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("n,ci,co,h", [(256, 64, 128, 32), (256, 128, 256, 16), (256, 256, 512, 8), (32, 128, 256, 16)])
def test_two_problem_forward_with_in_launch_batchnorm_equals_two_launches(pkg, gpu, n, ci, co, h):
    """afan_conv_fwd_multi_bn_nhwc_bf16: a block's first 3x3 / stride-2 convolution and its 1x1 / stride-2 projection as ONE launch
    with the first one's BatchNorm + ReLU inside it (only problem 0's workgroups meet at the barrier; the projection's leave after
    their sums) against afan_conv_fwd_multi_nhwc_bf16 + afan_bn_train_forward_acc: both raw outputs, the normalised output, the
    statistics block, the running buffers, and the projection's accumulator sums (read through its own BatchNorm) — every bit."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(11 * n + ci + co + h)
    x = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    w1 = _cl((torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5).to(gpu).bfloat16())
    wsc = _cl((torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5).to(gpu).bfloat16())
    out = {}
    for mode in ("two", "one"):
        bn, bsc = _mk_bn(co, gpu, 1), _mk_bn(co, gpu, 2)
        got = []
        for rep in range(2):
            ops.acc_reset(gpu)
            if mode == "one":
                r = ops.conv_fwd_multi_bn(x, [w1, wsc], 2, [1, 1], [bn.running_mean, bsc.running_mean], bn, 0.1)
                assert r is not None, "the in-launch form declined a launch of the training step's kind"
                (raw1, rawsc), (st1, stc), act, st = r
            else:
                (raw1, rawsc), (st1, stc) = ops.conv_fwd_multi(x, [w1, wsc], 2, [1, 1], [bn.running_mean, bsc.running_mean])
                act, st = ops.bn_train_forward(raw1, bn.weight, bn.bias, None, True, bn.eps, 0.1, bn.running_mean, bn.running_var,
                                               bn.num_batches_tracked, st1)
            ysc, ssc = ops.bn_train_forward(rawsc, bsc.weight, bsc.bias, None, False, bsc.eps, 0.1, bsc.running_mean, bsc.running_var,
                                            bsc.num_batches_tracked, stc)
            got.append((raw1.clone(), rawsc.clone(), act.clone(), st.clone(), ysc.clone(), ssc.clone(), _bn_state(bn), _bn_state(bsc)))
        out[mode] = got
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)
    for a, b in zip(out["one"], out["two"]):
        for p_, q_ in zip(a, b):
            if isinstance(p_, dict):
                for k in p_:
                    assert torch.equal(p_[k], q_[k]), k
            else:
                assert torch.equal(p_, q_)


def test_in_launch_batchnorm_beside_side_stream_kernels_takes_one_workgroup_per_cu(pkg, gpu):
    """Round 5 regression (DeepLab at 8 images, weight gradients on the side stream): 276 workgroups of the two-per-CU tile form beside
    a long-lived weight-gradient launch — the first workgroup of a CU lands behind the other kernel's LDS range, that kernel leaves,
    and the second never finds a contiguous range while the first spins for it (200 ms: the spin bound).  While kernels of another
    stream may run (ops.grid_shared / resnet_s.wgrad_stream) only launches of one workgroup per CU take the in-launch form; the
    same launch beside a real side-stream weight gradient then completes (two launches) and no barrier gives up."""
    ops, rs = pkg.ops, pkg.resnet_s
    n, ci, co, h = 8, 1024, 512, 33                         # 69 row tiles x 4 column tiles = 276 workgroups (DeepLab's layer4 conv1 at 8 images)
    g = torch.Generator().manual_seed(5)
    x = _cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16())
    w = _cl((torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5).to(gpu).bfloat16())
    xs = _cl(torch.randn(n, 256, h, h, generator=g).to(gpu).bfloat16())
    dys = _cl(torch.randn(n, 256, h, h, generator=g).to(gpu).bfloat16())
    gw = _cl(torch.zeros(256, 256, 3, 3, device=gpu))
    bn = _mk_bn(co, gpu, 1)
    ops.acc_reset(gpu)
    assert ops.conv_fwd_bn(x, w, bn, 0.1) is not None       # alone on the GPU: taken
    side = torch.cuda.Stream(device=gpu)
    with rs.wgrad_stream(True):
        for _ in range(3):
            side.wait_stream(torch.cuda.current_stream(gpu))
            with torch.cuda.stream(side):
                ops.conv_wgrad(xs, dys, 3, 1, gw, accumulate=True)      # ~288 long-lived workgroups with 40 KB of LDS each
            ops.acc_reset(gpu)
            assert ops.conv_fwd_bn(x, w, bn, 0.1) is None               # beside it: declined (the caller's two launches run)
            raw, st = ops.conv_fwd(x, w, 1, stats_shift=bn.running_mean, want_stats=True)
            ops.bn_train_forward(raw, bn.weight, bn.bias, None, True, bn.eps, 0.1, bn.running_mean, bn.running_var, bn.num_batches_tracked, st)
        torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)
    ops.acc_reset(gpu)
    assert ops.conv_fwd_bn(x, w, bn, 0.1) is not None       # and taken again afterwards
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)


@pytest.mark.parametrize("n,ci,co,h", [(256, 256, 256, 8), (256, 512, 512, 4), (64, 128, 128, 16), (100, 128, 256, 8)])
def test_dgrad_with_both_batchnorm_backwards_of_a_projection_block(pkg, gpu, n, ci, co, h):
    """The block-output form with the producing block's projection shortcut: its BatchNorm (no ReLU) receives the masked gradient
    as well, and afan_conv_dgrad_bn_nhwc_bf16(sc_x ...) runs that backward in the same launch (third column sum, second
    accumulator block, third output).  The main results keep their bits; the projection's input gradient and parameter gradients
    equal afan_bn_backward's on the launch's own masked gradient up to the summation order of the two channel sums."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(5 * n + ci + co + h)
    dy = _cl(torch.randn(n, co, h, h, generator=g).to(gpu).bfloat16())
    w = _cl((torch.randn(co, ci, 3, 3, generator=g) / (co * 9) ** 0.5).to(gpu).bfloat16())
    wt = _cl(w.permute(1, 0, 2, 3))
    bn_x, sc_x, addend, res = (_cl(torch.randn(n, ci, h, h, generator=g).to(gpu).bfloat16()) for _ in range(4))
    gamma, beta = (torch.rand(ci, generator=g) + 0.5).to(gpu), (torch.randn(ci, generator=g) * 0.3).to(gpu)
    gsc, bsc = (torch.rand(ci, generator=g) + 0.5).to(gpu), (torch.randn(ci, generator=g) * 0.3).to(gpu)
    ysc, st_sc = ops.bn_train_forward(sc_x, gsc, bsc, None, False, 1e-5, 0.1, None, None, None)
    y, stats = ops.bn_train_forward(bn_x, gamma, beta, ysc, True, 1e-5, 0.1, None, None, None)
    ops.acc_reset(gpu)
    dwb, dws = torch.zeros(2, ci, device=gpu), torch.zeros(2, ci, device=gpu)
    pair = torch.empty(2 * n, ci, h, h, device=gpu, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    r = ops.conv_dgrad_bn(dy, wt, (h, h), bn_x, stats, True, bn_y=y, addend=addend, want_dres=True, dweight=dwb[0], dbias=dwb[1],
                          sc=(sc_x, st_sc, pair[n:], dws[0], dws[1]))
    if r is None:                      # (the 768-thread x 128-column variant has no such form: two launches, as before)
        assert (n, ci, h) == (256, 128, 16)
        return
    dx, dres = r
    plain = ops.conv_dgrad_bn(dy, wt, (h, h), bn_x, stats, True, bn_y=y, addend=addend, want_dres=True)
    assert torch.equal(dx, plain[0]) and torch.equal(dres, plain[1])
    ref_w = torch.zeros(2, ci, device=gpu)
    ref, _ = ops.bn_backward(dres, sc_x, None, st_sc, gsc, bsc, False, False, ref_w[0], ref_w[1])
    torch.cuda.synchronize()
    assert not ops.grid_barrier_error(gpu)
    scale = max(1.0, float(ref_w.abs().max()))
    np.testing.assert_allclose(dws.cpu().numpy(), ref_w.cpu().numpy(), rtol=2e-4, atol=2e-4 * scale)
    a, b = pair[n:].float().cpu().numpy(), ref.float().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=2e-2, atol=2e-3 * max(1.0, float(np.abs(b).max())))
    assert float(np.mean(a != b)) < 0.02          # bf16 roundings that fell the other way: a handful
