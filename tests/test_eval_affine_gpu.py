"""The frozen-BatchNorm epilogue on the small-channel, 64 -> 64 weights-in-registers and 3-channel stem kernels
(afan_conv_fwd_affine_nhwc_bf16 with any_family = 1, ops.conv_fwd_affine(any_kernel=True)): bit for bit the convolution launch followed by
afan_affine_apply, on the kernel instantiation of its own.  afan_conv_fwd_affine_nhwc_bf16 keeps to the tiled kernel's shapes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _case(pkg, gpu, n, ci, co, h, w, k, st, seed, nan=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, h, w, generator=g)
    if nan:
        x[0, :, 1, 2] = float("nan")
    x = x.to(gpu).bfloat16().contiguous(memory_format=CL)
    wt = (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5).to(gpu).bfloat16().contiguous(memory_format=CL)
    mean, var = torch.randn(co, generator=g).to(gpu), (torch.rand(co, generator=g) + 0.5).to(gpu)
    weight, bias = (torch.rand(co, generator=g) + 0.5).to(gpu), torch.randn(co, generator=g).to(gpu)
    coefs = pkg.ops.affine_coefs(mean, torch.rsqrt(var + 1e-5), weight, bias)
    return g, x, wt, coefs


def _check(pkg, gpu, g, x, wt, coefs, st, res, relu, kernel):
    raw = pkg.ops.conv_fwd(x, wt, st)
    r = torch.randn(raw.shape, generator=g).to(gpu).bfloat16().contiguous(memory_format=CL) if res else None
    want = pkg.ops.affine_apply(raw, coefs, r, relu)
    with pkg.ops.conv_trace() as tr:
        got = pkg.ops.conv_fwd_affine(x, wt, st, coefs, r, relu, any_kernel=True)
    assert got is not None and got.stride() == want.stride()
    assert [t["kernel"] for t in tr.records] == [kernel]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), float((got.float() - want.float()).abs().nan_to_num().max())


@pytest.mark.parametrize("shape", [(128, 16, 16, 32, 32, 3, 1), (5, 16, 32, 32, 32, 3, 2), (3, 32, 64, 16, 16, 3, 2),
                                   (1, 16, 16, 32, 32, 3, 1), (7, 32, 32, 16, 16, 3, 1), (3, 64, 32, 8, 8, 1, 1),
                                   (9, 16, 32, 32, 32, 3, 1), (2, 32, 64, 16, 16, 3, 1)])
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (False, False), (True, False)])
def test_small_channel_affine_epilogue(pkg, gpu, shape, res, relu):
    n, ci, co, h, w, k, st = shape
    g, x, wt, coefs = _case(pkg, gpu, n, ci, co, h, w, k, st, ci + 3 * co + n)
    _check(pkg, gpu, g, x, wt, coefs, st, res, relu, "small_fwd_aff<%d>" % {16: 1, 32: 2, 64: 4}[ci])


@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 32, 32), (3, 16, 16), (16, 32, 32), (5, 16, 16)])
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (False, False), (True, False)])
def test_c64_affine_epilogue(pkg, gpu, shape, res, relu):
    n, h, w = shape
    g, x, wt, coefs = _case(pkg, gpu, n, 64, 64, h, w, 3, 1, 64 + n + h)
    _check(pkg, gpu, g, x, wt, coefs, 1, res, relu, "c64_fwd_aff")


@pytest.mark.parametrize("shape", [(2, 64, 64, 32, 32, 3, 1), (4, 16, 16, 32, 32, 3, 1), (4, 32, 64, 16, 16, 3, 2), (2, 3, 16, 32, 32, 3, 1)])
def test_tiled_only_entry_point_still_declines_the_other_kernels(pkg, gpu, shape):
    """The tiled-only entry point (Detection's) keeps declining the shapes of the other forward kernels, launching nothing; the
    any-family entry point takes them."""
    n, ci, co, h, w, k, st = shape
    g, x, wt, coefs = _case(pkg, gpu, n, ci, co, h, w, k, st, 21)
    with pkg.ops.conv_trace() as tr:
        assert pkg.ops.conv_fwd_affine(x, wt, st, coefs) is None
    assert tr.records == []                                              # nothing launched
    assert pkg.ops.conv_fwd_affine(x, wt, st, coefs, any_kernel=True) is not None


@pytest.mark.parametrize("shape", [(128, 16, 32, 32), (3, 64, 32, 32), (1, 16, 32, 64), (5, 32, 8, 32), (4, 64, 224, 224)])
@pytest.mark.parametrize("relu", [True, False])
def test_stem_affine_epilogue(pkg, gpu, shape, relu):
    n, co, h, w = shape
    g, x, wt, coefs = _case(pkg, gpu, n, 3, co, h, w, 3, 1, co + n + w)
    _check(pkg, gpu, g, x, wt, coefs, 1, False, relu, "stem_fwd_aff<%d>" % (2 if co > 32 else 1))


def test_stem_declines_a_residual(pkg, gpu):
    g, x, wt, coefs = _case(pkg, gpu, 2, 3, 16, 32, 32, 3, 1, 5)
    r = torch.zeros(2, 16, 32, 32, device=gpu, dtype=torch.bfloat16).contiguous(memory_format=CL)
    assert pkg.ops.conv_fwd_affine(x, wt, 1, coefs, r, True, any_kernel=True) is None


@pytest.mark.parametrize("kind", ["small", "c64", "stem"])
@pytest.mark.parametrize("res", [False, True])
def test_affine_epilogue_passes_nan(pkg, gpu, kind, res):
    n, ci, co, h, w = {"small": (3, 16, 32, 32, 32), "c64": (2, 64, 64, 16, 16), "stem": (2, 3, 64, 32, 32)}[kind]
    res = res and kind != "stem"
    g, x, wt, coefs = _case(pkg, gpu, n, ci, co, h, w, 3, 1, 99, nan=True)
    kernel = {"small": "small_fwd_aff<1>", "c64": "c64_fwd_aff", "stem": "stem_fwd_aff<2>"}[kind]
    _check(pkg, gpu, g, x, wt, coefs, 1, res, True, kernel)
