"""The atrous epilogue forms (afan_conv_fwd_affine_nhwc_bf16, afan_conv_dgrad_affine_nhwc_bf16 at dilation > 1, any_family = 1;
ops.conv_fwd_affine / conv_dgrad_affine with dilation=) and the frozen bottleneck with an atrous 3x3 (afan_frozen_bottleneck_fwd / _bwd
with dilation > 1).

Two checks per problem:
  * elementwise against float64, with tests/test_conv_pinned_gpu.py's pin and its constant: the convolution's bf16 result r is the
    RNE bf16 of a value within C_BF16 * 2^-24 * S of the float64 result, and the epilogue is a monotone function of r evaluated the
    way the kernel evaluates it (one fp32 fma / multiply, the residual's fp32 add, the ReLU, one RNE to bf16) — so the output lies
    between the epilogue of the window's two ends, and equals the epilogue of RNE(float64) except at a few elements;
  * torch.equal against the two launches the form stands for (conv_fwd(dilation=) + affine_apply; conv_dgrad(dilation=) +
    affine_relu_backward): the library's definition of an epilogue form.
At dilation 1 any_family decides which kernel families answer.  Without a ReLU mask the tiled kernel has no input-gradient epilogue (its backward
epilogue always masks): dilation > 1 with act=None declines, launching nothing, and the two launches are what is pinned there.
The argument errors need no GPU (host pointers, nothing is launched)."""
import ctypes

import pytest
import torch

import test_conv_pinned_gpu as P

CL = torch.channels_last
GEOM = [(17, 19, 2), (17, 19, 6), (5, 5, 6), (5, 5, 18)]           # (h, w, dilation); on 5 x 5 every tap but the centre is outside
CHANNELS = [(64, 64), (128, 64), (64, 256)]
N = 2


def _operands(gpu, h, w, d, ci, co, salt):
    g = torch.Generator(device=gpu).manual_seed(P._seed(("affine_dil", h, w, d, ci, co), salt))
    x = P._cl(P._gauss((N, ci, h, w), 1.0, g, gpu))
    wt = P._cl(P._gauss((co, ci, 3, 3), (9 * ci) ** -0.5, g, gpu))
    return g, x, wt


def _coefs(pkg, gpu, g, c):
    mean, var = torch.randn(c, generator=g, device=gpu), torch.rand(c, generator=g, device=gpu) + 0.5
    weight, bias = torch.rand(c, generator=g, device=gpu) + 0.5, torch.randn(c, generator=g, device=gpu)
    weight[::3] *= -1.0                                             # both signs of alpha
    return pkg.ops.affine_coefs(mean, torch.rsqrt(var + 1e-5), weight, bias)


def _window(ref, bound):
    tol = P.C_BF16 * 2.0 ** -24 * bound
    return (ref - tol).float().to(torch.bfloat16), ref.float().to(torch.bfloat16), (ref + tol).float().to(torch.bfloat16)


def _between(got, ends, mid, what):
    """got between the epilogue of the window's two ends (either order: alpha has both signs), and the epilogue of RNE(float64)
    everywhere but at a few elements (test_conv_pinned_gpu._check_bf16's allowance)."""
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    gk, a, b = P._key(got), P._key(ends[0]), P._key(ends[1])
    bad = (gk < torch.minimum(a, b)) | (gk > torch.maximum(a, b))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} elements outside the float64 window; first at {bad.nonzero()[0].tolist()}"
    off = int((gk != P._key(mid)).sum())
    assert off <= max(8, got.numel() // 1000), f"{what}: {off} of {got.numel()} elements off the epilogue of the RNE bf16 of the float64 result"


def _affine64(r, coefs, res, relu):
    """afan_affine_apply's arithmetic on a bf16 tensor r: fmaf(r, alpha, beta) (one rounding to fp32: the float64 product and sum of
    an 8-bit and a 24-bit significand are exact), + residual in fp32, the ReLU, RNE to bf16."""
    al, be = coefs[2].double().view(1, -1, 1, 1), coefs[3].double().view(1, -1, 1, 1)
    t = (r.double() * al + be).float()
    if res is not None:
        t = t + res.float()
    if relu:
        t = torch.relu(t)
    return t.to(torch.bfloat16)


def _affine_bwd64(r, alpha, act):
    t = r.double() if act is None else torch.where(act.float() > 0, r.double(), torch.zeros_like(r, dtype=torch.float64))
    return (t * alpha.double().view(1, -1, 1, 1)).float().to(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("ci,co", CHANNELS)
@pytest.mark.parametrize("h,w,d", GEOM)
def test_fwd_affine_dil(pkg, gpu, h, w, d, ci, co):
    g, x, wt = _operands(gpu, h, w, d, ci, co, 1)
    coefs = _coefs(pkg, gpu, g, co)
    lo, mid, hi = _window(P._ref_fwd(x, wt, 1, d), P._ref_fwd(x.abs(), wt.abs(), 1, d))
    raw = pkg.ops.conv_fwd(x, wt, 1, dilation=d)
    resid = P._cl(P._gauss((N, co, h, w), 1.0, g, gpu))
    for res in (None, resid):
        for relu in (False, True):
            with pkg.ops.conv_trace() as tr:
                got = pkg.ops.conv_fwd_affine(x, wt, 1, coefs, res, relu, dilation=d)
            what = f"fwd_affine d={d} {h}x{w} {ci}->{co} res={res is not None} relu={relu} on {P._kernels(tr)}"
            assert got is not None and len(tr.records) == 1, what                 # one launch, on the tiled kernel
            assert tr.records[0]["kernel"].startswith("igemm_fwd<") and tr.records[0]["problem"] == (N, h, w, ci, co, 3, 1, d), what
            _between(got, (_affine64(lo, coefs, res, relu), _affine64(hi, coefs, res, relu)), _affine64(mid, coefs, res, relu), what)
            want = pkg.ops.affine_apply(raw, coefs, res, relu)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{what}: not conv_fwd + affine_apply"


@pytest.mark.gpu
@pytest.mark.parametrize("ci,co", CHANNELS)
@pytest.mark.parametrize("h,w,d", GEOM)
def test_dgrad_affine_dil(pkg, gpu, h, w, d, ci, co):
    g, _, wt = _operands(gpu, h, w, d, ci, co, 2)
    dy = P._cl(P._gauss((N, co, h, w), 1.0, g, gpu))
    act = P._cl(P._gauss((N, ci, h, w), 1.0, g, gpu))                # the producer's stored output: about half of it <= 0
    alpha = _coefs(pkg, gpu, g, ci)[2]
    wtt = P._wt(wt)
    lo, mid, hi = _window(P._ref_dgrad(dy, wt, (N, ci, h, w), 1, d), P._ref_dgrad(dy.abs(), wt.abs(), (N, ci, h, w), 1, d))
    raw = pkg.ops.conv_dgrad(dy, wtt, (h, w), 1, dilation=d)
    # with the ReLU mask: one launch
    with pkg.ops.conv_trace() as tr:
        got = pkg.ops.conv_dgrad_affine(dy, wtt, (h, w), 1, alpha, act, dilation=d)
    what = f"dgrad_affine d={d} {h}x{w} {ci}<-{co} masked on {P._kernels(tr)}"
    assert got is not None and len(tr.records) == 1 and tr.records[0]["kernel"].startswith("igemm_dgrad<"), what
    _between(got, (_affine_bwd64(lo, alpha, act), _affine_bwd64(hi, alpha, act)), _affine_bwd64(mid, alpha, act), what)
    want, _ = pkg.ops.affine_relu_backward(raw, act, alpha, True)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{what}: not conv_dgrad + affine_relu_backward"
    # without it: the tiled kernel declines and launches nothing; the two launches are the form, pinned the same way
    with pkg.ops.conv_trace() as tr:
        assert pkg.ops.conv_dgrad_affine(dy, wtt, (h, w), 1, alpha, None, dilation=d) is None
    assert tr.records == []
    two, _ = pkg.ops.affine_relu_backward(raw, None, alpha, False)
    _between(two, (_affine_bwd64(lo, alpha, None), _affine_bwd64(hi, alpha, None)), _affine_bwd64(mid, alpha, None),
             f"dgrad d={d} {h}x{w} {ci}<-{co} + affine_relu_backward(relu=0)")


@pytest.mark.gpu
@pytest.mark.parametrize("ci,co,k,st", [(64, 64, 3, 1), (128, 64, 3, 1), (64, 256, 3, 2), (64, 32, 3, 1), (256, 64, 1, 1)])
def test_dilation_one_any_family(pkg, gpu, ci, co, k, st):
    """dilation = 1, both directions: on a shape the tiled kernel takes, any_family = 0 and 1 give identical bits; on a shape of
    another family (here the small-channel kernel) any_family = 0 answers AFAN_ESHAPE where 1 launches.  Without the ReLU mask
    any_family = 1 is the entry the ops wrapper calls (the tiled kernel declines there), any_family = 0 asks for the mask."""
    lib = pkg._lib.load()
    g = torch.Generator(device=gpu).manual_seed(7 + ci + co)
    x, wt = P._cl(P._gauss((N, ci, 17, 19), 1.0, g, gpu)), P._cl(P._gauss((co, ci, k, k), (k * k * ci) ** -0.5, g, gpu))
    coefs, alpha = _coefs(pkg, gpu, g, co), _coefs(pkg, gpu, g, ci)[2]
    ho, wo = P._out_hw(17, 19, k, st, 1)
    res = P._cl(P._gauss((N, co, ho, wo), 1.0, g, gpu))
    tiled_shape = not (ci == 64 and co == 32)                        # (64 -> 64 at 17 x 19 is not the weights-in-registers kernel's: W = 19)

    def check(call, shape, want, what):
        """call(any_family, out) -> rc; want: the ops wrapper's result for any_kernel=True"""
        outs = [torch.empty(shape, dtype=torch.bfloat16, device=gpu).contiguous(memory_format=CL) for _ in range(2)]
        with pkg.ops.conv_trace() as tr:
            rc1 = call(1, outs[1])
        assert rc1 == 0 and torch.equal(outs[1].view(torch.int16), want.view(torch.int16)), what
        assert len(tr.records) == 1 and tr.records[0]["kernel"].startswith("igemm_") == tiled_shape, (what, P._kernels(tr))
        with pkg.ops.conv_trace() as tr:
            rc0 = call(0, outs[0])
        if tiled_shape:
            assert rc0 == 0 and torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{what}: any_family = 0 differs from 1"
        else:
            assert rc0 == -3 and tr.records == [], f"{what}: any_family = 0 on another family's shape"

    check(lambda af, out: lib.afan_conv_fwd_affine_nhwc_bf16(x.data_ptr(), wt.data_ptr(), out.data_ptr(), N, 17, 19, ci, co, k, st, 1,
                                                             coefs.data_ptr(), res.data_ptr(), 1, af, pkg.ops._stream(x)),
          (N, co, ho, wo), pkg.ops.conv_fwd_affine(x, wt, st, coefs, res, True, any_kernel=True), f"fwd {ci}->{co} k{k} s{st}")
    dy, act = P._cl(P._gauss((N, co, ho, wo), 1.0, g, gpu)), P._cl(P._gauss((N, ci, 17, 19), 1.0, g, gpu))
    wtt = P._wt(wt)

    def dgrad(af, out, a):
        return lib.afan_conv_dgrad_affine_nhwc_bf16(dy.data_ptr(), wtt.data_ptr(), out.data_ptr(), N, 17, 19, ci, co, k, st, 1,
                                                    alpha.data_ptr(), None if a is None else a.data_ptr(), af, pkg.ops._stream(dy))

    check(lambda af, out: dgrad(af, out, act), (N, ci, 17, 19),
          pkg.ops.conv_dgrad_affine(dy, wtt, (17, 19), st, alpha, act, any_kernel=True), f"dgrad {ci}<-{co} k{k} s{st}")
    want = pkg.ops.conv_dgrad_affine(dy, wtt, (17, 19), st, alpha, None, any_kernel=True)
    got = torch.empty((N, ci, 17, 19), dtype=torch.bfloat16, device=gpu).contiguous(memory_format=CL)
    rc = dgrad(1, got, None)
    if want is None:
        assert rc == -3 and tiled_shape                              # (the tiled kernel without a mask declines)
    else:
        assert rc == 0 and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert dgrad(0, got, None) == -4                                 # (any_family = 0: the mask is required)


@pytest.mark.gpu
@pytest.mark.parametrize("projection", [False, True], ids=["identity", "projection"])
def test_frozen_bottleneck_dil_equals_launch_by_launch(pkg, gpu, projection):
    """One block, planes 64, cin 256, 9 x 9, dilation 2: the output and dx of the one-call sequencers equal the block issued launch by
    launch through ops."""
    ops = pkg.ops
    n, cin, planes, h, w, d = 2, 256, 64, 9, 9, 2
    co = 4 * planes
    g = torch.Generator(device=gpu).manual_seed(31 + projection)
    x = P._cl(torch.relu(P._gauss((n, cin, h, w), 1.0, g, gpu)))
    shapes = [(planes, cin, 1), (planes, planes, 3), (co, planes, 1)] + ([(co, cin, 1)] if projection else [])
    ws = [P._cl(P._gauss((o, i, k, k), (k * k * i) ** -0.5, g, gpu)) for o, i, k in shapes] + ([] if projection else [None])
    ks = [_coefs(pkg, gpu, g, s[0]) for s in shapes] + ([] if projection else [None])
    wts = [None if t is None else P._wt(t) for t in ws]
    als = [None if k is None else k[2] for k in ks]
    plan = ops.frozen_bottleneck_plan(x, planes, 1, tuple(ws), tuple(ks), tuple(wts), tuple(als), (None,) * 4, dilation=d)
    assert plan.dilation == d and plan.n_wgrad == 0
    out, a1, a2 = ops.frozen_bottleneck_fwd_plan(x, plan)
    # launch by launch
    e1 = ops.affine_apply(ops.conv_fwd(x, ws[0], 1), ks[0], None, True)
    e2 = ops.affine_apply(ops.conv_fwd(e1, ws[1], 1, dilation=d), ks[1], None, True)
    res = ops.affine_apply(ops.conv_fwd(x, ws[3], 1), ks[3], None, False) if projection else x
    eo = ops.affine_apply(ops.conv_fwd(e2, ws[2], 1), ks[2], res, True)
    for got, want, name in ((a1, e1, "a1"), (a2, e2, "a2"), (out, eo, "out")):
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), name
    gy = P._cl(P._gauss((n, co, h, w), 1.0, g, gpu))
    dx = ops.frozen_bottleneck_bwd_plan(gy, x, a1, a2, out, plan, True)
    d3, dres = ops.affine_relu_backward(gy, eo, als[2], True, want_dx=True, want_dres=True)
    d2, _ = ops.affine_relu_backward(ops.conv_dgrad(d3, wts[2], (h, w), 1), e2, als[1], True)
    d1, _ = ops.affine_relu_backward(ops.conv_dgrad(d2, wts[1], (h, w), 1, dilation=d), e1, als[0], True)
    if projection:
        dd, _ = ops.affine_relu_backward(dres, None, als[3], False)
        addend = ops.conv_dgrad(dd, wts[3], (h, w), 1)
    else:
        addend = dres
    want = ops.conv_dgrad(d1, wts[0], (h, w), 1, addend=addend)
    assert torch.equal(dx.view(torch.int16), want.view(torch.int16))
    assert ops.frozen_bottleneck_bwd_plan(gy, x, a1, a2, out, plan, False) is None        # no dx asked for: none made


def test_argument_errors_without_gpu(pkg):
    """Null, misaligned and shape errors are reported before anything is launched (host pointers)."""
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)
    ESHAPE, ENULL, EALIGN = -3, -4, -2
    fwd, dgr = lib.afan_conv_fwd_affine_nhwc_bf16, lib.afan_conv_dgrad_affine_nhwc_bf16          # (any_family = 1 throughout)
    assert fwd(p, p, p, 1, 8, 8, 256, 256, 3, 2, 2, p, None, 1, 1, None) == ESHAPE       # dilation needs stride 1
    assert fwd(p, p, p, 1, 8, 8, 256, 256, 1, 1, 2, p, None, 1, 1, None) == ESHAPE       # ... and a 3x3
    assert fwd(p, p, p, 1, 8, 8, 256, 256, 3, 1, 0, p, None, 1, 1, None) == ESHAPE
    assert fwd(p, p, p, 1, 8, 8, 20, 256, 3, 1, 2, p, None, 1, 1, None) == ESHAPE        # channels no kernel takes
    assert fwd(p, p, p, 1, 8, 8, 32, 64, 3, 1, 2, p, None, 1, 1, None) == ESHAPE         # the small-channel kernel has no atrous form
    assert fwd(None, p, p, 1, 8, 8, 256, 256, 3, 1, 2, p, None, 1, 1, None) == ENULL
    assert fwd(p, p, p, 1, 8, 8, 256, 256, 3, 1, 2, None, None, 1, 1, None) == ENULL     # coefs
    assert fwd(odd, p, p, 1, 8, 8, 256, 256, 3, 1, 2, p, None, 1, 1, None) == EALIGN
    assert fwd(p, p, p, 1, 8, 8, 256, 256, 3, 1, 2, p, odd, 1, 1, None) == EALIGN        # residual
    assert fwd(p, p, p, 1, 8, 8, 256, 256, 3, 1, 1, None, None, 1, 1, None) == ENULL     # dilation 1: the same answers
    assert dgr(p, p, p, 1, 8, 8, 256, 256, 3, 2, 2, p, p, 1, None) == ESHAPE
    assert dgr(p, p, p, 1, 8, 8, 256, 256, 1, 1, 2, p, p, 1, None) == ESHAPE
    assert dgr(p, p, p, 1, 8, 8, 256, 256, 3, 1, 2, None, p, 1, None) == ENULL           # alpha
    assert dgr(None, p, p, 1, 8, 8, 256, 256, 3, 1, 2, p, p, 1, None) == ENULL
    assert dgr(p, odd, p, 1, 8, 8, 256, 256, 3, 1, 2, p, p, 1, None) == EALIGN
    assert dgr(p, p, p, 1, 8, 8, 256, 256, 3, 1, 2, p, None, 1, None) == ESHAPE          # no mask: the tiled kernel always masks
    assert dgr(p, p, p, 1, 8, 8, 256, 256, 3, 1, 2, p, odd, 1, None) == ESHAPE           # a misaligned mask, as at dilation 1
    bf, bb = lib.afan_frozen_bottleneck_fwd, lib.afan_frozen_bottleneck_bwd
    assert bf(p, 1, 9, 9, 256, 64, 2, 2, p, p, p, p, p, p, p, p, p, p, p, p, None) == ESHAPE         # atrous 3x3: stride 1
    assert bf(p, 1, 9, 9, 256, 64, 1, 0, p, p, p, None, p, p, p, None, p, p, p, p, None) == ESHAPE
    assert bf(None, 1, 9, 9, 256, 64, 1, 2, p, p, p, None, p, p, p, None, p, p, p, p, None) == ENULL
    assert bf(p, 1, 9, 9, 128, 64, 1, 2, p, p, p, None, p, p, p, None, p, p, p, p, None) == ESHAPE   # identity shortcut: cin = 4 planes
    args = (p, None, None, p, p, p, p, 1, 9, 9, 256, 64)
    tail = (p, p, p, None, p, p, p, None, None, None, None, None, None, p, p, None, None, None, None)
    assert bb(*args, 2, 2, *tail) == ESHAPE
    assert bb(*args, 1, 0, *tail) == ESHAPE
    assert bb(None, None, None, p, p, p, p, 1, 9, 9, 256, 64, 1, 2, *tail) == ENULL                  # neither g nor the pre-step pair
