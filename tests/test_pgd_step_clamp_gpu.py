"""afan_pgd_step_clamp (csrc/afan_pgd.hip; ops.pgd_step_clamp_, pgd.step(clamp=...)): the last image-PGD step with the final clamp to
scalar bounds in one launch, bit for bit against

  (a) the composition it stands for, on the GPU: ops.pgd_step_ followed by ops.tensor_clamp_ with bound tensors filled with lo / hi;
  (b) the C oracle's oracle_pgd_step followed by the two compares in numpy;
  (c) a numpy restatement, one numpy operation per fp32 rounding (the only reference where there is no gradient: the composition
      has no gradient-less step).

A NaN is compared by position, everything else by its bits; the bf16 shadow against torch's round-to-nearest-even cast of (a).

Sizes.  1, 3, 4, 5, 7, 8, 9, and one below, at and above every boundary the kernel as written has — BLOCK = 256 threads, a grid of at
most 2048 workgroups:
    vector body (16-byte aligned tensors, 4 elements per lane):  vector width 4 (3, 4, 5);  a block's elements per pass 1024
        (1023, 1024, 1025);  the grid stride 2048 * 256 * 4 = 2097152 (2097151, 2097152, 2097153: the second trip of the loop)
    scalar body (anything else, one element per lane):  a block's elements per pass 256 (255, 256, 257);  the grid stride
        2048 * 256 = 524288 (524287, 524288, 524289)
Every size runs on aligned tensors AND on views offset by one element, which forces the scalar body; plus 2 x 3 x 32 x 32
channels-last.  Operands: the clean image spans [-0.2, 1.2] so that both bounds bite; the head of every tensor that is long enough
holds values below lo, above hi, exactly lo and hi, +-0, +-inf and NaN in x_adv, and zero (+-0), +-inf and NaN gradients."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ptr

pytestmark = pytest.mark.gpu

F = np.float32
GAMMA, EPS = F(0.5 / 255), F(2.0 / 255)
SIZES = [1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 524287, 524288, 524289, 2097151, 2097152, 2097153]
# (x_adv, grad) pairs written over the head of the operands
SPECIAL = [(-0.5, 1.0), (1.5, -1.0), (0.0, 1.0), (1.0, 1.0), (0.0, -1.0), (1.0, -1.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (np.inf, 1.0),
           (-np.inf, -1.0), (np.nan, 1.0), (0.5, np.nan), (0.5, 0.0), (0.5, -0.0), (0.5, np.inf), (0.5, -np.inf), (-1e-9, 0.0), (1.0 + 1e-7, 0.0),
           (0.999, 3.0), (0.001, -3.0)]


def _operands(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, n).astype(F)
    xa = (x + rng.uniform(-0.02, 0.02, n)).astype(F)
    g = rng.standard_normal(n).astype(F)
    if n >= 2 * len(SPECIAL):
        for i, (a, b) in enumerate(SPECIAL):
            xa[i], g[i] = a, b
    return xa, g, x


def _clamp(t, lo, hi):
    """attack_algo.py:9-19: two compares in its order; NaN compares false and passes through, -0 stays -0 against +0."""
    t = np.where(t < lo, lo, t).astype(F)
    return np.where(t > hi, hi, t).astype(F)


def _reference(xa, g, x, gamma, eps, clip, lo, hi):
    """(c): one numpy operation per fp32 rounding.  g None: no step."""
    t = xa.astype(F)
    with np.errstate(invalid="ignore"):
        if g is not None:
            d = (F(gamma) * np.sign(g.astype(F))).astype(F)        # np.sign: 0 -> 0 (its sign kept: -0 * gamma = -0), NaN -> NaN
            d = np.where(g == 0, F(gamma) * F(0.0), d).astype(F)   # the kernel's sign(+-0) is +0
            t = (t + d).astype(F)
        if clip:
            t = _clamp(t, (x - F(eps)).astype(F), (x + F(eps)).astype(F))
        return _clamp(t, F(lo), F(hi))


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, F).ravel(), np.ascontiguousarray(want, F).ravel()
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:8]}"
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~gn)
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"


def _dev(a, gpu, offset, dtype=None):
    """`a` on the GPU; offset: as a view that starts one element into its allocation (never 16-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    if not offset:
        return t.to(gpu)
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=gpu)
    base[1:].copy_(t)
    v = base[1:]
    assert v.data_ptr() % 16 != 0
    return v


def _check(pkg, gpu, c_oracle, xa, g, x, *, offset=False, gdt=torch.float32, clip=True, shadow=True, gamma=GAMMA, eps=EPS, lo=0.0, hi=1.0,
           what=""):
    ops = pkg.ops
    n = xa.size
    g_t = None if g is None else _dev(g, gpu, offset, gdt)
    g_used = None if g is None else g_t.float().cpu().numpy()                      # what the kernel sees after the bf16 rounding
    x_t = _dev(x, gpu, offset)
    got = _dev(xa, gpu, offset)
    sh = _dev(np.zeros(n, F), gpu, offset, torch.bfloat16) if shadow else None
    before = ops.CALLS["pgd_step_clamp"]
    r = ops.pgd_step_clamp_(got, g_t, float(gamma), x_t if clip else None, float(eps), clip, sh, lo, hi)
    assert r is got and ops.CALLS["pgd_step_clamp"] == before + 1
    got_np = got.cpu().numpy()
    want = _reference(xa, g_used, x, gamma, eps, clip, lo, hi)
    _same(got_np, want, what + " against numpy")
    if g is not None:
        comp = _dev(xa, gpu, offset)
        ops.pgd_step_(comp, g_t, float(gamma), x_t if clip else None, float(eps), clip)
        ops.tensor_clamp_(comp, torch.full_like(comp, lo), torch.full_like(comp, hi))
        _same(got_np, comp.cpu().numpy(), what + " against pgd_step_ + tensor_clamp_")
        ref = xa.copy()
        c_oracle.oracle_pgd_step(ptr(ref), ptr(np.ascontiguousarray(g_used)), ptr(x) if clip else None, n, F(gamma), F(eps), int(clip))
        _same(got_np, _clamp(ref, F(lo), F(hi)), what + " against the C oracle + two compares")
    if shadow:
        want_sh = torch.from_numpy(got_np).to(torch.bfloat16).float().numpy()      # torch's RNE cast of the fp32 result
        _same(sh.float().cpu().numpy(), want_sh, what + " shadow")


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_body(pkg, gpu, c_oracle, n, offset):
    xa, g, x = _operands(n, n)
    # clip x gradient dtype, the shadow on for one of each pair (every template argument is visited at every size)
    for k, (clip, gdt) in enumerate([(False, torch.float32), (True, torch.float32), (False, torch.bfloat16), (True, torch.bfloat16)]):
        _check(pkg, gpu, c_oracle, xa, g, x, offset=offset, gdt=gdt, clip=clip, shadow=k in (1, 2), what=f"n={n} clip={clip} {gdt}")


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset1"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("shadow", [False, True])
def test_variants(pkg, gpu, c_oracle, offset, clip, shadow):
    n = 1029
    xa, g, x = _operands(n, 77)
    kw = dict(offset=offset, clip=clip, shadow=shadow)
    _check(pkg, gpu, c_oracle, xa, g, x, gdt=torch.bfloat16 if shadow else torch.float32, what="plain", **kw)
    _check(pkg, gpu, c_oracle, xa, g, x, gamma=F(0.0), what="gamma = 0", **kw)
    _check(pkg, gpu, c_oracle, xa, np.zeros(n, F), x, what="zero gradients", **kw)
    _check(pkg, gpu, c_oracle, xa, None, x, what="grad = None", **kw)
    _check(pkg, gpu, c_oracle, xa, g, x, lo=-0.25, hi=0.75, what="lo / hi = -0.25 / 0.75", **kw)
    _check(pkg, gpu, c_oracle, xa, None, x, lo=0.125, hi=0.5, what="grad = None, lo / hi = 0.125 / 0.5", **kw)


def test_special_operands_land_where_the_issue_says(pkg, gpu):
    """The contract's named cases, value by value: NaN passes through, -0 stays -0 against lo = +0, sign(0) = 0, sign(NaN) = NaN."""
    xa = np.array([np.nan, -0.0, 0.5, 0.5, -3.0, 7.0, 0.0, 1.0, np.inf, -np.inf, -0.0], F)
    g = np.array([1.0, 1.0, np.nan, 0.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, np.nan], F)
    got = torch.from_numpy(xa).to(gpu)
    pkg.ops.pgd_step_clamp_(got, None, 0.0)
    out = got.cpu().numpy()
    assert np.isnan(out[0]) and np.signbit(out[1]) and out[1] == 0 and np.signbit(out[10])
    np.testing.assert_array_equal(out[2:10], np.array([0.5, 0.5, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0], F))
    got = torch.from_numpy(xa).to(gpu)
    pkg.ops.pgd_step_clamp_(got, torch.from_numpy(g).to(gpu), 0.25)
    out = got.cpu().numpy()
    assert np.isnan(out[0]) and np.isnan(out[2]) and np.isnan(out[10])
    np.testing.assert_array_equal(out[[1, 3, 4, 5, 6, 7, 8, 9]], np.array([0.25, 0.5, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0], F))


def test_channels_last_batch(pkg, gpu, c_oracle):
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(-0.2, 1.2, (2, 3, 32, 32)).astype(F)).to(gpu).contiguous(memory_format=torch.channels_last)
    xa = (x + torch.from_numpy(rng.uniform(-0.02, 0.02, (2, 3, 32, 32)).astype(F)).to(gpu)).contiguous(memory_format=torch.channels_last)
    g = torch.from_numpy(rng.standard_normal((2, 3, 32, 32)).astype(F)).to(gpu).contiguous(memory_format=torch.channels_last)
    assert not xa.is_contiguous() and xa.is_contiguous(memory_format=torch.channels_last)
    for gdt in (torch.float32, torch.bfloat16):
        gg = g.to(gdt)
        comp, sh_c = xa.clone(), torch.empty_like(xa, dtype=torch.bfloat16)
        pkg.ops.pgd_step_(comp, gg, float(GAMMA), x, float(EPS), True, sh_c)
        pkg.ops.tensor_clamp_(comp, torch.zeros_like(comp), torch.ones_like(comp))
        got, sh = xa.clone(), torch.empty_like(xa, dtype=torch.bfloat16)
        pkg.pgd.step(got, gg, float(GAMMA), x, float(EPS), True, shadow=sh, clamp=(0.0, 1.0))
        assert got.stride() == xa.stride() and torch.equal(got, comp)
        assert torch.equal(sh, comp.to(torch.bfloat16))
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and float((got - xa).abs().max()) > 0
        # a gradient in the other memory order is brought to x_adv's, as pgd.step does for the plain step
        got2 = xa.clone()
        pkg.pgd.step(got2, gg.contiguous(), float(GAMMA), x, float(EPS), True, clamp=(0.0, 1.0))
        assert torch.equal(got2, comp)
    with pytest.raises(ValueError, match="layout"):
        pkg.ops.pgd_step_clamp_(xa.clone(), g.contiguous(), float(GAMMA))


def test_error_returns(pkg):
    """The export's argument errors, returned before anything is launched (host pointers: nothing is dereferenced)."""
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd, odd2 = ctypes.c_void_p(p.value + 1), ctypes.c_void_p(p.value + 2)
    f = lib.afan_pgd_step_clamp
    assert f(p, p, 0, None, None, 0, 0.1, 0.1, 0, 0.0, 1.0, None) == 0            # n == 0: no launch
    assert f(None, None, 9, None, None, 0, 0.1, 0.1, 1, 0.0, 1.0, None) == 0      # ... whatever else is passed
    assert f(p, p, 0, None, None, -1, 0.1, 0.1, 0, 0.0, 1.0, None) == -3          # AFAN_ESHAPE
    assert f(None, p, 0, None, None, 4, 0.1, 0.1, 0, 0.0, 1.0, None) == -4        # AFAN_ENULL: x_adv
    assert f(p, p, 0, None, None, 4, 0.1, 0.1, 1, 0.0, 1.0, None) == -4           # AFAN_ENULL: clip without x_clean
    assert f(p, None, 0, None, None, 4, 0.1, 0.1, 1, 0.0, 1.0, None) == -4        # ... also without a gradient
    assert f(p, p, 7, None, None, 4, 0.1, 0.1, 0, 0.0, 1.0, None) == -1           # AFAN_EDTYPE with a gradient
    assert f(p, p, -1, p, None, 4, 0.1, 0.1, 1, 0.0, 1.0, None) == -1
    assert f(odd, p, 0, None, None, 4, 0.1, 0.1, 0, 0.0, 1.0, None) == -2         # AFAN_EALIGN: x_adv
    assert f(p, odd2, 0, None, None, 4, 0.1, 0.1, 0, 0.0, 1.0, None) == -2        # an fp32 gradient on a 2-byte boundary
    assert f(p, odd, 1, None, None, 4, 0.1, 0.1, 0, 0.0, 1.0, None) == -2         # a bf16 gradient on an odd byte
    assert f(p, p, 0, odd2, None, 4, 0.1, 0.1, 1, 0.0, 1.0, None) == -2           # x_clean
    assert f(p, p, 0, None, odd, 4, 0.1, 0.1, 0, 0.0, 1.0, None) == -2            # shadow
    assert f(odd, None, 0, None, None, 4, 0.1, 0.1, 0, 0.0, 1.0, None) == -2      # without a gradient too


def test_wrapper_checks(pkg, gpu):
    ops = pkg.ops
    xa = torch.zeros(8, device=gpu)
    with pytest.raises(pkg.AfanLibraryError):
        ops.pgd_step_clamp_(torch.zeros(4), torch.zeros(4), 0.1)                   # CPU tensors: no CPU path
    with pytest.raises(TypeError):
        ops.pgd_step_clamp_(xa, torch.zeros(8, device=gpu, dtype=torch.float16), 0.1)
    with pytest.raises(TypeError):
        ops.pgd_step_clamp_(xa, torch.zeros(4, device=gpu), 0.1)
    with pytest.raises(TypeError):
        ops.pgd_step_clamp_(xa.double(), None, 0.1)
    with pytest.raises(TypeError):
        ops.pgd_step_clamp_(xa, None, 0.1, None, 0.1, True)                        # clip without x_clean
    with pytest.raises(ValueError):
        ops.pgd_step_clamp_(xa, None, 0.1, torch.zeros(4, device=gpu), 0.1, True)
    with pytest.raises(TypeError):
        ops.pgd_step_clamp_(xa, None, 0.1, shadow=torch.zeros(8, device=gpu))     # the shadow is bf16
    empty = torch.zeros(0, device=gpu)
    assert ops.pgd_step_clamp_(empty, torch.zeros(0, device=gpu), 0.1) is empty


def test_pgd_step_refuses_clamp_outside_the_linf_step(pkg, gpu):
    xa, g, x = torch.zeros(2, 8, device=gpu), torch.ones(2, 8, device=gpu), torch.zeros(2, 8, device=gpu)
    with pytest.raises(ValueError, match="clamp"):
        pkg.pgd.step(xa, g, 0.1, x, 0.2, True, norm="l2", clamp=(0.0, 1.0))
    with pytest.raises(ValueError, match="clamp"):
        pkg.pgd.step(xa, g, 0.1, x, 0.2, True, norms=True, clamp=(0.0, 1.0))
    with pytest.raises(ValueError, match="norm must be"):
        pkg.pgd.step(xa, g, 0.1, x, 0.2, True, norm="l1", clamp=(0.0, 1.0))
    assert float(xa.abs().max()) == 0.0                                            # nothing was launched
    assert pkg.pgd.step(xa, g, 0.25, x, 0.2, True, clamp=(0.0, 0.125)) is None
    assert torch.equal(xa, torch.full_like(xa, 0.125))
    # every existing caller keeps its launches: clamp01_ is still the composition
    before = dict(pkg.ops.CALLS.other)
    pkg.pgd.clamp01_(xa)
    assert pkg.ops.CALLS["tensor_clamp"] == before["tensor_clamp"] + 1 and pkg.ops.CALLS["pgd_step_clamp"] == before["pgd_step_clamp"]
