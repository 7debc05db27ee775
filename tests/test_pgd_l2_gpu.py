"""afan_pgd_step_l2 (csrc/afan_pgd.hip) through the C ABI with ctypes: the normalised-gradient L2 step, the projection onto the L2
ball, the projection-only form, the shadow and the two norm outputs.

Conventions (tests/test_update_pinned_gpu.py's): every buffer is its own allocation with a 256-byte guard band on both sides, all of
it pre-filled with the byte 0xA5, and after the call every guard band is intact; misalignment is a byte offset into that
allocation; fp32 and bf16 results are compared as bit patterns, any NaN equal to any NaN.  Each case prints "L2PIN <case>" and its
figures (run with -s) before it asserts.

Every case is held to two things:
  (a) gnorm_out and dnorm_out lie in the counted window (tests/pgd_l2_refs.py: C_G, C_D roundings per term, the step's own error
      for dnorm) of the float64 formula computed on the CPU;
  (b) given the kernel's OWN norms, x_adv and the shadow equal the fp32 restatement (pgd_l2_refs.step_l2) in every bit.  dnorm_out
      is min(nd, eps) under clip, so nd itself is read from a call with clip = 0 on equal inputs and the same pointers' alignment
      (launches 1 and 2 are the same kernels on the same data: the same sums), which also pins the unclipped iterate.
The clipped call then runs twice on equal inputs: every output has the same bits both times (the sums are deterministic).

Tables: xc Gaussian, x_adv = xc + a perturbation of norm 0.3 eps (sample inside) or 3 eps (outside) in turn, gamma = eps / 4, so that
in the float64 reference every sample ends below 0.9 eps or above 1.1 eps (asserted per case: no case depends on the branch at the
ball's edge, none is left out).  per_sample in {1, 3, 4, 5, 7, 8, 9, 63, 64, 257, 3072}; 4097 (two chunks, the scalar loop's second
trip), 4100 (the float4 body's; a bf16 gradient's 8-wide body refuses it and runs scalar beside the float4 projection), 4104 (the
8-wide body's); batch in {1, 2, 5}; fp32 and bf16 gradients; with and without the shadow; clip on and off (off without the shadow:
no x_clean, no dnorm_out); the projection-only form; one case of 256 * 4096 + 8 elements (the second trip of the chain over a
sample's partials); a 4-byte (bf16: 2-byte) offset of each pointer in turn; the edge, zero-gradient, NaN-gradient and empty cases.

On an MI355X every case passes.  The module's 456 cases take 3.9 s in all when run alone: the first (which loads the library) 0.37 s,
the wrapper case 0.38 s, the 1 M-element case 0.26 s and every other case 0.02 s or less.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pgd_l2_refs as L

pytestmark = pytest.mark.gpu

F = np.float32
U16 = np.uint16
F32, BF16 = 0, 1
GN = {F32: "f32", BF16: "bf16"}
SENT, GUARD = 0xA5, 256
EPS, GAMMA = F(0.5), F(0.125)
SIZES = (1, 3, 4, 5, 7, 8, 9, 63, 64, 257, 3072, 4097, 4100, 4104)
BIG = 256 * L.L2_CHUNK + 8
PTRS = ("x_adv", "grad", "x_clean", "shadow", "workspace", "gnorm", "dnorm")


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """nbytes of device memory `off` bytes past a 256-byte boundary, a guard band on both sides, all of it filled with SENT."""

    def __init__(self, dev, nbytes, off=0, init=None):
        self.raw = torch.full((GUARD + off + nbytes + GUARD,), SENT, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.lo, self.n = GUARD + off, nbytes
        if init is not None:
            a = np.ascontiguousarray(init)
            assert a.nbytes == nbytes, (a.nbytes, nbytes)
            self.raw[self.lo:self.lo + nbytes].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))

    def p(self):
        return ctypes.c_void_p(self.raw.data_ptr() + self.lo)

    def get(self, dt):
        return self.raw[self.lo:self.lo + self.n].cpu().numpy().view(dt)

    def guards_ok(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.lo + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.raw == SENT).all())


def P(b):
    return None if b is None else b.p()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


# -------------------------------------------------------------------------------------------------------------------------- tables
@functools.lru_cache(maxsize=None)
def table(batch, per, gdt, seed=0):
    """(x_adv, grad as fp32 values, grad as stored, x_clean), [batch, per]."""
    rng = np.random.default_rng(1000 * per + 10 * batch + gdt + seed)
    xc = rng.standard_normal((batch, per)).astype(F)
    dl = rng.standard_normal((batch, per))
    scale = np.array([3.0 if (b + per) % 2 else 0.3 for b in range(batch)]) * float(EPS)
    dl *= (scale / np.sqrt((dl * dl).sum(axis=1)))[:, None]
    xa = (xc + dl).astype(F)
    g = rng.standard_normal((batch, per)).astype(F)
    gs = g
    if gdt == BF16:
        gs = L.bf16_bits(g)
        g = L.bf16_widen(gs)
    for a in (xa, g, gs, xc):
        a.setflags(write=False)
    return xa, g, gs, xc


class Run:
    """One call of afan_pgd_step_l2 on fresh guarded buffers."""

    def __init__(self, lib, dev, xa, gs, gdt, xc, shadow, clip, gamma, eps, want_g=True, want_d=True, offs=None, ws_floats=None):
        offs = offs or {}
        b, per = xa.shape
        o = lambda name: offs.get(name, 0)
        self.xa = Buf(dev, xa.nbytes, o("x_adv"), xa)
        self.g = None if gs is None else Buf(dev, gs.nbytes, o("grad"), gs)
        self.xc = None if xc is None else Buf(dev, xc.nbytes, o("x_clean"), xc)
        self.sh = Buf(dev, 2 * b * per, o("shadow")) if shadow else None
        nws = int(lib.afan_pgd_step_l2_workspace_floats(b, per)) if ws_floats is None else ws_floats
        assert nws == L.workspace_floats(b, per) or ws_floats is not None
        self.ws = Buf(dev, 4 * max(nws, 1), o("workspace"))
        self.gn = Buf(dev, 4 * max(b, 1), o("gnorm")) if want_g else None
        self.dn = Buf(dev, 4 * max(b, 1), o("dnorm")) if want_d else None
        self.shape = (b, per)
        self.rc = lib.afan_pgd_step_l2(P(self.xa), P(self.g), gdt, P(self.xc), P(self.sh), b, per, float(gamma), float(eps),
                                       int(clip), P(self.ws), P(self.gn), P(self.dn), _st())
        torch.cuda.synchronize()

    def bufs(self):
        return [x for x in (self.xa, self.g, self.xc, self.sh, self.ws, self.gn, self.dn) if x is not None]

    def x(self):
        return self.xa.get(F).reshape(self.shape)

    def shadow(self):
        return self.sh.get(U16).reshape(self.shape)

    def gnorm(self):
        return self.gn.get(F)[:self.shape[0]]

    def dnorm(self):
        return self.dn.get(F)[:self.shape[0]]


def _in_window(got, want64, win):
    got = np.asarray(got, np.float64)
    return bool(np.all((np.abs(got - want64) <= win) | (np.isnan(got) & np.isnan(want64))))


def check(lib, dev, what, xa, g, gs, gdt, xc, shadow, clip, offs=None, gamma=GAMMA, eps=EPS, margins=True):
    """Conditions (a) and (b) and the determinism of one case; returns the clipped (or only) run."""
    print(f"L2PIN {what}")
    b, per = xa.shape
    fails = []
    have_xc = xc is not None
    r64 = L.step_l2_f64(xa, g, xc, gamma, eps, clip)
    if margins and have_xc:
        nd64 = r64["nd"]
        ok = (nd64 < 0.9 * float(eps)) | (nd64 > 1.1 * float(eps)) | np.isnan(nd64)
        assert ok.all(), f"{what}: a sample of the table sits within 10 % of the ball's edge: {nd64 / float(eps)}"
    # the unclipped call: ng, nd and the stepped iterate
    free = Run(lib, dev, xa, gs, gdt, xc, shadow, False, gamma, eps, want_d=have_xc, offs=offs)
    runs = [free]
    if free.rc != 0:
        pytest.fail(f"{what}: the unclipped call returned {free.rc}")
    ng = free.gnorm()
    nd = free.dnorm() if have_xc else None
    stepped = (ng != 0) if g is not None else np.zeros(b, bool)
    gwin = L.norm_window(r64["ng"], L.c_g(per), per)
    print(f"  gnorm {ng[:5]} float64 {r64['ng'][:5]} window {gwin[:5]}")
    if not _in_window(ng, r64["ng"], gwin):
        fails.append(f"gnorm outside its window: {ng} vs {r64['ng']} +- {gwin}")
    if have_xc:
        dwin = L.dnorm_window(r64["nd"], np.sqrt((r64["x_new"] ** 2).sum(axis=1)), gamma, per, stepped)
        print(f"  nd {nd[:5]} float64 {r64['nd'][:5]} window {dwin[:5]}")
        if not _in_window(nd, r64["nd"], dwin):
            fails.append(f"dnorm (clip = 0) outside its window: {nd} vs {r64['nd']} +- {dwin}")
    want, want_sh = L.step_l2(xa, g, xc, gamma, eps, False, ng, nd)
    i = L.same_f32(free.x(), want)
    if i is not None:
        fails.append(f"clip = 0: x_adv differs from the restatement at {i}: {free.x().ravel()[i]!r} vs {want.ravel()[i]!r}")
    if shadow and L.same_bf16(free.shadow(), want_sh) is not None:
        fails.append("clip = 0: the shadow differs from the restatement")
    last = free
    if clip:
        one = Run(lib, dev, xa, gs, gdt, xc, shadow, True, gamma, eps, offs=offs)
        two = Run(lib, dev, xa, gs, gdt, xc, shadow, True, gamma, eps, offs=offs)
        runs += [one, two]
        if one.rc != 0 or two.rc != 0:
            pytest.fail(f"{what}: the clipped call returned {one.rc}, {two.rc}")
        want, want_sh = L.step_l2(xa, g, xc, gamma, eps, True, ng, nd)
        with np.errstate(invalid="ignore"):
            want_dn = np.where(nd > eps, eps, nd).astype(F)
            dn64 = np.where(r64["nd"] > float(eps), float(eps), r64["nd"])
        print(f"  dnorm {one.dnorm()[:5]} float64 {dn64[:5]}")
        if L.same_f32(one.gnorm(), ng) is not None:
            fails.append("gnorm differs between the clipped and the unclipped call")
        if L.same_f32(one.dnorm(), want_dn) is not None:
            fails.append(f"dnorm is not min(nd, eps) of the unclipped call's nd: {one.dnorm()} vs {want_dn}")
        if not _in_window(one.dnorm(), dn64, dwin):
            fails.append(f"dnorm outside its window: {one.dnorm()} vs {dn64} +- {dwin}")
        i = L.same_f32(one.x(), want)
        if i is not None:
            fails.append(f"x_adv differs from the restatement at {i}: {one.x().ravel()[i]!r} vs {want.ravel()[i]!r}")
        if shadow and L.same_bf16(one.shadow(), want_sh) is not None:
            fails.append("the shadow differs from the restatement")
        same = L.same_f32(one.x(), two.x()) is None and L.same_f32(one.gnorm(), two.gnorm()) is None \
            and L.same_f32(one.dnorm(), two.dnorm()) is None and (not shadow or L.same_bf16(one.shadow(), two.shadow()) is None)
        if not same:
            fails.append("two calls on equal inputs differ")
        last = one
    for r in runs:
        for k, bf in enumerate(r.bufs()):
            if not bf.guards_ok():
                fails.append(f"the guard band of buffer {k} was written")
        if r.g is not None and not np.array_equal(r.g.get(np.uint8), np.ascontiguousarray(gs).reshape(-1).view(np.uint8)):
            fails.append("the gradient was written")
        if r.xc is not None and not np.array_equal(r.xc.get(F), np.asarray(xc).ravel()):
            fails.append("x_clean was written")
    assert not fails, f"{what}:\n  " + "\n  ".join(fails[:12])
    return last


# ------------------------------------------------------------------------------------------------------------------- the main table
@pytest.mark.parametrize("shadow", [False, True], ids=["noshadow", "shadow"])
@pytest.mark.parametrize("clip", [False, True], ids=["free", "clip"])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("per", SIZES)
def test_step(lib, gpu, per, batch, gdt, clip, shadow):
    xa, g, gs, xc = table(batch, per, gdt)
    bare = not clip and not shadow                       # no x_clean, no dnorm_out: two launches, nothing read but x_adv and grad
    check(lib, gpu, f"step per{per} b{batch} {GN[gdt]} clip{int(clip)} shadow{int(shadow)}", xa, g, gs, gdt, None if bare else xc, shadow, clip)


@pytest.mark.parametrize("shadow", [False, True], ids=["noshadow", "shadow"])
@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("per", SIZES)
def test_projection_only(lib, gpu, per, batch, shadow):
    xa, _, _, xc = table(batch, per, F32)
    r = check(lib, gpu, f"proj per{per} b{batch} shadow{int(shadow)}", xa, None, None, F32, xc, shadow, True)
    assert not r.gnorm().any()                            # no gradient: gnorm_out reads 0
    inside = np.array([not (b + per) % 2 for b in range(batch)])
    assert L.same_f32(r.x()[inside], xa[inside]) is None  # a sample inside the ball keeps its bits


def test_many_chunks(lib, gpu):
    """More than 256 chunks in a sample: the second trip of every thread's chain over the partials."""
    xa, g, gs, xc = table(1, BIG, F32)
    assert L.chunks_of(BIG) == 257 and L.c_g(BIG) == L.c_g(4096) + 1
    check(lib, gpu, f"step per{BIG} b1 f32 clip1 shadow1", xa, g, gs, F32, xc, True, True)
    xa, g, gs, xc = table(2, BIG, BF16)
    check(lib, gpu, f"step per{BIG} b2 bf16 clip1 shadow0", xa, g, gs, BF16, xc, False, True)


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("which", PTRS)
def test_misaligned_pointer(lib, gpu, which, gdt):
    """Each pointer in turn one element off a 16-byte boundary: the scalar bodies (or, for the small outputs, nothing) take it."""
    per, batch = 4104, 2
    xa, g, gs, xc = table(batch, per, gdt, seed=1)
    off = 2 if (which == "shadow" or (which == "grad" and gdt == BF16)) else 4
    check(lib, gpu, f"misaligned {which}+{off} {GN[gdt]}", xa, g, gs, gdt, xc, True, True, offs={which: off})


@pytest.mark.parametrize("which", PTRS)
def test_pointer_off_its_element_is_refused(lib, gpu, which):
    xa, g, gs, xc = table(2, 64, BF16 if which == "grad" else F32)
    off = 1 if which in ("shadow", "grad") else 2
    r = Run(lib, gpu, xa, gs, BF16 if which == "grad" else F32, xc, True, True, GAMMA, EPS, offs={which: off})
    assert r.rc == -2                                      # AFAN_EALIGN, before any launch
    assert r.sh.untouched() and r.ws.untouched() and r.gn.untouched() and r.dn.untouched() and np.array_equal(r.x(), xa)


# ----------------------------------------------------------------------------------------------------------------- the special cases
@pytest.mark.parametrize("form", ["projection", "zero_gradient"])
@pytest.mark.parametrize("per", [5, 8, 4100])
def test_edge_of_the_ball(lib, gpu, per, form):
    """One non-zero element: |d| == eps stays inside and keeps its bits, |d| == nextafter(eps) is projected (sums of one term are
    exact and sqrt(fl(d * d)) == |d|, so neither sample's branch depends on rounding)."""
    up = np.nextafter(EPS, F(np.inf))
    xa = np.zeros((3, per), F)
    xa[0, per // 2], xa[1, per - 1], xa[2, 0] = EPS, -up, -EPS
    xc = np.zeros_like(xa)
    g = None if form == "projection" else np.zeros_like(xa)
    r = check(lib, gpu, f"edge {form} per{per}", xa, g, g, F32, xc, True, True, margins=False)
    assert L.same_f32(r.x()[[0, 2]], xa[[0, 2]]) is None
    assert r.x()[1, per - 1] == -EPS and not r.x()[1, :per - 1].any()
    assert L.same_f32(r.dnorm(), np.array([EPS, EPS, EPS], F)) is None and not r.gnorm().any()
    free = Run(lib, gpu, xa, g, F32, xc, False, False, GAMMA, EPS)
    assert L.same_f32(free.dnorm(), np.array([EPS, up, EPS], F)) is None


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("per", [7, 64, 4104])
def test_zero_and_nan_gradient_samples(lib, gpu, per, gdt):
    """Sample 1 has a zero gradient (with a -0.0): its bits stay, gnorm == 0.  Sample 3 has one NaN in its gradient: it becomes NaN
    through the formulas; samples 0, 2 and 4 beside them equal the restatement in every bit (check's condition (b))."""
    xa, g, gs, xc = (np.array(a, copy=True) for a in table(5, per, gdt, seed=2))
    g[1], gs[1] = 0, 0
    g[1, 0] = F(-0.0)
    gs[1, 0] = 0x8000 if gdt == BF16 else F(-0.0)
    g[3, per // 2] = np.nan
    gs[3, per // 2] = 0x7fc0 if gdt == BF16 else np.nan
    xa[1, per - 1] = F(-0.0)
    r = check(lib, gpu, f"zero/NaN gradient per{per} {GN[gdt]}", xa, g, gs, gdt, xc, True, False, margins=False)
    assert r.gnorm()[1] == 0 and np.isnan(r.gnorm()[3]) and np.isnan(r.x()[3]).all() and np.isnan(r.dnorm()[3])
    assert L.same_f32(r.x()[1], xa[1]) is None and np.signbit(r.x()[1, per - 1])
    assert np.isfinite(r.x()[[0, 2, 4]]).all()
    proj = check(lib, gpu, f"zero/NaN gradient per{per} {GN[gdt]} clip", xa, g, gs, gdt, xc, True, True, margins=False)
    assert np.isnan(proj.x()[3]).all() and np.isfinite(proj.x()[[0, 1, 2, 4]]).all()


def test_empty_and_argument_errors(lib, gpu):
    xa, g, gs, xc = table(2, 8, F32)
    for b, per in ((0, 8), (2, 0), (0, 0)):
        bufs = [Buf(gpu, 64) for _ in range(7)]
        rc = lib.afan_pgd_step_l2(*[P(x) for x in bufs[:2]], F32, *[P(x) for x in bufs[2:4]], b, per, 0.1, 0.1, 1, *[P(x) for x in bufs[4:]], _st())
        torch.cuda.synchronize()
        assert rc == 0 and all(x.untouched() for x in bufs), (b, per)
    assert lib.afan_pgd_step_l2_workspace_floats(0, 8) == 0 and lib.afan_pgd_step_l2_workspace_floats(5, 4097) == 20
    bufs = [Buf(gpu, 64) for _ in range(7)]
    p = [P(x) for x in bufs]
    call = lambda xa_, g_, dt, xc_, sh_, b, per, clip, ws_, gn_, dn_: lib.afan_pgd_step_l2(xa_, g_, dt, xc_, sh_, b, per, 0.1, 0.1, clip, ws_, gn_, dn_, _st())
    assert call(p[0], p[1], F32, p[2], p[3], -1, 4, 1, p[4], p[5], p[6]) == -3          # AFAN_ESHAPE
    assert call(p[0], p[1], F32, p[2], p[3], 1, -4, 1, p[4], p[5], p[6]) == -3
    assert call(p[0], p[1], F32, p[2], p[3], 1 << 40, 1 << 40, 1, p[4], p[5], p[6]) == -3
    assert call(None, p[1], F32, p[2], p[3], 1, 4, 1, p[4], p[5], p[6]) == -4            # AFAN_ENULL
    assert call(p[0], p[1], F32, p[2], p[3], 1, 4, 1, None, p[5], p[6]) == -4
    assert call(p[0], p[1], F32, None, p[3], 1, 4, 1, p[4], p[5], None) == -4            # clip without x_clean
    assert call(p[0], p[1], F32, None, p[3], 1, 4, 0, p[4], p[5], p[6]) == -4            # dnorm_out without x_clean
    assert call(p[0], p[1], 7, p[2], p[3], 1, 4, 1, p[4], p[5], p[6]) == -1              # AFAN_EDTYPE
    torch.cuda.synchronize()
    assert all(x.untouched() for x in bufs)


def test_ops_wrapper_and_l2ball_proj(pkg, gpu):
    """ops.pgd_step_l2_ on a channels-last tensor (sample b is the block at b * per_sample in either layout) equals the C entry on
    the same memory; attack_algo.l2ball_proj is its projection-only form under the reference's signature."""
    torch.manual_seed(3)
    x = torch.randn(3, 4, 5, 6, device=gpu).contiguous(memory_format=torch.channels_last)
    gr = torch.randn(3, 4, 5, 6, device=gpu).contiguous(memory_format=torch.channels_last)
    scale = torch.tensor([0.1, 4.0, 0.1], device=gpu).view(3, 1, 1, 1)
    xa = (x + scale * float(EPS) * torch.nn.functional.normalize(torch.randn_like(x).flatten(1), dim=1).view_as(x)).contiguous(memory_format=torch.channels_last)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(3, -1).cpu().numpy()
    sh = torch.empty_like(xa, dtype=torch.bfloat16)
    out, gn, dn = pkg.ops.pgd_step_l2_(xa.clone(memory_format=torch.preserve_format), gr, float(GAMMA), x, float(EPS), True, sh, want_norms=True)
    free = pkg.ops.pgd_step_l2_(xa.clone(memory_format=torch.preserve_format), gr, float(GAMMA), x, float(EPS), False, None, want_norms=True)
    want, want_sh = L.step_l2(flat(xa), flat(gr), flat(x), GAMMA, EPS, True, gn.cpu().numpy(), free[2].cpu().numpy())
    assert L.same_f32(flat(out), want) is None and L.same_bf16(flat(sh.view(torch.int16)).view(U16), want_sh) is None
    assert dn.cpu().numpy()[1] == EPS and (dn.cpu().numpy()[[0, 2]] < 0.9 * EPS).all()
    t = xa.clone(memory_format=torch.preserve_format)
    res = pkg.attack_algo.l2ball_proj(x, float(EPS), t, in_place=False)
    assert res is not t and torch.equal(t, xa)
    nd = pkg.ops.pgd_step_l2_(xa.clone(memory_format=torch.preserve_format), None, 0.0, x, 0.0, False, None, want_norms=True)[2]
    want, _ = L.step_l2(flat(xa), None, flat(x), 0.0, EPS, True, None, nd.cpu().numpy())
    assert L.same_f32(flat(res), want) is None
    assert pkg.attack_algo.l2ball_proj(x, float(EPS), t) is t and torch.equal(t, res)
    zero = x.clone(memory_format=torch.preserve_format)
    assert torch.equal(pkg.attack_algo.l2ball_proj(x, float(EPS), zero), x)            # a zero perturbation stays zero
    with pytest.raises(pkg.ops.AfanLibraryError):
        pkg.ops.pgd_step_l2_(xa.cpu(), gr.cpu(), 0.1)
