"""The kernels that write the model's state on every step, pinned BIT FOR BIT: the PGD sign step, the fused step + norms, the noise,
clamp, cast and start of csrc/afan_pgd.hip, the SGD update (plain and guarded) and the guarded copy of csrc/afan_sgd.hip, and the
KRSC -> CRSK weight transpose at the end of csrc/afan_conv.hip.  Every arithmetic step of these kernels is one correctly rounded fp32
operation (-ffp-contract=off) or a copy, so the references of tests/update_pinned_refs.py (np.float32, one numpy operation per
rounding; tests/test_update_pinned_ref.py checks them on the CPU against the C oracle and torch) are met in every bit.  The only
tolerance is the l2 window of the norms, taken unchanged from tests/test_tail_pinned_gpu.py (c_norm_ss).

Conventions: every kernel is called through the C ABI with ctypes; every buffer is its own allocation with a 256-byte guard band on
both sides, pre-filled (outputs and guard bands alike) with the byte 0xA5, and after the call every guard band is intact.
Misalignment is a byte offset into that allocation (4 bytes for fp32, 2 or 4 or 8 for bf16), which the entry either accepts on its
scalar path or refuses with a return code before any launch.  fp32 and bf16 results are compared as bit patterns, any NaN equal to any
NaN.  Each case prints "UPDPIN <form> <case>" (run with -s) before it asserts.

Sizes: T4, T8 and T1 (update_pinned_refs) are the smallest at which the float4, 8-wide and scalar grid-stride loops make a second
trip under grid_for's cap of 2048 workgroups; every other case has at most a few thousand elements, and the kernels with a vector
body and a tail see n in {1, 3, 4, 5, 7, 8, 9, 63, 64, 257}.  Random operands are Gaussian with special values laid over the first
elements (the vector body) and the last (the ragged tail): gradient +0, -0, NaN, +-inf, iterate NaN and -0, iterates exactly on and
one ulp either side of both edges of the ball.  Subnormals are left out of every table: the build's float mode is not what this
module pins, and no tensor on the training path holds them.

The fused step + norms is held to three things per case: x_adv and the shadow have the bits of afan_pgd_step on the same inputs (and
of the reference); linf equals the reference; l2 lies in the derived window AND has the bits of afan_perturb_norms on the stepped
tensor: the two are one template with the same order of operations, so equality is the derived expectation.  (Its scalar cases
misalign x_adv or take per_sample % 4 != 0, which sends afan_perturb_norms down its scalar path too; a misaligned gradient alone would
leave the two on different summation orders.)

The transpose reads sources whose elements are an arange of uint16 patterns (it wraps at 65 536: an element misplaced by a multiple
of that would not show, any other does) and is compared over the whole destination allocation, so that every element no descriptor
owns (the gaps, slot 9 of a shared operand when only the 3x3 was given) still holds the fill.

Coverage: EXPECTED_VARIANTS lists every instantiation and inner path the tables must reach; tests/test_update_pinned_ref.py holds the
test that the dispatch predicates restated in tests/update_pinned_refs.py map the tables onto exactly that list.

On an MI355X every case passes: no kernel differs from its reference in any bit.  The module's 215 GPU cases take 5.0 s in all when run
alone; the slowest kernel case takes 0.27 s (the module's first, which loads the library) and the T4 / T8 cases 0.03 to 0.17 s; the
case above the ABI, which builds a model, an arena and an optimizer, takes 1.5 s when it is the process's first use of them and under 1.3 s within the whole suite.
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_tail_pinned_gpu as TG
import update_pinned_refs as R

pytestmark = pytest.mark.gpu

F = np.float32
U16 = np.uint16
F32, BF16 = 0, 1                    # AFAN_F32, AFAN_BF16
GN = {F32: "f32", BF16: "bf16"}
GB = {F32: 4, BF16: 2}
SENT = 0xA5
GUARD = 256
GAMMA, EPS = F(2.0 / 255), F(8.0 / 255)
Z4 = (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """nbytes of device memory `off` bytes past a 256-byte boundary, a guard band on both sides, all of it filled with SENT."""

    def __init__(self, dev, nbytes, off=0, init=None):
        self.raw = torch.full((GUARD + off + nbytes + GUARD,), SENT, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.lo, self.n = GUARD + off, nbytes
        if init is not None:
            self.put(init)

    def p(self, plus=0):
        return ctypes.c_void_p(self.raw.data_ptr() + self.lo + plus)

    def put(self, a):
        a = np.array(a, copy=True)
        assert a.nbytes == self.n, (a.nbytes, self.n)
        self.raw[self.lo:self.lo + self.n].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))

    def get(self, dt):
        return self.raw[self.lo:self.lo + self.n].cpu().numpy().view(dt)

    def guards_ok(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.lo + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.raw == SENT).all())


def P(b, plus=0):
    return None if b is None else b.p(plus)


class Report:
    def __init__(self, form, case):
        self.what, self.fails, self.bufs = f"{form} {case}", [], []
        print(f"UPDPIN {form} {case}")

    def buf(self, *a, **k):
        b = Buf(*a, **k)
        self.bufs.append(b)
        return b

    def expect(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def f32(self, name, got, want):
        i = R.same_f32(got, want)
        if i is not None:
            g, w = np.asarray(got, F).ravel(), np.asarray(want, F).ravel()
            self.expect(False, f"{name}: first difference at {i} of {g.size}: got {g[i]!r} ({g[i:i + 1].view(np.uint32)[0]:#010x}), "
                               f"expected {w[i]!r} ({w[i:i + 1].view(np.uint32)[0]:#010x})")

    def bf16(self, name, got, want):
        i = R.same_bf16(got, want)
        if i is not None:
            self.expect(False, f"{name}: first difference at {i} of {np.size(got)}: got {int(np.ravel(got)[i]):#06x}, expected {int(np.ravel(want)[i]):#06x}")

    def done(self):
        for k, b in enumerate(self.bufs):
            self.expect(b.guards_ok(), f"the guard band of buffer {k} was written")
        assert not self.fails, f"{self.what}:\n  " + "\n  ".join(self.fails[:12])


def offs_id(o):
    return "aligned" if not any(o) else "off" + ".".join(str(v) for v in o)


def overlay(arrays, rows, n):
    """Lay the special rows over the first elements and, where there is room, in the same order over the last (the ragged tail)."""
    k = min(len(rows), n)
    for i in range(k):
        for a, v in zip(arrays, rows[i]):
            a[i] = v
    if n >= 2 * len(rows):
        for i, r in enumerate(rows):
            for a, v in zip(arrays, r):
                a[n - len(rows) + i] = v


# ================================================================================================================== afan_pgd_step
def _step_specials(with_nan):
    c = F(0.75)
    lo, hi = F(c - EPS), F(c + EPS)
    nan, inf, up, dn = F(np.nan), F(np.inf), F(np.inf), F(-np.inf)
    h = F(0.5)
    #       x_adv                 grad      x_clean
    rows = [(lo, F(0), c), (np.nextafter(lo, dn), F(0), c), (np.nextafter(lo, up), F(0), c),
            (hi, F(0), c), (np.nextafter(hi, up), F(0), c), (np.nextafter(hi, dn), F(0), c),
            (h, F(0), h), (h, F(-0.0), h), (F(-0.0), F(0), F(0)), (h, inf, h), (h, -inf, h),
            (h, nan, h), (nan, F(1), h), (np.nextafter(lo, dn), F(-1), c)]
    return [r for r in rows if with_nan or not any(np.isnan(v) for v in r)]


@functools.lru_cache(maxsize=None)
def step_inputs(n, gdt, with_nan=True):
    """(x_adv, grad as fp32 values, grad as stored, x_clean): Gaussian, iterates up to 1.5 eps off the centre, the specials laid over
    (without the NaN rows for the norms tables, whose first and last sample would otherwise always be NaN)."""
    rng = np.random.default_rng(n * 2 + gdt)
    xc = rng.standard_normal(n).astype(F)
    xa = (xc + (EPS * rng.uniform(-1.5, 1.5, n).astype(F)).astype(F)).astype(F)
    g = rng.standard_normal(n).astype(F)
    overlay((xa, g, xc), _step_specials(with_nan), n)
    if gdt == BF16:
        gs = R.bf16_bits(g)
        g = R.bf16_widen(gs)
    else:
        gs = g
    return xa, g, gs, xc


SC = collections.namedtuple("SC", "gdt clip shadow n offs kind")
N_RAGGED = 4 * 257 + 3             # two workgroups of float4 work (the second nearly idle), five of scalar work, 3 ragged elements
STEP_CASES = []
for _g in (F32, BF16):
    for _clip in (1, 0):
        for _sh in (1, 0):
            STEP_CASES += [SC(_g, _clip, _sh, N_RAGGED, Z4, ""), SC(_g, _clip, _sh, N_RAGGED, (4, 0, 0, 0), "")]
    STEP_CASES += [SC(_g, 1, 1, _n, Z4, "") for _n in R.SMALL_N]
    STEP_CASES += [SC(_g, 1, 1, R.T4, Z4, ""), SC(_g, 1, 1, R.T1, (4, 0, 0, 0), "")]
# the scalar kernel by each term of the alignment predicate in turn (the x_adv term: the 16 forms above)
STEP_CASES += [SC(F32, 1, 1, N_RAGGED, (0, 4, 0, 0), ""), SC(BF16, 1, 1, N_RAGGED, (0, 2, 0, 0), ""), SC(BF16, 1, 1, N_RAGGED, (0, 4, 0, 0), ""),
               SC(F32, 1, 1, N_RAGGED, (0, 0, 4, 0), ""), SC(F32, 1, 1, N_RAGGED, (0, 0, 0, 2), ""),
               # a misaligned x_clean or shadow that the form does not read: still the float4 kernel
               SC(F32, 0, 0, N_RAGGED, (0, 0, 4, 2), ""),
               SC(F32, 0, 1, N_RAGGED, Z4, "null_clean"), SC(BF16, 0, 0, N_RAGGED, (4, 0, 0, 0), "null_clean"),
               SC(F32, 1, 1, N_RAGGED, Z4, "eps0"), SC(BF16, 1, 0, N_RAGGED, (4, 0, 0, 0), "eps0")]


def step_id(c):
    return f"{GN[c.gdt]}-clip{c.clip}-shadow{c.shadow}-n{c.n}-{offs_id(c.offs)}" + (f"-{c.kind}" if c.kind else "")


def step_labels(c):
    return R.step_tags(GN[c.gdt], GB[c.gdt], c.clip, c.shadow, c.n, c.offs, c.kind == "null_clean", c.kind == "eps0")


def run_step(rep, lib, dev, c, eps):
    """-> (rc, x_adv, shadow bits or None) of afan_pgd_step on step_inputs(c.n, c.gdt)."""
    xa, g, gs, xc = step_inputs(c.n, c.gdt)
    bxa, bg = rep.buf(dev, 4 * c.n, c.offs[0], xa), rep.buf(dev, GB[c.gdt] * c.n, c.offs[1], gs)
    bxc = None if c.kind == "null_clean" else rep.buf(dev, 4 * c.n, c.offs[2], xc)
    bsh = rep.buf(dev, 2 * c.n, c.offs[3]) if c.shadow else None
    rc = lib.afan_pgd_step(P(bxa), P(bg), c.gdt, P(bxc), P(bsh), c.n, float(GAMMA), float(eps), c.clip, _st())
    out = bxa.get(F), (bsh.get(U16) if bsh else None)
    rep.expect(np.array_equal(bg.get(U16), np.asarray(gs).view(U16)), "the gradient was written")
    if bxc is not None:
        rep.expect(R.same_f32(bxc.get(F), xc) is None, "x_clean was written")
    return (rc,) + out


@pytest.mark.parametrize("case", STEP_CASES, ids=step_id)
def test_pgd_step_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    form = sorted(t for t in step_labels(c) if t.startswith("pgd_step<"))[0]
    rep = Report(form, step_id(c))
    eps = F(0) if c.kind == "eps0" else EPS
    xa, g, _, xc = step_inputs(c.n, c.gdt)
    want = R.pgd_step(xa, g, xc, GAMMA, eps, c.clip)
    rc, got, sh = run_step(rep, lib, gpu, c, eps)
    rep.expect(rc == 0, f"afan_pgd_step returned {rc}")
    rep.f32("x_adv", got, want)
    if c.shadow:
        rep.bf16("shadow (RNE bf16 of the fp32 result)", sh, R.bf16_bits(want))
    if c.kind == "eps0":
        ok = np.isnan(want) | (want == xc)
        rep.expect(bool(ok.all()), "the reference itself: eps = 0 must return x_clean wherever the step is not NaN")
    rep.done()


# ============================================================================================================ afan_pgd_step_norms
NC = collections.namedtuple("NC", "gdt clip shadow batch per offs kind")
P_FIN_V, P_FIN_S = 65 * R.NORM_CHUNK + 4, 65 * R.NORM_CHUNK + 3            # 66 slices: the finalize wave's second trip
NORM_CASES = []
for _g in (F32, BF16):
    for _clip in (1, 0):
        for _sh in (1, 0):
            NORM_CASES += [NC(_g, _clip, _sh, 2, 4100, Z4, ""), NC(_g, _clip, _sh, 2, 4097, Z4, "")]
NORM_CASES += [NC(F32, 1, 1, 3, 1, Z4, ""), NC(F32, 1, 1, 3, 7, Z4, ""), NC(BF16, 1, 1, 2, 4096, Z4, ""), NC(F32, 1, 1, 3, 4097, Z4, ""),
               NC(F32, 1, 1, 3, 4100, Z4, ""), NC(F32, 1, 1, 3, 8, Z4, ""),
               NC(F32, 1, 1, 2, P_FIN_V, Z4, ""), NC(BF16, 1, 1, 2, P_FIN_S, Z4, ""),
               NC(F32, 1, 1, 2, 4096, (4, 0, 0, 0), ""),                   # a misaligned base: the scalar kernel at per_sample % 4 == 0
               NC(F32, 1, 1, R.MAX_BATCH, 1, Z4, ""), NC(BF16, 1, 1, R.MAX_BATCH, 4, Z4, ""),
               NC(F32, 1, 1, 3, 4100, Z4, "nan"), NC(BF16, 1, 0, 3, 4097, Z4, "nan")]


def norm_id(c):
    return f"{GN[c.gdt]}-clip{c.clip}-shadow{c.shadow}-{c.batch}x{c.per}-{offs_id(c.offs)}" + (f"-{c.kind}" if c.kind else "")


def norm_labels(c):
    return R.step_norms_tags(GN[c.gdt], GB[c.gdt], c.clip, c.shadow, c.batch, c.per, c.offs, c.kind == "nan")


@functools.lru_cache(maxsize=None)
def norm_inputs(batch, per, gdt, nan):
    xa, g, gs, xc = (np.array(a, copy=True) for a in step_inputs(batch * per, gdt, False))
    if nan:                          # one NaN gradient in sample 1, in the second slice
        g[per + per - 2] = np.nan
        gs = R.bf16_bits(g) if gdt == BF16 else g
    return xa, g, gs, xc


def l2_window(per, l2, ss):
    """The window of test_tail_pinned_gpu.test_perturb_norms_pinned; a sample without any perturbation has l2 = 0 exactly."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(l2 > 0, TG.U * (TG.c_norm_ss(per) * ss / (2 * l2) + l2), 0.0)


@pytest.mark.parametrize("case", NORM_CASES, ids=norm_id)
def test_pgd_step_norms_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    form = sorted(t for t in norm_labels(c) if t.startswith("step_norms<"))[0]
    rep = Report(form, norm_id(c))
    n = c.batch * c.per
    xa, g, gs, xc = norm_inputs(c.batch, c.per, c.gdt, c.kind == "nan")
    nws = int(lib.afan_norms_workspace_floats(c.batch, c.per))
    assert nws == R.norms_workspace_floats(c.batch, c.per)
    bxa, bg, bxc = rep.buf(gpu, 4 * n, c.offs[0], xa), rep.buf(gpu, GB[c.gdt] * n, c.offs[1], gs), rep.buf(gpu, 4 * n, c.offs[2], xc)
    bsh = rep.buf(gpu, 2 * n, c.offs[3]) if c.shadow else None
    ws, l2, li = rep.buf(gpu, 4 * nws), rep.buf(gpu, 4 * c.batch), rep.buf(gpu, 4 * c.batch)
    rc = lib.afan_pgd_step_norms(P(bxa), P(bg), c.gdt, P(bxc), P(bsh), c.batch, c.per, float(GAMMA), float(EPS), c.clip,
                                 P(ws), P(l2), P(li), _st())
    rep.expect(rc == 0, f"afan_pgd_step_norms returned {rc}")
    # 1: the bits of afan_pgd_step on the same inputs (and of the reference)
    pxa, pg, pxc = rep.buf(gpu, 4 * n, c.offs[0], xa), rep.buf(gpu, GB[c.gdt] * n, c.offs[1], gs), rep.buf(gpu, 4 * n, c.offs[2], xc)
    psh = rep.buf(gpu, 2 * n, c.offs[3]) if c.shadow else None
    rc = lib.afan_pgd_step(P(pxa), P(pg), c.gdt, P(pxc), P(psh), n, float(GAMMA), float(EPS), c.clip, _st())
    rep.expect(rc == 0, f"afan_pgd_step returned {rc}")
    want = R.pgd_step(xa, g, xc, GAMMA, EPS, c.clip)
    got = bxa.get(F)
    rep.f32("x_adv against the reference", got, want)
    rep.f32("x_adv against afan_pgd_step", got, pxa.get(F))
    if c.shadow:
        rep.bf16("shadow against the reference", bsh.get(U16), R.bf16_bits(want))
        rep.bf16("shadow against afan_pgd_step", bsh.get(U16), psh.get(U16))
    # 2: linf bit for bit
    linf, l2r, ss = R.perturb_norms(want.reshape(c.batch, c.per), xc.reshape(c.batch, c.per))
    rep.f32("linf", li.get(F), linf)
    # 3: l2 in the derived window, and the bits of afan_perturb_norms on the stepped tensor
    got2 = l2.get(F)
    nan = np.isnan(l2r)
    rep.expect(np.array_equal(np.isnan(got2), nan), f"l2 is NaN for samples {np.flatnonzero(np.isnan(got2)).tolist()[:8]}, expected {np.flatnonzero(nan).tolist()[:8]}")
    if c.kind == "nan":
        rep.expect(nan.tolist() == [False, True, False] and np.isnan(linf).tolist() == [False, True, False], "the reference: sample 1 alone is NaN")
    with np.errstate(invalid="ignore"):
        out = ~nan & ~np.isnan(got2) & ~(np.abs(got2.astype(np.float64) - l2r) <= l2_window(c.per, l2r, ss))
    rep.expect(not out.any(), f"l2 outside the window for samples {np.flatnonzero(out).tolist()[:8]}")
    ws2, l22, li2 = rep.buf(gpu, 4 * nws), rep.buf(gpu, 4 * c.batch), rep.buf(gpu, 4 * c.batch)
    rc = lib.afan_perturb_norms(P(bxa), P(bxc), c.batch, c.per, P(ws2), P(l22), P(li2), _st())
    rep.expect(rc == 0, f"afan_perturb_norms returned {rc}")
    assert R.norms_vec(c.per, c.offs[0], c.offs[2]) == (not R.step_norms_scalar_terms(GB[c.gdt], c.shadow, c.per, c.offs))
    rep.f32("l2 against afan_perturb_norms of the stepped tensor", got2, l22.get(F))
    rep.f32("linf against afan_perturb_norms of the stepped tensor", li.get(F), li2.get(F))
    # every workspace slot was written (a sum of squares or a maximum is never the negative fill), none beyond (the guard band)
    w = ws.get(np.uint32)
    rep.expect(not (w == 0xA5A5A5A5).any(), f"{int((w == 0xA5A5A5A5).sum())} of {nws} workspace floats were not written")
    rep.done()


def test_pgd_step_norms_refuses_batch_65536(pkg, gpu):
    lib = pkg._lib.load()
    rep = Report("step_norms|batch_refused", "65536x1")
    b = R.MAX_BATCH + 1
    bufs = [rep.buf(gpu, 4 * b) for _ in range(3)] + [rep.buf(gpu, 2 * b)] + [rep.buf(gpu, 4 * 2 * b), rep.buf(gpu, 4 * b), rep.buf(gpu, 4 * b)]
    xa, g, xc, sh, ws, l2, li = bufs
    rc = lib.afan_pgd_step_norms(P(xa), P(g), F32, P(xc), P(sh), b, 1, float(GAMMA), float(EPS), 1, P(ws), P(l2), P(li), _st())
    rep.expect(rc == R.AFAN_ESHAPE, f"returned {rc}, expected AFAN_ESHAPE")
    rc = lib.afan_perturb_norms(P(xa), P(xc), b, 1, P(ws), P(l2), P(li), _st())
    rep.expect(rc == R.AFAN_ESHAPE, f"afan_perturb_norms returned {rc}, expected AFAN_ESHAPE")
    rep.expect(all(x.untouched() for x in bufs), "a refused call wrote")
    rep.done()


# ================================================================================================================= afan_axpy_noise
ZC = collections.namedtuple("ZC", "shadow n offs")
NOISE_CASES = ([ZC(_s, _n, _o) for _s in (1, 0) for _n in (N_RAGGED,) for _o in ((0, 0, 0), (0, 4, 0))] +
               [ZC(1, _n, (0, 0, 0)) for _n in R.SMALL_N] + [ZC(1, N_RAGGED, (4, 0, 0)), ZC(1, N_RAGGED, (0, 0, 2)), ZC(0, N_RAGGED, (0, 0, 2)),
                                                             ZC(1, R.T4, (0, 0, 0)), ZC(0, R.T1, (4, 0, 0))])


def noise_id(c):
    return f"shadow{c.shadow}-n{c.n}-{offs_id(c.offs)}"


@functools.lru_cache(maxsize=None)
def noise_inputs(n):
    rng = np.random.default_rng(n + 17)
    xa, u = rng.standard_normal(n).astype(F), rng.random(n, dtype=F)
    overlay((xa, u), [(F(0.5), F(0)), (F(0.5), F(0.5)), (F(0.5), np.nextafter(F(1), F(0))), (F(-0.0), F(0.5))], n)
    return xa, u


@pytest.mark.parametrize("case", NOISE_CASES, ids=noise_id)
def test_axpy_noise_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    rep = Report(sorted(t for t in R.noise_tags(c.shadow, c.n, c.offs) if t.startswith("noise<"))[0], noise_id(c))
    xa, u = noise_inputs(c.n)
    bxa, bu = rep.buf(gpu, 4 * c.n, c.offs[0], xa), rep.buf(gpu, 4 * c.n, c.offs[1], u)
    bsh = rep.buf(gpu, 2 * c.n, c.offs[2]) if c.shadow else None
    rc = lib.afan_axpy_noise(P(bxa), P(bu), c.n, float(EPS), P(bsh), _st())
    rep.expect(rc == 0, f"afan_axpy_noise returned {rc}")
    want = R.axpy_noise(xa, u, EPS)
    rep.f32("x_adv", bxa.get(F), want)
    if c.shadow:
        rep.bf16("shadow", bsh.get(U16), R.bf16_bits(want))
    rep.expect(R.same_f32(bu.get(F), u) is None, "u was written")
    rep.done()


# =============================================================================================================== afan_tensor_clamp
CLAMP_CASES = [(_n, _o) for _n in (1, 3, 257, N_RAGGED) for _o in ((0, 0, 0),)] + [(N_RAGGED, (4, 4, 0)), (R.T1, (0, 0, 0))]


@functools.lru_cache(maxsize=None)
def clamp_inputs(n):
    rng = np.random.default_rng(n + 29)
    t, c = (rng.standard_normal(n) * 2).astype(F), rng.standard_normal(n).astype(F)
    lo, hi = (c - F(0.5)).astype(F), (c + F(0.5)).astype(F)
    nan = F(np.nan)
    #        t        lo       hi
    rows = [(F(0), F(1), F(-1)),      # lo > hi: the first `if` lifts t to lo = 1, the second takes it down to hi = -1
            (F(2), F(1), F(-1)), (F(-2), F(1), F(-1)), (nan, F(-1), F(1)), (F(-3), nan, F(1)), (F(3), nan, F(1)), (F(3), F(-1), nan),
            (F(-3), F(-1), nan), (F(-0.0), F(0), F(0)), (F(0), F(-0.0), F(-0.0))]
    overlay((t, lo, hi), rows, n)
    return t, lo, hi


@pytest.mark.parametrize("case", CLAMP_CASES, ids=lambda c: f"n{c[0]}-{offs_id(c[1])}")
def test_tensor_clamp_pinned(pkg, gpu, case):
    (n, o), lib = case, pkg._lib.load()
    rep = Report("clamp", f"n{n}-{offs_id(o)}")
    t, lo, hi = clamp_inputs(n)
    bt, bl, bh = rep.buf(gpu, 4 * n, o[0], t), rep.buf(gpu, 4 * n, o[1], lo), rep.buf(gpu, 4 * n, o[2], hi)
    rc = lib.afan_tensor_clamp(P(bt), P(bl), P(bh), n, _st())
    rep.expect(rc == 0, f"afan_tensor_clamp returned {rc}")
    rep.f32("t", bt.get(F), R.clamp(t, lo, hi))
    rep.expect(R.same_f32(bl.get(F), lo) is None and R.same_f32(bh.get(F), hi) is None, "a bound was written")
    rep.done()


# ==================================================================================================================== afan_cast_bf16
# fp32 bit patterns -> the bf16 pattern: ties to even in both directions, their neighbours, the carry into the exponent, the largest
# finite fp32 (rounds to infinity), the smallest normal, +-0, +-inf, NaN (0x7fc0 stands for "a NaN")
CAST_TABLE = [(0x3f808000, 0x3f80), (0x3f818000, 0x3f82), (0x3f808001, 0x3f81), (0x3f807fff, 0x3f80), (0x3f817fff, 0x3f81),
              (0xbf808000, 0xbf80), (0xbf818000, 0xbf82), (0xbf808001, 0xbf81), (0x3fff8000, 0x4000), (0x3ffe8000, 0x3ffe),
              (0x7f7fffff, 0x7f80), (0xff7fffff, 0xff80), (0x7f7f7fff, 0x7f7f), (0x7f7f8000, 0x7f80), (0x00800000, 0x0080), (0x80800000, 0x8080),
              (0x00000000, 0x0000), (0x80000000, 0x8000), (0x7f800000, 0x7f80), (0xff800000, 0xff80), (0x7fc00000, 0x7fc0), (0x7f800001, 0x7fc0),
              (0xffc12345, 0x7fc0)]
CAST_CASES = [(_n, (0, 0)) for _n in R.SMALL_N + (N_RAGGED,)] + [(N_RAGGED, (0, 2)), (N_RAGGED, (4, 0)), (N_RAGGED, (0, 8)),
                                                                   (R.T8, (0, 0)), (R.T1, (0, 2))]


@functools.lru_cache(maxsize=None)
def cast_inputs(n):
    rng = np.random.default_rng(n + 41)
    x = rng.standard_normal(n).astype(F)
    x[::3] = (x[::3].view(np.uint32) & 0xffff0000 | 0x8000).view(F)          # a third of the operands are ties
    overlay((x.view(np.uint32),), [(np.uint32(a),) for a, _ in CAST_TABLE], n)
    return x


@pytest.mark.parametrize("case", CAST_CASES, ids=lambda c: f"n{c[0]}-{offs_id(c[1])}")
def test_cast_bf16_pinned(pkg, gpu, case):
    (n, o), lib = case, pkg._lib.load()
    rep = Report(sorted(t for t in R.cast_tags(n, o) if t.startswith("cast<"))[0], f"n{n}-{offs_id(o)}")
    x = cast_inputs(n)
    bs, bd = rep.buf(gpu, 4 * n, o[0], x), rep.buf(gpu, 2 * n, o[1])
    rc = lib.afan_cast_bf16(P(bs), P(bd), n, _st())
    rep.expect(rc == 0, f"afan_cast_bf16 returned {rc}")
    got = bd.get(U16)
    rep.bf16("dst", got, R.bf16_bits(x))
    if n >= 2 * len(CAST_TABLE):
        for where in (slice(0, len(CAST_TABLE)), slice(n - len(CAST_TABLE), n)):
            rep.bf16(f"the table at {where.start}", got[where], np.array([b for _, b in CAST_TABLE], U16))
    rep.expect(np.array_equal(bs.get(np.uint32), x.view(np.uint32)), "src was written")
    rep.done()


# ===================================================================================================================== afan_pgd_init
IC = collections.namedtuple("IC", "src x32 shadow n offs")       # offs: x, x32, x_adv, shadow
INIT_CASES = []
for _s in (F32, BF16):
    for _sh in (1, 0):
        INIT_CASES += [IC(_s, 1, _sh, N_RAGGED, Z4), IC(_s, 1, _sh, N_RAGGED, (0, 0, 4, 0))]
    INIT_CASES += [IC(_s, 1, 1, _n, Z4) for _n in R.SMALL_N]
INIT_CASES += [IC(F32, 0, 1, N_RAGGED, Z4), IC(F32, 0, 0, N_RAGGED, (4, 0, 0, 0)), IC(F32, 0, 1, N_RAGGED, (0, 4, 0, 0)),
               IC(F32, 1, 1, N_RAGGED, (0, 0, 0, 8)), IC(BF16, 1, 1, N_RAGGED, (0, 0, 0, 8)), IC(BF16, 1, 1, N_RAGGED, (8, 0, 0, 0)),
               IC(F32, 1, 1, N_RAGGED, (0, 4, 0, 0)),
               IC(F32, 1, 1, R.T8, Z4), IC(BF16, 1, 1, R.T8, Z4), IC(F32, 0, 1, R.T1, (0, 0, 4, 0)), IC(BF16, 1, 1, R.T1, (2, 0, 0, 0))]


def init_id(c):
    return f"{GN[c.src]}-x32{c.x32}-shadow{c.shadow}-n{c.n}-{offs_id(c.offs)}"


@pytest.mark.parametrize("case", INIT_CASES, ids=init_id)
def test_pgd_init_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    rep = Report(sorted(t for t in R.init_tags(GN[c.src], c.x32, c.shadow, c.n, c.offs) if t.startswith("init<"))[0], init_id(c))
    x = cast_inputs(c.n)
    xs = R.bf16_bits(x) if c.src == BF16 else x
    want = R.bf16_widen(xs) if c.src == BF16 else x
    bx = rep.buf(gpu, GB[c.src] * c.n, c.offs[0], xs)
    b32 = rep.buf(gpu, 4 * c.n, c.offs[1]) if c.x32 else None
    bxa = rep.buf(gpu, 4 * c.n, c.offs[2])
    bsh = rep.buf(gpu, 2 * c.n, c.offs[3]) if c.shadow else None
    rc = lib.afan_pgd_init(P(bx), c.src, P(b32), P(bxa), P(bsh), c.n, _st())
    rep.expect(rc == 0, f"afan_pgd_init returned {rc}")
    rep.f32("x_adv", bxa.get(F), want)
    if c.x32:
        rep.f32("x32", b32.get(F), want)
    if c.shadow:
        rep.bf16("shadow", bsh.get(U16), R.bf16_bits(want))
    rep.expect(np.array_equal(bx.get(U16), np.asarray(xs).view(U16)), "x was written")
    rep.done()


def test_pgd_init_needs_x32_for_a_bf16_source(pkg, gpu):
    lib = pkg._lib.load()
    rep = Report("init|x32_null|bf16_refused", "n64")
    bx, bxa, bsh = rep.buf(gpu, 2 * 64, 0, np.zeros(64, U16)), rep.buf(gpu, 4 * 64), rep.buf(gpu, 2 * 64)
    rc = lib.afan_pgd_init(P(bx), BF16, None, P(bxa), P(bsh), 64, _st())
    rep.expect(rc == R.AFAN_ENULL, f"returned {rc}, expected AFAN_ENULL")
    rep.expect(bxa.untouched() and bsh.untouched(), "a refused call wrote")
    rep.done()


# ============================================================================================================================= SGD
GC = collections.namedtuple("GC", "first shadow n offs kind mom wd gscale")
MOM, WD = 0.9, 5e-4
SGD_CASES = ([GC(_f, _s, N_RAGGED, _o, "", MOM, WD, 1.0) for _f in (0, 1) for _s in (1, 0) for _o in (Z4, (0, 4, 0, 0))] +
             [GC(_n % 2, 1, _n, Z4, "", MOM, WD, 1.0) for _n in R.SMALL_N] +
             [GC(0, 1, R.T4, Z4, "", MOM, WD, 1.0), GC(1, 1, R.T4, Z4, "", MOM, WD, 1.0),
              GC(0, 1, R.T1, (4, 0, 0, 0), "", MOM, WD, 1.0), GC(1, 1, R.T1, (0, 0, 4, 0), "", MOM, WD, 1.0),
              GC(0, 1, N_RAGGED, (0, 0, 0, 2), "", MOM, WD, 1.0), GC(0, 0, N_RAGGED, (0, 0, 0, 2), "", MOM, WD, 1.0),
              GC(1, 1, N_RAGGED, Z4, "first_nan_momentum", MOM, WD, 1.0), GC(1, 0, N_RAGGED, (4, 0, 0, 0), "first_nan_momentum", MOM, WD, 1.0),
              GC(0, 1, N_RAGGED, Z4, "gscale_1/256", MOM, WD, 1.0 / 256), GC(0, 1, N_RAGGED, (4, 0, 0, 0), "gscale_1/256", MOM, WD, 1.0 / 256),
              GC(0, 1, N_RAGGED, Z4, "gscale_0", MOM, WD, 0.0), GC(1, 1, N_RAGGED, Z4, "gscale_0", MOM, WD, 0.0),
              GC(0, 1, N_RAGGED, Z4, "wd0", MOM, 0.0, 1.0), GC(0, 1, N_RAGGED, Z4, "mom0", 0.0, WD, 1.0),
              GC(0, 1, N_RAGGED, Z4, "guard_clear", MOM, WD, 1.0), GC(1, 0, N_RAGGED, (4, 0, 0, 0), "guard_clear", MOM, WD, 1.0),
              GC(0, 1, N_RAGGED, Z4, "guard_set", MOM, WD, 1.0), GC(1, 1, N_RAGGED, (4, 0, 0, 0), "guard_set", MOM, WD, 1.0),
              GC(0, 1, R.T4, Z4, "guard_set", MOM, WD, 1.0)])
LRS = (0.1, 0.0, 0.025)


def lr_seq(n):
    """The learning rates of a case's launches, written to device memory between them; one launch at the large sizes."""
    return LRS[:1] if n > 4096 else LRS


def sgd_id(c):
    return f"first{c.first}-shadow{c.shadow}-n{c.n}-{offs_id(c.offs)}" + (f"-{c.kind}" if c.kind else "")


@functools.lru_cache(maxsize=None)
def sgd_inputs(n):
    rng = np.random.default_rng(n + 53)
    return tuple(rng.standard_normal(n).astype(F) for _ in range(3))     # p, g, m


def call_sgd(lib, c, bp, bg, bm, bsh, lr, first, guard):
    a = (P(bp), P(bg), P(bm), P(bsh), c.n, ctypes.c_void_p(lr.data_ptr()), float(c.mom), float(c.wd), float(c.gscale), first)
    if guard is None:
        return lib.afan_sgd_step(*a, _st())
    return lib.afan_sgd_step_guarded(*a, guard, _st())


@pytest.mark.parametrize("case", SGD_CASES, ids=sgd_id)
def test_sgd_step_pinned(pkg, gpu, case):
    """Three launches that carry their state, the learning rate (0.1, 0, 0.025) changed in device memory in between (with first_step = 0
    no host argument changes); the first launch takes the case's first_step, the later ones 0."""
    c, lib = case, pkg._lib.load()
    rep = Report(sorted(t for t in R.sgd_tags(c.first, c.shadow, c.n, c.offs) if t.startswith("sgd<"))[0], sgd_id(c))
    p, g, m = sgd_inputs(c.n)
    if c.kind == "first_nan_momentum":
        m = np.full(c.n, np.nan, F)
    bp, bg, bm = rep.buf(gpu, 4 * c.n, c.offs[0], p), rep.buf(gpu, 4 * c.n, c.offs[1], g), rep.buf(gpu, 4 * c.n, c.offs[2], m)
    bsh = rep.buf(gpu, 2 * c.n, c.offs[3]) if c.shadow else None
    lr = torch.zeros(1, device=gpu)
    word = torch.zeros(1, dtype=torch.int32, device=gpu)                    # the test's own guard word, not the library's barrier
    guard = ctypes.c_void_p(word.data_ptr()) if c.kind.startswith("guard") else None
    if c.kind == "guard_set":
        word.fill_(3)
        for it, lr_v in enumerate(lr_seq(c.n)):
            lr.fill_(lr_v)
            rc = call_sgd(lib, c, bp, bg, bm, bsh, lr, c.first if it == 0 else 0, guard)
            rep.expect(rc == 0, f"launch {it} returned {rc}")
        rep.f32("param (must keep its contents)", bp.get(F), p)
        rep.f32("momentum (must keep its contents)", bm.get(F), m)
        rep.expect(bsh is None or bsh.untouched(), "the shadow was written")
        rep.expect(int(word.item()) == 3, "the guard word was written")
        rep.done()
        return
    wp, wm = p, m
    for it, lr_v in enumerate(lr_seq(c.n)):
        first = c.first if it == 0 else 0
        lr.fill_(lr_v)
        rc = call_sgd(lib, c, bp, bg, bm, bsh, lr, first, guard)
        rep.expect(rc == 0, f"launch {it} returned {rc}")
        wp, wm = R.sgd_step(wp, g, wm, lr_v, c.mom, c.wd, c.gscale, first)
        rep.f32(f"param after launch {it} (lr {lr_v})", bp.get(F), wp)
        rep.f32(f"momentum after launch {it}", bm.get(F), wm)
        if c.shadow:
            rep.bf16(f"shadow after launch {it}", bsh.get(U16), R.bf16_bits(wp))
        if c.kind == "first_nan_momentum":
            rep.expect(bool(np.isfinite(wp).all() and np.isfinite(wm).all()), "the reference: first_step = 1 never reads the momentum")
    rep.expect(R.same_f32(bg.get(F), g) is None, "the gradient was written")
    if guard is not None:
        # the same bits as the plain entry
        qp, qg, qm = rep.buf(gpu, 4 * c.n, c.offs[0], p), rep.buf(gpu, 4 * c.n, c.offs[1], g), rep.buf(gpu, 4 * c.n, c.offs[2], m)
        qsh = rep.buf(gpu, 2 * c.n, c.offs[3]) if c.shadow else None
        for it, lr_v in enumerate(lr_seq(c.n)):
            lr.fill_(lr_v)
            rc = call_sgd(lib, c, qp, qg, qm, qsh, lr, c.first if it == 0 else 0, None)
            rep.expect(rc == 0, f"plain launch {it} returned {rc}")
        rep.f32("param: guarded against plain", bp.get(F), qp.get(F))
        rep.f32("momentum: guarded against plain", bm.get(F), qm.get(F))
        if c.shadow:
            rep.bf16("shadow: guarded against plain", bsh.get(U16), qsh.get(U16))
        rep.expect(int(word.item()) == 0, "the guard word was written")
    rep.done()


def test_sgd_guard_pointer_is_checked_before_any_launch(pkg, gpu):
    lib = pkg._lib.load()
    rep = Report("sgd|guard_refused", "n64")
    c = GC(0, 1, 64, Z4, "", MOM, WD, 1.0)
    bufs = [rep.buf(gpu, 4 * 64) for _ in range(3)] + [rep.buf(gpu, 2 * 64)]
    lr = torch.full((1,), 0.1, device=gpu)
    word = torch.zeros(2, dtype=torch.int32, device=gpu)
    rc = lib.afan_sgd_step_guarded(*[P(b) for b in bufs], 64, ctypes.c_void_p(lr.data_ptr()), MOM, WD, 1.0, 0, None, _st())
    rep.expect(rc == R.AFAN_ENULL, f"guard NULL returned {rc}, expected AFAN_ENULL")
    for plus in (1, 2, 3):
        rc = call_sgd(lib, c, *bufs, lr, 0, ctypes.c_void_p(word.data_ptr() + plus))
        rep.expect(rc == R.AFAN_EALIGN, f"guard at +{plus} bytes returned {rc}, expected AFAN_EALIGN")
    rep.expect(all(b.untouched() for b in bufs), "a refused call wrote")
    rep.done()


# =============================================================================================================== afan_guarded_copy
COPY_BYTES = (16, 16 * R.T1)


@pytest.mark.parametrize("nbytes", COPY_BYTES)
def test_guarded_copy_pinned(pkg, gpu, nbytes):
    lib = pkg._lib.load()
    rep = Report("copy", f"{nbytes}B")
    src = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    bs = rep.buf(gpu, nbytes, 0, src)
    word, count = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    pw, pc = ctypes.c_void_p(word.data_ptr()), ctypes.c_void_p(count.data_ptr())
    for k in (1, 2):
        bd = rep.buf(gpu, nbytes)
        rc = lib.afan_guarded_copy(P(bd), P(bs), nbytes, pw, pc, _st())
        rep.expect(rc == 0, f"copy {k} returned {rc}")
        rep.expect(np.array_equal(bd.get(np.uint8), src), f"copy {k}: dst differs from src")
        rep.expect(int(count.item()) == k, f"after copy {k} the counter is {int(count.item())}")
    bd = rep.buf(gpu, nbytes)
    rc = lib.afan_guarded_copy(P(bd), P(bs), nbytes, pw, None, _st())         # counter = NULL: the copy alone
    rep.expect(rc == 0 and np.array_equal(bd.get(np.uint8), src) and int(count.item()) == 2, "counter = NULL: the copy alone")
    word.fill_(1)
    bd = rep.buf(gpu, nbytes)
    rc = lib.afan_guarded_copy(P(bd), P(bs), nbytes, pw, pc, _st())
    rep.expect(rc == 0, f"the guarded-off copy returned {rc}")
    rep.expect(bd.untouched(), "dst was written although the guard word is set")
    rep.expect(int(count.item()) == 2, f"the counter moved to {int(count.item())} although the guard word is set")
    rep.expect(np.array_equal(bs.get(np.uint8), src), "src was written")
    rep.done()


def test_guarded_copy_refuses_a_ragged_size(pkg, gpu):
    lib = pkg._lib.load()
    rep = Report("copy|refused", "24B")
    bs, bd = rep.buf(gpu, 32), rep.buf(gpu, 32)
    word, count = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    for nbytes in (24, 8, 17):
        rc = lib.afan_guarded_copy(P(bd), P(bs), nbytes, ctypes.c_void_p(word.data_ptr()), ctypes.c_void_p(count.data_ptr()), _st())
        rep.expect(rc == R.AFAN_ESHAPE, f"{nbytes} bytes returned {rc}, expected AFAN_ESHAPE")
    rep.expect(bd.untouched() and int(count.item()) == 0, "a refused call wrote")
    rep.done()


# ========================================================================================================== afan_transpose_weights
def _plain(k, rs, c):
    return [(0, 0, k, rs, c, rs, 0)]


def _six():
    """Six descriptors in one launch: two plain tensors, a 3x3 / projection pair sharing a [C][10][K] operand at (128, ., 64) as the
    arena builds it and the same pair at the ragged (80, ., 48); sources and destinations out of order with gaps between them."""
    shapes = dict(A=(16, 9, 16), B=(72, 1, 40), P3=(128, 9, 64), P1=(128, 1, 64), Q3=(80, 9, 48), Q1=(80, 1, 48))
    so, off = {}, 8
    for name, gap in (("B", 24), ("Q1", 8), ("A", 0), ("P3", 40), ("P1", 16), ("Q3", 8)):
        k, rs, c = shapes[name]
        so[name], off = off, off + k * rs * c + gap
    do, off = {}, 16
    for name, size, gap in (("Q", 48 * 10 * 80, 8), ("A", 16 * 9 * 16, 32), ("P", 64 * 10 * 128, 0), ("B", 40 * 72, 8)):
        do[name], off = off, off + size + gap
    rows = [(so["A"], do["A"]) + shapes["A"] + (9, 0), (so["B"], do["B"]) + shapes["B"] + (1, 0),
            (so["P3"], do["P"]) + shapes["P3"] + (10, 0), (so["P1"], do["P"]) + shapes["P1"] + (10, 9),
            (so["Q3"], do["Q"]) + shapes["Q3"] + (10, 0), (so["Q1"], do["Q"]) + shapes["Q1"] + (10, 9)]
    return rows


TRANSPOSE_CASES = [_plain(*s) for s in ((8, 1, 8), (16, 9, 16), (32, 9, 16), (72, 1, 40), (64, 1, 48), (80, 9, 48), (256, 9, 304),
                                         (64, 49, 8), (2048, 1, 512))]
TRANSPOSE_CASES += [[(0, 0, 80, 9, 48, 10, 0)],                       # only the 3x3 of a pair: slot 9 keeps the fill
                    [(8, 24, 128, 1, 64, 10, 9)],                     # only the projection: slots 0 .. 8 keep the fill
                    _six()]


def transpose_id(rows):
    return "+".join(f"{k}x{rs}x{c}" + (f"@{drs}.{rs0}" if drs != rs else "") for _, _, k, rs, c, drs, rs0 in rows)


def transpose_extent(rows):
    return (max(so + k * rs * c for so, _, k, rs, c, _, _ in rows) + 8, max(do + c * drs * k for _, do, k, _, c, drs, _ in rows) + 8)


@pytest.mark.parametrize("rows", TRANSPOSE_CASES, ids=transpose_id)
def test_transpose_weights_pinned(pkg, gpu, rows):
    lib = pkg._lib.load()
    rep = Report("transpose", transpose_id(rows))
    descs, tiles = R.make_descs(rows)
    n_src, n_dst = transpose_extent(rows)
    src = (np.arange(n_src) & 0xffff).astype(U16)
    bs, bd = rep.buf(gpu, 2 * n_src, 0, src), rep.buf(gpu, 2 * n_dst)
    dd = torch.from_numpy(descs).to(gpu)
    for nd, nt in ((0, tiles), (len(rows), 0)):
        rc = lib.afan_transpose_weights(P(bs), P(bd), ctypes.c_void_p(dd.data_ptr()), nd, nt, _st())
        rep.expect(rc == 0 and bd.untouched(), f"n_desc = {nd}, total_tiles = {nt}: returned {rc} or wrote")
    rc = lib.afan_transpose_weights(P(bs), P(bd), ctypes.c_void_p(dd.data_ptr()), len(rows), tiles, _st())
    rep.expect(rc == 0, f"afan_transpose_weights returned {rc}")
    want = R.transpose_weights(src, np.full(n_dst, SENT * 0x101, U16), descs)
    got = bd.get(U16)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        rep.expect(False, f"{bad.size} of {n_dst} destination elements differ; first at {i}: got {int(got[i]):#06x}, expected {int(want[i]):#06x}")
    rep.expect(np.array_equal(bs.get(U16), src), "the source was written")
    rep.done()


# ====================================================================================================== one case above the ABI
def test_arena_sgd_keeps_param_shadow_and_transposed_weights_in_step(pkg, gpu):
    """Three convolutions 3 -> 16 -> 32 -> 48 (3x3, 3x3, 1x1; channels-last, bf16) under ParamArena + ArenaSGD.  The first has 3 input
    channels, which the arena leaves without a CRSK operand; the other two are the 16 / 32 / 48-channel partial tiles of the transpose.
    After two step()s on fixed gradients: the parameters are the reference applied to the flat arena (padding included: it stays zero),
    the shadow is their RNE bf16, every CRSK operand is its shadow permuted."""
    nn = torch.nn
    C = pkg.resnet_s.Conv2d

    class Net(nn.Module):
        compute_dtype = torch.bfloat16
        channels_last = True

        def __init__(self):
            super().__init__()
            self.c0, self.c1, self.c2 = C(3, 16, 3, padding=1, bias=False), C(16, 32, 3, padding=1, bias=True), C(32, 48, 1, bias=False)

    rep = Report("arena", "3-16-32-48")
    torch.manual_seed(11)
    net = Net()
    for m in net.modules():
        if isinstance(m, C):
            m.compute_dtype = torch.bfloat16
    net.to(gpu)
    arena = pkg.arena.ParamArena(net, skip=(), bf16_shadow=True, channels_last=True)
    opt = pkg.arena.ArenaSGD(arena, lr=0.1, momentum=0.9, weight_decay=5e-4)
    used = np.zeros(arena.numel, bool)
    for o, p in zip(arena.offsets, arena.params):
        used[o:o + p.numel()] = True
    assert not used.all(), "the case is meant to hold padding"
    wp, wm = arena.param.cpu().numpy().copy(), np.zeros(arena.numel, F)
    rep.expect(not wp[~used].any(), "the padding does not start at zero")
    gen = torch.Generator().manual_seed(12)
    for it in range(2):
        for p in arena.params:
            p.grad.copy_(torch.randn(p.shape, generator=gen).to(gpu))
        g = arena.grad.cpu().numpy().copy()
        rep.expect(not g[~used].any(), "a gradient reached the padding")
        opt.step()
        wp, wm = R.sgd_step(wp, g, wm, 0.1, 0.9, 5e-4, 1.0, False)
        rep.f32(f"arena.param after step {it}", arena.param.cpu().numpy(), wp)
        rep.f32(f"arena.momentum_buf after step {it}", arena.momentum_buf.cpu().numpy(), wm)
    rep.expect(not arena.param.cpu().numpy()[~used].any(), "the padding did not stay zero")
    rep.bf16("arena.shadow", arena.shadow.view(torch.int16).cpu().numpy().view(U16), R.bf16_bits(wp))
    rep.expect(not hasattr(net.c0, "_arena_wt"), "a 3-channel convolution got a CRSK operand")
    covered = 0
    for m in (net.c1, net.c2):
        wt, sh = m._arena_wt, m._arena_shadow
        rep.expect(tuple(wt.shape) == (m.in_channels, m.out_channels) + tuple(m.kernel_size), f"_arena_wt has shape {tuple(wt.shape)}")
        same = torch.equal(wt.contiguous().view(torch.int16), sh.permute(1, 0, 2, 3).contiguous().view(torch.int16))
        rep.expect(same, f"the CRSK operand of the {m.in_channels} -> {m.out_channels} convolution is not its shadow permuted")
        rep.expect(bool((sh.float() != 0).any()), "the shadow is all zero")
        covered += wt.numel()
    rep.expect(covered == arena.shadow_t.numel(), "shadow_t holds elements no convolution owns")
    rep.done()


# ==================================================================================================================== coverage
_G = ("f32", "bf16")
_V = ("vec", "scalar")
EXPECTED_VARIANTS = sorted(
    [f"pgd_step<{g},{c},{s},{v}>" for g in _G for c in ("clip", "noclip") for s in ("shadow", "noshadow") for v in _V] +
    ["pgd_step|trip2|vec", "pgd_step|trip2|scalar", "pgd_step|ragged_tail", "pgd_step|x_clean_null", "pgd_step|eps0"] +
    [f"pgd_step|scalar_by|{t}" for t in ("x_adv", "grad", "x_clean", "shadow")] +
    [f"step_norms<{g},{c},{s},{v}>" for g in _G for c in ("clip", "noclip") for s in ("shadow", "noshadow") for v in _V] +
    [f"step_norms|{t}|{v}" for t in ("multi_slice", "ragged_slice", "finalize_trip2", "idle_threads", "batch_limit", "nan_sample") for v in _V] +
    ["step_norms|scalar_by|per%4", "step_norms|scalar_by|x_adv", "step_norms|batch_refused"] +
    [f"noise<{v}>|{s}" for v in _V for s in ("shadow", "noshadow")] + ["noise|trip2|vec", "noise|trip2|scalar", "noise|ragged_tail"] +
    ["clamp", "clamp|trip2|scalar"] +
    ["cast<vec>", "cast<scalar>", "cast|trip2|vec", "cast|trip2|scalar", "cast|ragged_tail"] +
    [f"init<{g},{v}>|{s}" for g in _G for v in _V for s in ("shadow", "noshadow")] +
    ["init|trip2|vec", "init|trip2|scalar", "init|ragged_tail", "init|x32_null|vec", "init|x32_null|scalar", "init|x32_null|bf16_refused",
     "init|scalar_by|shadow"] +
    [f"sgd<{f},{s}>|{v}" for f in ("first", "later") for s in ("shadow", "noshadow") for v in _V] +
    ["sgd|trip2|vec", "sgd|trip2|scalar", "sgd|ragged_tail", "sgd|first_nan_momentum", "sgd|gscale_1/256", "sgd|gscale_0", "sgd|wd0", "sgd|mom0",
     "sgd|guard_clear", "sgd|guard_set", "sgd|guard_set|trip2"] +
    ["copy", "copy|trip2|scalar"] +
    [f"transpose|{t}" for t in ("partial_k_tile", "partial_c_tile", "multi_k_tile", "multi_c_tile", "full_tiles", "rs>1", "multi_desc",
                                "shared_operand|rs0=0", "shared_operand|rs0=9", "slot_left_alone", "offsets_out_of_order")])


def table_variants():
    got = set()
    for c in STEP_CASES:
        got |= step_labels(c)
    for c in NORM_CASES:
        got |= norm_labels(c)
    got |= R.step_norms_tags("f32", 4, 1, 1, R.MAX_BATCH + 1, 1, Z4)          # test_pgd_step_norms_refuses_batch_65536
    for c in NOISE_CASES:
        got |= R.noise_tags(c.shadow, c.n, c.offs)
    for n, _ in CLAMP_CASES:
        got |= R.clamp_tags(n)
    for n, o in CAST_CASES:
        got |= R.cast_tags(n, o)
    for c in INIT_CASES:
        got |= R.init_tags(GN[c.src], c.x32, c.shadow, c.n, c.offs)
    got |= R.init_tags("bf16", 0, 1, 64, Z4)                                  # test_pgd_init_needs_x32_for_a_bf16_source
    for c in SGD_CASES:
        got |= R.sgd_tags(c.first, c.shadow, c.n, c.offs, c.kind)
    for nbytes in COPY_BYTES:
        got |= R.copy_tags(nbytes)
    for rows in TRANSPOSE_CASES:
        got |= R.transpose_tags(rows)
    return got
