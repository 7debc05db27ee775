"""Every kernel variant of csrc/afan_conv_f32.hip (the general fp32-arithmetic convolutions: forward, input gradient, weight gradient
and its slab reduction) pinned ELEMENTWISE to float64.  afan_conv_fwd / afan_conv_dgrad / afan_conv_wgrad are called through the C ABI
with ctypes, so that the activation layout, the weight layout, the pointer offsets and the workspace are the test's choice; every
operand and output lives inside a larger sentinel-filled buffer.  The references, the case table and the restated dispatch are
tests/conv_f32_pinned_refs.py (tests/test_conv_f32_pinned_ref.py checks them against torch on the CPU and shows that the table reaches
exactly EXPECTED_VARIANTS).

Each row runs in the four activation / weight layout pairs, both storages, aligned and with either or both operands one element late:
  * exact: sparse integers in {-2..2}, integer bias in [-4, 4].  fp32 results equal float64 bit for bit, bf16 results are the RNE
    bf16 of float64, weight gradients (fp32 for both storages) are bit-exact, also when added into an integer-valued gradient; a
    gradient pre-filled with NaN is overwritten without accumulate; the slab workspace is pre-filled with NaN.
  * rounding-aware (Gaussian operands, fp32 storage): |got - float64| <= C * 2^-24 * S elementwise, S the same operation on absolute
    values (plus |bias|), C the number of fp32 roundings on the longest path - the kernel's header: one fmaf per product:
    forward / dgrad: in-image products + 1 (bias); wgrad: in-image pixel products + slices + 1 (accumulate).
    Printed as "F32PIN <op> <worst ratio of the error to that bound> <case>" (run with -s) before the assertion.
  * same bits across variants (Gaussian operands, no tolerance): the LDS image and the MFMA sequence depend neither on the staging
    mode nor on the strides, so all layout pairs and offsets give torch.equal results; bf16 storage gives f32_result.to(bfloat16) on
    the same bf16-representable values and the same fp32 weight gradient; KCRS and KRSC gradient orders agree.
  * writes: the sentinel around every operand, output and the workspace (exactly workspace_floats long) is intact.

Worst ratios measured on an MI355X over this table (error / (C * 2^-24 * S); the limit is 1: the header's "one fmaf per product"
holds, C is not raised anywhere):
  fwd        0.349   1x300x1x5-co21-k1s1p0d1   (5 products + bias)
  dgrad      0.232   1x3x2x68-co8-k1s1p0d1     (8 products)
  wgrad      0.541   2x1x1x36-co20-k1s2p0d1    (2 pixel products + 1 slice)
  wgrad_acc  0.376   2x1x1x36-co20-k1s2p0d1    (added into a Gaussian gradient: + 1)
The short sums come closest: a long sum's error is a random walk far below C * S (weight gradient of 2x33x35x4, 2310 pixels: 0.0002;
of 2x128x128x3, 32768 pixels: below 0.0001), so on the long rows the exact and the same-bits checks are the ones that bind.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_f32_pinned_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = {R.F32: F32, R.BF16: BF16}
NCHW, NHWC = R.NCHW, R.NHWC
LAY = {NCHW: "nchw", NHWC: "nhwc"}
WLAY = {NCHW: "kcrs", NHWC: "krsc"}
U = R.U
SENTINEL = -777.0
GUARD = 64                          # elements of sentinel before and after every tensor: 256 / 128 bytes, the content stays aligned
OK, EDTYPE, EALIGN, ESHAPE, ENULL, ELAYOUT = 0, -1, -2, -3, -4, -5


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Report:
    def __init__(self, what):
        self.what, self.fails = what, []

    def expect(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def figure(self, key, value, note=""):
        print(f"F32PIN {key} {value:.4f} {self.what} {note}")

    def done(self):
        assert not self.fails, f"{self.what}: {len(self.fails)} failures:\n  " + "\n  ".join(self.fails[:12])


class Buf:
    """A logical [N, C, H, W] tensor (weights: [Co, Ci, k, k]) in NCHW / NHWC memory order, placed GUARD (+ late) elements into a
    larger sentinel-filled device buffer.  vals = None leaves the content at the sentinel as well."""

    def __init__(self, shape, dt, layout, dev, late=0, vals=None):
        self.shape, self.layout, self.off = tuple(shape), layout, GUARD + late
        self.numel = int(np.prod(shape))
        self.raw = torch.full((self.off + self.numel + GUARD,), SENTINEL, dtype=dt, device=dev)
        self.flat = self.raw[self.off:self.off + self.numel]
        if vals is not None:
            v = torch.as_tensor(vals).reshape(self.shape)
            v = v.permute(0, 2, 3, 1) if layout == NHWC else v
            self.flat.copy_(v.reshape(-1).to(dt))

    def nchw(self):
        n, c, h, w = self.shape
        t = self.flat.cpu()
        return t.view(n, h, w, c).permute(0, 3, 1, 2).contiguous() if self.layout == NHWC else t.view(n, c, h, w)

    def guard_ok(self):
        s = torch.full((1,), SENTINEL, dtype=self.raw.dtype, device=self.raw.device)
        return bool((self.raw[:self.off] == s).all()) and bool((self.raw[self.off + self.numel:] == s).all())


def check_exact(rep, name, got, ref):
    """ref (float64) is an fp32 value: fp32 got equals it bit for bit, bf16 got is its RNE rounding."""
    ref = torch.from_numpy(ref)
    assert bool((ref.float().double() == ref).all()), f"{name}: the float64 result is not an fp32 value"
    want = ref.float().to(got.dtype)
    bad = ~(got == want)
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements differ from float64; first at {i}: got {float(got[i])!r}, expected {float(want[i])!r}")


def check_same(rep, name, got, base):
    if not torch.equal(got, base):
        bad = ~(got == base)
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the aligned nhwc / krsc fp32 call; first at {i}: "
                          f"{float(got[i])!r} vs {float(base[i])!r}")


def check_bound(rep, op, name, got, ref, scale, roundings):
    """|got - float64| <= roundings * 2^-24 * S elementwise; returns and prints the worst ratio of the error to the bound."""
    err = np.abs(got.double().numpy() - ref)
    lim = roundings * U * scale
    if not np.isfinite(err).all():
        rep.expect(False, f"{name}: non-finite values")
        return float("inf")
    pos = lim > 0
    ratio = float((err[pos] / lim[pos]).max()) if pos.any() else 0.0
    if (err[~pos] > 0).any():
        ratio = float("inf")
    rep.figure(op, ratio, name)
    bad = err > lim
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        rep.expect(False, f"{name}: {int(bad.sum())} of {err.size} elements past C * 2^-24 * S (worst ratio {ratio:.3f}); first at {i}: got "
                          f"{float(got[i])!r}, float64 {ref[i]!r}, C {np.broadcast_to(roundings, err.shape)[i]}, S {scale[i]!r}")
    return ratio


def call_id(dt, lay, wl, mis):
    return f"{R.TN[dt]} {LAY[lay]} {WLAY[wl]} late {mis}"


def geo(c):
    return (c.n, c.hi, c.wi, c.ci, c.co, c.k, c.stride, c.pad, c.dil)


# ------------------------------------------------------------------------------------------------------------------ the three entries
def run_fwd(lib, dev, pr, dt, lay, wl, mis):
    c, t = pr.case, DT[dt]
    x = Buf(pr.x.shape, t, lay, dev, mis & 1, pr.x)
    w = Buf(pr.w.shape, t, wl, dev, (mis >> 1) & 1, pr.w)
    y = Buf(pr.y.shape, t, lay, dev, int(mis != 0))
    b = None if pr.b is None else torch.from_numpy(pr.b).float().to(dev)
    rc = lib.afan_conv_fwd(P(x.flat), P(w.flat), P(b), P(y.flat), dt, lay, wl, *geo(c), _st())
    return rc, y.nchw(), x.guard_ok() and w.guard_ok() and y.guard_ok()


def run_dgrad(lib, dev, pr, dt, lay, wl, mis):
    c, t = pr.case, DT[dt]
    dy = Buf(pr.dy.shape, t, lay, dev, mis & 1, pr.dy)
    w = Buf(pr.w.shape, t, wl, dev, (mis >> 1) & 1, pr.w)
    dx = Buf(pr.x.shape, t, lay, dev, int(mis != 0))
    rc = lib.afan_conv_dgrad(P(dy.flat), P(w.flat), P(dx.flat), dt, lay, wl, *geo(c), _st())
    return rc, dx.nchw(), dy.guard_ok() and w.guard_ok() and dx.guard_ok()


def run_wgrad(lib, dev, pr, dt, lay, wl, mis, acc, g0):
    """g0: the gradient tensor's previous content (float64 [Co, Ci, k, k]).  The workspace is exactly workspace_floats long, NaN
    inside, sentinel around."""
    c, t = pr.case, DT[dt]
    x = Buf(pr.x.shape, t, lay, dev, mis & 1, pr.x)
    dy = Buf(pr.dy.shape, t, lay, dev, (mis >> 1) & 1, pr.dy)
    g = Buf(pr.w.shape, F32, wl, dev, int(mis != 0), g0)
    nws = int(lib.afan_conv_wgrad_f32_workspace_floats(*geo(c)))
    ws = Buf((1, 1, 1, nws), F32, NCHW, dev, 0, torch.full((nws,), float("nan")))
    rc = lib.afan_conv_wgrad(P(x.flat), P(dy.flat), P(g.flat), dt, lay, wl, *geo(c), P(ws.flat), acc, _st())
    return rc, g.nchw(), x.guard_ok() and dy.guard_ok() and g.guard_ok() and ws.guard_ok(), nws


def wgrad_roundings(pr, acc):
    c = pr.case
    return pr.dw_cnt[None, None] + R.workspace_floats(c) // (c.co * c.k * c.k * c.ci) + acc


ROWS = [(i, op) for i in range(len(R.CASES)) for op in R.OPS]


@pytest.mark.parametrize("idx,op", ROWS, ids=lambda v: v if isinstance(v, str) else R.case_id(R.CASES[v]))
def test_conv_f32_pinned(pkg, gpu, idx, op):
    lib, c = pkg._lib.load(), R.CASES[idx]
    rep = Report(f"afan_conv_{op} {R.case_id(c)}")
    nan_g = np.full((c.co, c.ci, c.k, c.k), np.nan)
    for kind in R.KINDS:
        pr = R.problem(idx, kind)
        if op == "wgrad":
            rep.expect(int(lib.afan_conv_wgrad_f32_workspace_floats(*geo(c))) == R.workspace_floats(c),
                       f"workspace_floats {int(lib.afan_conv_wgrad_f32_workspace_floats(*geo(c)))}, the restated plan gives {R.workspace_floats(c)}")
        got = {}
        for dt, lay, wl, mis in R.calls(kind):
            nm = f"{kind} {call_id(dt, lay, wl, mis)}"
            if op == "fwd":
                rc, res, ok = run_fwd(lib, gpu, pr, dt, lay, wl, mis)
            elif op == "dgrad":
                rc, res, ok = run_dgrad(lib, gpu, pr, dt, lay, wl, mis)
            else:
                rc, res, ok, _ = run_wgrad(lib, gpu, pr, dt, lay, wl, mis, 0, nan_g)      # accumulate = 0: the NaNs are overwritten
            rep.expect(rc == OK, f"{nm}: returned {rc}")
            rep.expect(ok, f"{nm}: wrote outside the output / the workspace, or into an operand's surroundings")
            if rc == OK:
                got[(dt, lay, wl, mis)] = res
            if op == "wgrad" and kind == "exact":
                rc, res, ok, _ = run_wgrad(lib, gpu, pr, dt, lay, wl, mis, 1, pr.g0)
                rep.expect(rc == OK and ok, f"{nm} accumulate: returned {rc}, guards intact {ok}")
                if rc == OK:
                    check_exact(rep, f"{nm} accumulate", res, pr.dw + pr.g0)
        key0 = (R.F32, NHWC, NHWC, 0)
        if key0 not in got:
            continue
        base = got[key0]
        ref, scale, cnt = {"fwd": (pr.y, pr.y_s, pr.y_cnt[None, None] + (pr.b is not None)),
                           "dgrad": (pr.dx, pr.dx_s, pr.dx_cnt[None, None]),
                           "wgrad": (pr.dw, pr.dw_s, wgrad_roundings(pr, 0))}[op]
        if kind == "exact":
            check_exact(rep, f"exact {call_id(*key0)}", base, ref)
        else:
            check_bound(rep, op, f"{kind} {call_id(*key0)}", base, ref, scale, cnt)
        for key, res in got.items():
            want = base if (key[0] == R.F32 or op == "wgrad") else base.to(BF16)
            check_same(rep, f"{kind} {call_id(*key)}", res, want)
        if op == "wgrad" and kind == "gauss32":          # added into a Gaussian gradient: one more rounding, of the sum
            rc, res, ok, _ = run_wgrad(lib, gpu, pr, R.F32, NHWC, NHWC, 0, 1, pr.g0)
            rep.expect(rc == OK and ok, f"gauss32 accumulate: returned {rc}, guards intact {ok}")
            if rc == OK:
                check_bound(rep, "wgrad_acc", "gauss32 accumulate", res, pr.dw + pr.g0, pr.dw_s + np.abs(pr.g0), wgrad_roundings(pr, 1))
    rep.done()


# ------------------------------------------------------------------------------------------------- return codes, degenerate sizes
def test_return_codes_and_degenerate_sizes(pkg, gpu):
    lib = pkg._lib.load()
    rep = Report("afan_conv_f32 return codes")
    mk = lambda dt=F32, n=4096: torch.full((n,), SENTINEL, dtype=dt, device=gpu)
    x, w, y, ws = mk(), mk(), mk(), mk()
    untouched = lambda *ts: all(bool((t == SENTINEL).all()) for t in ts)

    def all_three(g, dt=R.F32, lay=NHWC, wl=NHWC, px=None, pw=None, py=None, pws=None, wgrad_only=False):
        px, pw, py, pws = (P(x) if px is None else px), (P(w) if pw is None else pw), (P(y) if py is None else py), (P(ws) if pws is None else pws)
        if wgrad_only:
            return lib.afan_conv_wgrad(px, pw, py, dt, lay, wl, *g, pws, 0, _st())
        return (lib.afan_conv_fwd(px, pw, None, py, dt, lay, wl, *g, _st()), lib.afan_conv_dgrad(px, pw, py, dt, lay, wl, *g, _st()),
                lib.afan_conv_wgrad(px, pw, py, dt, lay, wl, *g, pws, 0, _st()))

    good = (1, 8, 8, 4, 4, 3, 1, 1, 1)
    bad_shapes = {"k = 8": (1, 8, 8, 4, 4, 8, 1, 4, 1), "k = 0": (1, 8, 8, 4, 4, 0, 1, 0, 1), "stride 3": (1, 8, 8, 4, 4, 3, 3, 1, 1),
                  "pad 128": (1, 8, 8, 4, 4, 3, 1, 128, 1), "dilation 65": (1, 8, 8, 4, 4, 3, 1, 65, 65), "dilation 0": (1, 8, 8, 4, 4, 3, 1, 1, 0),
                  "window larger than the padded input": (1, 4, 4, 4, 4, 3, 1, 1, 3), "window wider than the padded input": (1, 8, 2, 4, 4, 5, 1, 1, 1),
                  "negative n": (-1, 8, 8, 4, 4, 3, 1, 1, 1), "ci = 0": (1, 8, 8, 0, 4, 3, 1, 1, 1)}
    for name, g in bad_shapes.items():
        rep.expect(all_three(g) == (ESHAPE,) * 3, f"{name}: returned {all_three(g)}, expected AFAN_ESHAPE")
        rep.expect(int(lib.afan_conv_wgrad_f32_workspace_floats(*g)) == 0, f"{name}: workspace_floats is not 0")
    rep.expect(all_three(good, dt=2) == (EDTYPE,) * 3, f"dtype 2: returned {all_three(good, dt=2)}")
    rep.expect(all_three(good, lay=2) == (ELAYOUT,) * 3 and all_three(good, wl=2) == (ELAYOUT,) * 3, "layout 2 was not declined with AFAN_ELAYOUT")
    null = ctypes.c_void_p(None)
    for name, kw in (("x", dict(px=null)), ("w / dy", dict(pw=null)), ("y / dx / grad", dict(py=null))):
        rep.expect(all_three(good, **kw) == (ENULL,) * 3, f"NULL {name}: returned {all_three(good, **kw)}")
    rep.expect(all_three(good, pws=null, wgrad_only=True) == ENULL, "NULL workspace was not declined")
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)
    for dt, by in ((R.F32, 1), (R.F32, 2), (R.BF16, 1)):
        for name, kw in (("x", dict(px=odd(x, by))), ("w / dy", dict(pw=odd(w, by)))):
            rep.expect(all_three(good, dt=dt, **kw) == (EALIGN,) * 3, f"{name} {by} bytes past an element of dtype {dt}: returned {all_three(good, dt=dt, **kw)}")
        r = all_three(good, dt=dt, py=odd(y, by))
        rep.expect(r == (EALIGN,) * 3, f"output {by} bytes past an element of dtype {dt}: returned {r}")
    rep.expect(all_three(good, pws=odd(ws, 4), wgrad_only=True) == EALIGN, "a workspace that is not 16-byte aligned was not declined")
    rep.expect(untouched(x, w, y, ws), "a declined call wrote to its tensors")
    rep.expect(all_three(good) == (OK,) * 3, f"the plain call of this test returned {all_three(good)}")
    # n = 0: OK, y untouched, pointers not looked at; the weight gradient is zeroed, or left as it is under accumulate
    empty = (0,) + good[1:]
    y2 = mk()
    r = (lib.afan_conv_fwd(null, null, None, P(y2), R.F32, NHWC, NHWC, *empty, _st()), lib.afan_conv_dgrad(null, null, P(y2), R.F32, NHWC, NHWC, *empty, _st()))
    rep.expect(r == (OK, OK) and untouched(y2), f"n = 0: returned {r} or wrote y")
    rep.expect(int(lib.afan_conv_wgrad_f32_workspace_floats(*empty)) == 0, "n = 0: workspace_floats is not 0")
    numel = 4 * 4 * 9
    for wl in (NHWC, NCHW):
        g = Buf((4, 4, 3, 3), F32, wl, gpu, 0, np.full((4, 4, 3, 3), 5.0))
        rc = lib.afan_conv_wgrad(null, null, P(g.flat), R.F32, NHWC, wl, *empty, null, 1, _st())
        rep.expect(rc == OK and bool((g.flat == 5.0).all()) and g.guard_ok(), f"n = 0 accumulate ({WLAY[wl]}): returned {rc} or changed grad")
        rc = lib.afan_conv_wgrad(null, null, P(g.flat), R.BF16, NCHW, wl, *empty, null, 0, _st())
        rep.expect(rc == OK and bool((g.flat == 0.0).all()) and g.flat.numel() == numel and g.guard_ok(), f"n = 0 ({WLAY[wl]}): returned {rc}, grad not zeroed or written past")
    rep.done()


# ------------------------------------------------------------------------------------------------------------------ through ops
@pytest.mark.parametrize("shape", [(3, 1, 6, 5, 4, 3, 1, 1, 1), (3, 8, 1, 1, 4, 1, 1, 0, 1), (2, 1, 1, 1, 1, 3, 1, 1, 1)],
                         ids=["c1", "hw1", "c1-hw1"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_ambiguous_layouts_through_ops(pkg, gpu, shape, dt):
    """C = 1 or H * W = 1: the tensor is dense in both memory orders and torch reports both; either stride flavour, on either side, must
    give the same results through ops, and they must match float64 (exact operands: bit for bit)."""
    n, ci, hi, wi, co, k, stride, pad, dil = shape
    rep = Report(f"ops.conv_general_* {shape}")
    rng = np.random.RandomState(7)
    draw = lambda s: (rng.randint(-2, 3, size=s) * (rng.random_sample(s) < 0.7)).astype(np.float64)
    ho, wo = R.out_dim(hi, k, stride, pad, dil), R.out_dim(wi, k, stride, pad, dil)
    x64, w64, dy64, b64 = draw((n, ci, hi, wi)), draw((co, ci, k, k)), draw((n, co, ho, wo)), rng.randint(-4, 5, size=co).astype(np.float64)
    y_ref = R.fwd(x64, w64, b64, stride, pad, dil)[0]
    dx_ref = R.dgrad(dy64, w64, (hi, wi), stride, pad, dil)[0]
    dw_ref = R.wgrad(x64, dy64, k, stride, pad, dil)[0]

    def flavours(a, t):
        """The tensor with NCHW strides and with channels-last strides (size-1 dimensions carry the strides a permute would give)."""
        v = torch.from_numpy(a).to(t).to(gpu)
        s0, s1, s2, s3 = v.shape
        cl = torch.empty_strided(v.shape, (s1 * s2 * s3, 1, s3 * s1, s1), dtype=t, device=gpu)
        cl.copy_(v)
        return [("nchw-strides", v.contiguous()), ("nhwc-strides", cl)]

    b = torch.from_numpy(b64).float().to(gpu)
    for (nx, x), (nw, w), (nd, dy) in [(a, b_, c_) for a in flavours(x64, dt) for b_ in flavours(w64, dt) for c_ in flavours(dy64, dt)]:
        nm = f"x {nx}, w {nw}, dy {nd}"
        check_exact(rep, f"fwd {nm}", pkg.ops.conv_general_fwd(x, w, b, stride, pad, dil).cpu(), y_ref)
        check_exact(rep, f"dgrad {nm}", pkg.ops.conv_general_dgrad(dy, w, (hi, wi), stride, pad, dil).cpu(), dx_ref)
        check_exact(rep, f"wgrad {nm}", pkg.ops.conv_general_wgrad(x, dy, k, stride, pad, dil).cpu(), dw_ref)
        for (ng, g) in flavours(np.ones_like(w64), F32):
            pkg.ops.conv_general_wgrad(x, dy, k, stride, pad, dil, grad=g, accumulate=True)
            check_exact(rep, f"wgrad into a {ng} gradient, {nm}", g.cpu(), dw_ref + 1.0)
    rep.done()
