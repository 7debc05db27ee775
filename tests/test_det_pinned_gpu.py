"""Every ROIAlign kernel form of csrc/afan_det.hip and the linear-pair kernels of csrc/afan_linear.hip pinned ELEMENTWISE to float64.
Every kernel is called through the C ABI with ctypes, so that workspace = NULL and the buffers are the test's choice.  The references
are tests/det_pinned_refs.py (float64 after an fp32 geometry, written from the definition; tests/test_det_pinned_ref.py checks them
against the C oracle and the torch restatement on the CPU).

Two checks per case:
  * exact: operands for which every fp32 operation of every form is exact (ROIAlign: scale 1/16, starts on eighths of a cell,
    extents bin * P with dyadic bins, integer values in [-8, 8]; linear pair: ternary operands, integer biases).  fp32 results must
    equal float64 bit for bit IN ANY summation order (the scatter's atomics included); bf16 results must be the RNE bf16 of float64.
  * rounding-aware: Gaussian operands, random ROIs (malformed, outside the map, r / P an integer, bins below one cell);
    |got - float64| <= C * 2^-24 * S elementwise, S the same operation on absolute values, C the number of fp32 roundings on the
    longest path of the kernel's expression (stated at each c_* below).  A bf16 result must be the RNE bf16 of float64; the other
    neighbour only where float64 lies within that noise of the rounding midpoint, for at most 1 % of a case's elements.
Every case prints "DETPIN <form> <worst ratio> <case>" (run with -s) before it asserts: the worst |got - float64| / (C * 2^-24 * S).

Worst ratios on an MI355X (this table; every exact check bit for bit; the share of bf16 outputs that are not the RNE bf16 of float64
below 1e-4 in every case):
    fwd_elt f32    nchw 0.354   nhwc 0.464   nhwc unaligned 0.419        fwd_elt bf16   nchw 0.000   nhwc 0.000   nhwc unaligned 0.075
    fwd_bins       f32 0.474    f32 stride loop 0.475    bf16 0.050
    bwd_scatter f32   nchw 0.263   nhwc cvec 0.314   nhwc maxp 0.294   nhwc unaligned 0.284
    bwd_scatter bf16  nchw 0.336   nhwc cvec 0.339   nhwc maxp 0.343   nhwc unaligned 0.338
    bwd_gather     f32 0.252 (tables and NULL: the same bits)    bf16 0.262    (R = 1300: 0.030 / 0.018, R = 2100: 0.009 / 0.016)
    linear pair    forward 0.147   input gradient 0.135   weight gradient 0.906 (M = 1: one product, C = 1)   bias gradient 0.309

Coverage: EXPECTED_VARIANTS lists every instantiation and inner path the tables must reach; the host-side dispatch conditions of
afan_roi_align_fwd / afan_roi_align_bwd_ws and of the linear pair are restated here with the source's constants named.
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import det_pinned_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF16: "bf16"}
DTC = {F32: 0, BF16: 1}
VEC = {F32: 4, BF16: 8}                      # `vec`: elements per 16-byte access
NCHW, NHWC = 0, 1
LAY = {NCHW: "nchw", NHWC: "nhwc"}
U = R.U
N, H, W = 2, 13, 18                          # not a multiple of the 4 x 4 tile
SCALE = 1 / 16
# constants of csrc/afan_det.hip
BINS_MIN_VECS = 16                           # the `c / vec >= 16` rule of the geometry-once-per-bin forward
BINS_THREADS = 256                           # its workgroup: more channel vectors take the `cv += blockDim.x` loop
RG_TH, RG_TW, RG_NV, RG_MAXP, RG_THREADS, RG_LIST = 4, 4, 16, 16, 256, 1024
# constants of csrc/afan_linear.hip
RT, KT, NMAX = 32, 64, 128
BF16_SHARE_CAP = 0.01


# ---- roundings counted from the kernels' expressions (-ffp-contract=off: every operation rounds once) -------------------------------
def c_fwd(k):
    """roi_align_fwd_kernel / roi_align_fwd_bins_kernel: out += w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4 with w1 = hy * hx per sample,
    out / count at the end.  The longest path of one tap: the weight product (1), the tap product (1), the three inner adds (3), one
    add into `out` per sample of the bin (k), the division (1).  l and h = 1 - l are fp32 values in the reference too."""
    return 6 + k


def c_scatter(k):
    """roi_align_bwd_kernel: g1 = gtop * w1 / count, unsafeAtomicAdd: the weight product (1), the product (1), the division (1) and
    one add per non-zero term arriving at the cell (k), in any order."""
    return 3 + k


def c_gather(ty, tx, k):
    """roi_align_bwd_gather_kernel / roi_bwd_tables_kernel: Wy = (sum of up to ty sample weights) / count (ty + 1), Wx = sum of up to
    tx sample weights (tx), w = wy * wx (1), acc = fmaf(w, d, acc) once per non-zero (ROI, ph, pw) term of the cell (k)."""
    return ty + tx + 2 + k


# ------------------------------------------------------------------------------------------------------------------------ helpers
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

    def figure(self, key, value):
        print(f"DETPIN {key} {value:.4f} {self.what}")

    def done(self):
        assert not self.fails, f"{self.what}:\n  " + "\n  ".join(self.fails[:12])


def check_exact(rep, name, got, ref):
    """ref (float64) is an fp32 value: fp32 got equals it bit for bit, bf16 got is its RNE rounding."""
    assert bool((ref.float().double() == ref).all()), f"{name}: the float64 result is not an fp32 value"
    want = R.rne_bf16(ref) if got.dtype == BF16 else ref.float()
    bad = ~(got == want)
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements differ from float64; first at {i}: got {float(got[i])!r}, "
                          f"expected {float(want[i])!r}")


def check_window(rep, key, name, got, ref, noise):
    """got must round from a real value within `noise` of ref (float64); prints the worst ratio.  bf16: at most BF16_SHARE_CAP of
    the elements may be anything but the RNE bf16 of ref."""
    rep.expect(bool(torch.isfinite(got.float()).all()), f"{name}: non-finite values")
    if got.dtype == BF16:
        glo, ghi = R.bf16_edges(got)
        need = torch.maximum(glo - ref, ref - ghi).clamp_min(0.0)
        share = float((got != R.rne_bf16(ref)).double().mean())
        rep.figure(key + "|share", share)
        rep.expect(share <= BF16_SHARE_CAP, f"{name}: {share:.4f} of the elements are not the RNE bf16 of float64")
    else:
        need = (got.double() - ref).abs()
    need = torch.nan_to_num(need, nan=float("inf"))
    pos = noise > 0
    ratio = float((need[pos] / noise[pos]).max()) if bool(pos.any()) else 0.0
    if bool((need[~pos] > 0).any()):
        ratio = float("inf")
    rep.figure(key, ratio)
    bad = need > noise
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements outside the window (worst ratio {ratio:.3f}); first at {i}: got "
                          f"{float(got[i])!r}, float64 {float(ref[i])!r} +- {float(noise[i])!r}")


# ==================================================================================================================== ROIAlign
RC = collections.namedtuple("RC", "op dt layout c ph pw r sr corner off")


def _rc(op, dt, layout, c, p, r, sr, corner=False, off=0):
    """off: the input tensor (x of the forward, dy of the backward) starts `off` elements past a 16-byte boundary."""
    ph, pw = p if isinstance(p, tuple) else (p, p)
    return RC(op, dt, layout, c, ph, pw, r, sr, corner, off)


ROI_CASES = []
for _dt in (F32, BF16):
    _v = VEC[_dt]
    ROI_CASES += [
        # element-per-thread forward <T, NHWC>: C = 3, or C = 6 channels-last (C % vec != 0)
        _rc("fwd", _dt, NCHW, 3, (7, 5), 24, 0), _rc("fwd", _dt, NHWC, 6, (7, 5), 24, 2),
        # geometry once per bin: 16 channel vectors
        _rc("fwd", _dt, NHWC, BINS_MIN_VECS * _v, 7, 24, 0),
        # scatter: NCHW; channels-last with C % vec != 0; channels-last with a pooled size above RG_MAXP
        _rc("bwd", _dt, NCHW, 3, (7, 5), 24, 0), _rc("bwd", _dt, NHWC, 6, (7, 5), 24, 2), _rc("bwd", _dt, NHWC, _v, RG_MAXP + 1, 12, 0),
        # gather: a partial last slab; R = 1300: two list chunks, the second of two passes of 256 threads (the last partly filled);
        # R = 2100: three chunks, the third one partly filled pass; pooled 14 and 16; a corner of image 0 only (other tiles are
        # reached by no ROI)
        _rc("bwd", _dt, NHWC, RG_NV * _v + 2 * _v, 7, 24, 0), _rc("bwd", _dt, NHWC, _v, 7, 1300, 0), _rc("bwd", _dt, NHWC, _v, 7, 2100, 0),
        _rc("bwd", _dt, NHWC, _v, 14, 24, 2), _rc("bwd", _dt, NHWC, _v, RG_MAXP, 24, 4), _rc("bwd", _dt, NHWC, _v, 7, 6, 0, corner=True),
        # shapes of the vector forms on an input that is not 16-byte aligned: the element forward, the scatter
        _rc("fwd", _dt, NHWC, BINS_MIN_VECS * _v, 7, 8, 0, off=1), _rc("bwd", _dt, NHWC, _v, 7, 8, 0, off=1),
    ]
# one below the `c / vec >= 16` rule (element forward), and the stride loop of the bins forward: 257 channel vectors
ROI_CASES += [_rc("fwd", F32, NHWC, (BINS_MIN_VECS - 1) * 4, 7, 8, 0), _rc("fwd", F32, NHWC, (BINS_THREADS + 1) * 4, 7, 4, 0)]


def roi_id(c):
    return f"{c.op}-{DTN[c.dt]}-{LAY[c.layout]}-c{c.c}-p{c.ph}x{c.pw}-r{c.r}-sr{c.sr}" + ("-corner" if c.corner else "") + (f"-off{c.off}" if c.off else "")


@functools.lru_cache(maxsize=None)
def roi_tables(c):
    """{table: (rois, geometry)} of a case; the seed depends on the shape only, so that fp32 and bf16 see the same ROIs."""
    seed = c.ph * 1000 + c.pw * 100 + c.sr * 10 + c.r + c.c
    ex = R.exact_rois(c.r, N, H, W, c.ph, c.pw, seed, sampling_ratio=c.sr, corner=c.corner)
    ga = R.gauss_rois(c.r, N, H, W, c.ph, c.pw, seed + 1, corner=c.corner)
    return {"exact": (ex, R.roi_geom(ex, SCALE, c.ph, c.pw, H, W, c.sr)), "gauss": (ga, R.roi_geom(ga, SCALE, c.ph, c.pw, H, W, c.sr))}


def fwd_is_bins(c):
    """afan_roi_align_fwd: channels-last, whole 16-byte channel vectors, at least 16 of them, x and y 16-byte aligned."""
    vec = VEC[c.dt]
    return c.layout == NHWC and c.c % vec == 0 and c.c // vec >= BINS_MIN_VECS and c.off == 0


def bwd_is_gather(c):
    """afan_roi_align_bwd_ws: channels-last, whole channel vectors, pooled sizes up to RG_MAXP, dy and dx 16-byte aligned (R < 2^24)."""
    return c.layout == NHWC and c.r > 0 and c.c % VEC[c.dt] == 0 and c.ph <= RG_MAXP and c.pw <= RG_MAXP and c.off == 0


def untouched_tiles(kg):
    """Map tiles (n, ty, tx) of RG_TH x RG_TW cells no ROI leaves a term on, from the reference's term count [N, H, W]."""
    k = np.pad(kg.numpy(), ((0, 0), (0, (-H) % RG_TH), (0, (-W) % RG_TW)))
    return int((k.reshape(N, -1, RG_TH, k.shape[2] // RG_TW, RG_TW).sum((2, 4)) == 0).sum())


def roi_form(c):
    """The kernel form the host-side dispatch picks for the case."""
    d = DTN[c.dt]
    if c.op == "fwd":
        if not fwd_is_bins(c):
            return f"fwd_elt|{d}|{LAY[c.layout]}" + ("|unaligned" if c.off else "")
        return f"fwd_bins|{d}" + ("|stride" if c.c // VEC[c.dt] > BINS_THREADS else "")
    if not bwd_is_gather(c):
        why = "" if c.layout == NCHW else ("|cvec" if c.c % VEC[c.dt] else "|unaligned" if c.off else "|maxp")
        return f"bwd_scatter|{d}|{LAY[c.layout]}{why}"
    return f"bwd_gather|{d}"


def roi_labels(c):
    d = DTN[c.dt]
    if not (c.op == "bwd" and bwd_is_gather(c)):
        return {roi_form(c)}
    out = {f"bwd_gather|{d}|tab", f"bwd_gather|{d}|notab", f"bwd_gather|{d}|P{c.ph}"}
    cs = RG_NV * VEC[c.dt]
    if c.c > cs and c.c % cs:
        out.add(f"bwd_gather|{d}|partial_slab")
    chunks = -(-c.r // RG_LIST)
    if chunks > 1:
        last = c.r - (chunks - 1) * RG_LIST
        out.add(f"bwd_gather|{d}|chunks{chunks}" + ("|partial" if last % RG_THREADS else ""))
    tabs = roi_tables(c)
    paths = [R.gather_paths(g, RG_TW) for _, g in tabs.values()]
    if all(p[0] > 0 for p in paths) and not c.corner:
        out.add(f"bwd_gather|{d}|small")
    if all(p[1] > 0 for p in paths) and not c.corner:
        out.add(f"bwd_gather|{d}|loop")
    if all(untouched_tiles(R.roi_align_bwd(torch.zeros((c.r, 1, c.ph, c.pw), dtype=torch.float64), g, N)[3]) > 0 for _, g in tabs.values()):
        out.add(f"bwd_gather|{d}|empty_tile")
    return out


def _operands(c, table, shape, gen):
    if table == "exact":
        return R.ints(shape, 8, gen)
    return torch.randn(shape, generator=gen).to(c.dt).double()


def _to_dev(t64, c, dev):
    t = t64.permute(0, 2, 3, 1) if c.layout == NHWC else t64
    buf = torch.zeros((t.numel() + 16,), dtype=c.dt, device=dev)
    view = buf[c.off:c.off + t.numel()]
    view.copy_(t.reshape(-1).to(c.dt))
    assert (view.data_ptr() % 16 == 0) == (c.off == 0)
    return view


def _from_dev(t, c, shape):
    n, ch, a, b = shape
    t = t.cpu()
    return t.view(n, a, b, ch).permute(0, 3, 1, 2) if c.layout == NHWC else t.view(n, ch, a, b)


def run_fwd(lib, dev, c, x64, rois):
    x = _to_dev(x64, c, dev)
    y = torch.full((c.r * c.c * c.ph * c.pw,), float("nan"), dtype=c.dt, device=dev)
    rd = torch.from_numpy(rois).to(dev)
    rc = lib.afan_roi_align_fwd(P(x), P(rd), P(y), DTC[c.dt], c.layout, c.r, c.c, H, W, c.ph, c.pw, SCALE, c.sr, _st())
    return rc, _from_dev(y, c, (c.r, c.c, c.ph, c.pw))


def run_bwd(lib, dev, c, dy64, rois, ws):
    dy = _to_dev(dy64, c, dev)
    dx = torch.full((N * c.c * H * W,), float("nan"), dtype=F32, device=dev)       # (the gather writes every cell itself)
    rd = torch.from_numpy(rois).to(dev)
    wsb = None
    if ws:
        wsb = torch.empty(int(lib.afan_roi_align_bwd_workspace_bytes(c.r, H, W)), dtype=torch.uint8, device=dev)
    rc = lib.afan_roi_align_bwd_ws(P(dy), P(rd), P(dx), DTC[c.dt], c.layout, c.r, N, c.c, H, W, c.ph, c.pw, SCALE, c.sr, P(wsb), _st())
    return rc, _from_dev(dx, c, (N, c.c, H, W))


@pytest.mark.parametrize("case", ROI_CASES, ids=roi_id)
def test_roi_align_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    form = roi_form(c)
    rep = Report(f"{roi_id(c)} expected {form}")
    gen = torch.Generator().manual_seed(c.c * 7 + c.r)
    assert int(lib.afan_roi_align_bwd_workspace_bytes(c.r, H, W)) == c.r * (H + W) * (RG_MAXP * 4 + 4)
    for table, (rois, g) in roi_tables(c).items():
        if c.op == "fwd":
            x64 = _operands(c, table, (N, c.c, H, W), gen)
            ref, s, k = R.roi_align_fwd(x64, g)
            rc, y = run_fwd(lib, gpu, c, x64, rois)
            rep.expect(rc == 0, f"forward {table} returned {rc}")
            if rc:
                continue
            if table == "exact":
                ok, bits = R.exact_range_ok(g, float(s.max()))
                assert ok, (bits, float(s.max()))
                check_exact(rep, "forward exact", y, ref)
            else:
                check_window(rep, form, "forward", y, ref, c_fwd(k[:, None].double()) * U * s)
            continue
        dy64 = _operands(c, table, (c.r, c.c, c.ph, c.pw), gen)
        ref, s, ks, kg = R.roi_align_bwd(dy64, g, N)
        if table == "exact":
            ok, bits = R.exact_range_ok(g, float(s.max()))
            assert ok, (bits, float(s.max()))
        gather = bwd_is_gather(c)
        noise = (c_gather(R.axis_terms(g.y), R.axis_terms(g.x), kg) if gather else c_scatter(ks))[:, None].double() * U * s
        outs = []
        for ws in ((False, True) if gather else (False,)):
            rc, dx = run_bwd(lib, gpu, c, dy64, rois, ws)
            nm = f"backward {table}" + (" tables" if ws else "")
            rep.expect(rc == 0, f"{nm} returned {rc}")
            if rc:
                continue
            outs.append(dx)
            if table == "exact":
                check_exact(rep, nm, dx, ref)
            else:
                key = (form + ("|tab" if ws else "|notab")) if gather else form
                check_window(rep, key, nm, dx, ref, noise)
        if len(outs) == 2:
            rep.expect(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"backward {table}: tables given and NULL differ in bits")
    rep.done()


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_roi_align_and_pooler_through_det_ops_exact(pkg, gpu, nhwc):
    """det_ops.roi_align and det_ops.Pooler.apply on the exact table: forward and x.grad bit for bit, and the 2 x 2 max pool's routing
    (ties included: first maximum in scan order) that of float64."""
    c, r = 8, 16
    gen = torch.Generator().manual_seed(31 + nhwc)
    for (ph, pw, sr, pooler) in ((7, 7, 2, False), (14, 14, 0, True)):
        rois = R.exact_rois(r, N, H, W, ph, pw, seed=77 + ph, sampling_ratio=sr)
        g = R.roi_geom(rois, SCALE, ph, pw, H, W, sr)
        x64 = R.ints((N, c, H, W), 8, gen)
        ref, s, _ = R.roi_align_fwd(x64, g)
        xt = x64.float().to(gpu)
        xt = (xt.contiguous(memory_format=torch.channels_last) if nhwc else xt).requires_grad_(True)
        rd = torch.from_numpy(rois).to(gpu)
        if pooler:
            y = pkg.det_ops.Pooler.apply(xt, rd[:, 1:], rd[:, 0].long(), "align")
            r14 = ref.clone().requires_grad_(True)
            want = torch.nn.functional.max_pool2d(r14, kernel_size=2, stride=2)
            dyp = R.ints(want.shape, 8, gen)
            want.backward(dyp)
            dy64 = r14.grad
        else:
            y = pkg.det_ops.roi_align(xt, rd, (ph, pw), SCALE, sr)
            want, dyp = ref, R.ints(ref.shape, 8, gen)
            dy64 = dyp
        dref, sb, _, _ = R.roi_align_bwd(dy64, g, N)
        assert R.exact_range_ok(g, max(float(s.max()), float(sb.max())))[0]
        assert torch.equal(y.detach().cpu().double(), want.detach()), f"forward, pooler={pooler}"
        y.backward(dyp.float().to(gpu))
        assert torch.equal(xt.grad.cpu().double(), dref), f"x.grad, pooler={pooler}"


# ============================================================================================================== the linear pair
LC = collections.namedtuple("LC", "m k n1 n2")
LIN_CASES = [LC(1, 4, 8, 0), LC(5, 68, 32, 1), LC(32, 132, 31, 33), LC(33, 2048, 33, 32), LC(300, 68, 32, 64), LC(5, 2048, 33, 64),
             LC(33, 132, 64, 64), LC(5, 4160, 32, 33)]


def fwd_chunk(nt):
    return 128 if nt <= 64 else 64                     # KCH: reduction steps per LDS stage


def fwd_slices(k, nt):
    return max(1, min(64, -(-k // fwd_chunk(nt))))     # one slice per staging chunk, 64 at the most


def fwd_kslice(k, nt):
    kc = fwd_chunk(nt)
    return -(-(-(-k // kc)) // fwd_slices(k, nt)) * kc


def wgrad_slices(m, k):
    ktiles, rows = -(-k // KT), -(-m // RT)
    s = 1 if ktiles >= 256 else -(-256 // ktiles)
    return max(1, min(s, rows))


def wgrad_rslice(m, k):
    return -(-(-(-m // RT)) // wgrad_slices(m, k)) * RT


def lin_id(c):
    return f"m{c.m}-k{c.k}-n{c.n1}+{c.n2}"


def lin_labels(c):
    nt = c.n1 + c.n2
    s, ks = fwd_slices(c.k, nt), fwd_kslice(c.k, nt)
    out = {f"linear_fwd<{-(-nt // 32)},{fwd_chunk(nt)}>", "linear_fwd|" + ("split" if s > 1 else "direct"), f"linear_fwd|nt{nt}",
           "linear_dgrad", "linear_wgrad|" + ("slices1" if wgrad_slices(c.m, c.k) == 1 else "slicesN")}
    if ks > fwd_chunk(nt):
        out.add("linear_fwd|chunks_per_slice>1")
    if (s - 1) * ks >= c.k:
        out.add("linear_fwd|empty_slices")
    if c.m < RT and s > 1:
        out.add("linear_fwd|rows<32|split")
    if c.n2 == 0:
        out.add("linear_fwd|n2=0")
    elif c.n1 in (31, 32, 33):
        out.add(f"linear_fwd|n1={c.n1}")
    return out


def _lin_call(lib, dev, c, x, w1, b1, w2, b2):
    nt = c.n1 + c.n2
    dv = lambda t: None if t is None else t.float().contiguous().to(dev)
    xd, w1d, w2d, b1d, b2d = dv(x), dv(w1), dv(w2 if c.n2 else None), dv(b1), dv(b2 if c.n2 else None)
    y1 = torch.full((c.m, c.n1), float("nan"), device=dev)
    y2 = torch.full((c.m, c.n2), float("nan"), device=dev) if c.n2 else None
    nws = int(lib.afan_linear_pair_workspace_floats(0, c.m, c.n1, c.n2, c.k))
    s = fwd_slices(c.k, nt)
    assert nws == (s * c.m * nt if s > 1 else 0), f"forward workspace {nws}: expected {s} slices of {fwd_kslice(c.k, nt)}"
    ws = torch.full((max(nws, 4),), float("nan"), device=dev)
    rc = lib.afan_linear_pair_fwd_f32(P(xd), P(w1d), P(b1d), P(w2d), P(b2d), P(y1), P(y2), c.m, c.n1, c.n2, c.k, P(ws), _st())
    return rc, y1.cpu(), (y2.cpu() if c.n2 else torch.zeros((c.m, 0)))


@pytest.mark.parametrize("case", LIN_CASES, ids=lin_id)
def test_linear_pair_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    nt = c.n1 + c.n2
    rep = Report(f"linear pair {lin_id(c)}: {fwd_slices(c.k, nt)} slices of {fwd_kslice(c.k, nt)}, {wgrad_slices(c.m, c.k)} row slices")
    gen = torch.Generator().manual_seed(c.m * 13 + c.k + nt)
    dv = lambda t: t.float().contiguous().to(gpu)
    for exact in (True, False):
        tag = "exact" if exact else "gauss"
        if exact:
            x, w1, w2 = R.ternary((c.m, c.k), gen), R.ternary((c.n1, c.k), gen), R.ternary((c.n2, c.k), gen)
            b1, b2 = R.ints((c.n1,), 3, gen), R.ints((c.n2,), 3, gen)
            g1, g2 = R.ternary((c.m, c.n1), gen), R.ternary((c.m, c.n2), gen)
            start = [R.ints(s, 5, gen) for s in ((c.n1, c.k), (c.n1,), (c.n2, c.k), (c.n2,))]
        else:
            rn = lambda *s: torch.randn(s, generator=gen).double()
            x, w1, w2, b1, b2, g1, g2 = rn(c.m, c.k), rn(c.n1, c.k), rn(c.n2, c.k), rn(c.n1), rn(c.n2), rn(c.m, c.n1), rn(c.m, c.n2)
            start = [rn(c.n1, c.k), rn(c.n1), rn(c.n2, c.k), rn(c.n2)]

        def hold(key, name, got, ref, s, cc):
            if got.numel() == 0:
                return
            if exact:
                assert float(s.max()) < 2.0 ** 24, f"{name}: sum |a * b| = {float(s.max())} is not below 2^24"
                check_exact(rep, f"{name} exact", got, ref)
            else:
                check_window(rep, key, name, got, ref, cc * U * s)

        # forward: a fused multiply-add chain over the slice (the padding adds exact zeros), the slices' partials added in order, the bias
        c_f = min(fwd_kslice(c.k, nt), c.k) + (fwd_slices(c.k, nt) - 1) + 1
        for bias in (True, False):
            y1, s1, y2, s2 = R.linear_pair(x, w1, b1 if bias else None, w2, b2 if bias else None)
            rc, o1, o2 = _lin_call(lib, gpu, c, x, w1, b1 if bias else None, w2, b2 if bias else None)
            rep.expect(rc == 0, f"forward {tag} returned {rc}")
            if rc == 0:
                nm = f"forward {tag}" + ("" if bias else " without biases")
                hold("linear_fwd", nm + " y1", o1, y1, s1, c_f)
                hold("linear_fwd", nm + " y2", o2, y2, s2, c_f)
        # input gradient: one chain over the N1 + N2 columns
        gx, sx, ((gw1, sw1, gb1, sb1), (gw2, sw2, gb2, sb2)) = R.linear_pair_grads(g1, g2, x, w1, w2)
        gxd = torch.full((c.m, c.k), float("nan"), device=gpu)
        g1d, g2d, w1d, w2d, xd = dv(g1), (dv(g2) if c.n2 else None), dv(w1), (dv(w2) if c.n2 else None), dv(x)
        rc = lib.afan_linear_pair_dgrad_f32(P(g1d), P(g2d), P(w1d), P(w2d), P(gxd), c.m, c.n1, c.n2, c.k, _st())
        rep.expect(rc == 0, f"dgrad {tag} returned {rc}")
        if rc == 0:
            hold("linear_dgrad", f"dgrad {tag}", gxd.cpu(), gx, sx, nt)
        # parameter gradients: a chain over the slice's rows, the row slices' partials added in order, + the add onto the start value
        ws_n = int(lib.afan_linear_pair_workspace_floats(1, c.m, c.n1, c.n2, c.k))
        assert ws_n == wgrad_slices(c.m, c.k) * nt * (c.k + 1), f"wgrad workspace {ws_n}"
        wsd = torch.full((ws_n,), float("nan"), device=gpu)
        for acc in (0, 1):
            outs = [dv(t) for t in start]
            if not c.n2:
                outs[2] = outs[3] = None
            rc = lib.afan_linear_pair_wgrad_f32(P(g1d), P(g2d), P(xd), P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), acc, c.m, c.n1, c.n2, c.k,
                                                P(wsd), _st())
            rep.expect(rc == 0, f"wgrad {tag} accumulate={acc} returned {rc}")
            if rc:
                continue
            c_w = min(wgrad_rslice(c.m, c.k), c.m) + (wgrad_slices(c.m, c.k) - 1) + acc
            refs = [(gw1, sw1), (gb1, sb1), (gw2, sw2), (gb2, sb2)]
            for i, nm in enumerate(("gw1", "gb1", "gw2", "gb2")):
                if outs[i] is None:
                    continue
                ref, s = refs[i]
                if acc:
                    ref, s = ref + start[i].float().double(), s + start[i].float().double().abs()
                hold("linear_wgrad" if nm[1] == "w" else "linear_bgrad", f"{nm} {tag} accumulate={acc}", outs[i].cpu(), ref, s, c_w)
    rep.done()


# ======================================================================================================================= coverage
_G = [f"bwd_gather|{d}|{f}" for d in ("f32", "bf16") for f in ("tab", "notab", "P7", "P14", "P16", "partial_slab", "chunks2|partial", "chunks3|partial",
                                                                 "small",
                                                                 "loop", "empty_tile")]
EXPECTED_VARIANTS = sorted(
    [f"fwd_elt|{d}|{lay}" for d in ("f32", "bf16") for lay in ("nchw", "nhwc", "nhwc|unaligned")] + ["fwd_bins|f32", "fwd_bins|bf16", "fwd_bins|f32|stride"] +
    [f"bwd_scatter|{d}|{v}" for d in ("f32", "bf16") for v in ("nchw", "nhwc|cvec", "nhwc|maxp", "nhwc|unaligned")] + _G +
    ["linear_fwd<1,128>", "linear_fwd<2,128>", "linear_fwd<3,64>", "linear_fwd<4,64>", "linear_fwd|direct", "linear_fwd|split",
     "linear_fwd|chunks_per_slice>1", "linear_fwd|empty_slices", "linear_fwd|rows<32|split", "linear_fwd|n2=0", "linear_fwd|n1=31",
     "linear_fwd|n1=32", "linear_fwd|n1=33", "linear_dgrad", "linear_wgrad|slices1", "linear_wgrad|slicesN"] +
    [f"linear_fwd|nt{n}" for n in (8, 33, 64, 65, 96, 97, 128)])


def table_variants():
    got = set()
    for c in ROI_CASES:
        got |= roi_labels(c)
    for c in LIN_CASES:
        got |= lin_labels(c)
    return got


def test_tables_reach_every_variant():
    """The tables reach every kernel form exactly: the four element forwards, the bins forward per type and its stride loop, the
    scatter per type and reason, the gather <T, TAB> with a partial last slab, a ROI list of two and of three chunks with a
    partly filled last pass, both inner paths, the three pooled sizes and a tile no ROI reaches; the linear pair's four
    forward instantiations, the split and the direct reduction, empty trailing slices, few rows with a split reduction, n1 on and
    beside a 32-column group boundary, one and several row slices of the parameter gradient."""
    got = table_variants()
    assert sorted(got) == EXPECTED_VARIANTS, f"missing {sorted(set(EXPECTED_VARIANTS) - got)}, unexpected {sorted(got - set(EXPECTED_VARIANTS))}"
    # shapes the issue names
    assert {c.k for c in LIN_CASES} == {4, 68, 132, 2048, 4160} and {c.m for c in LIN_CASES} == {1, 5, 32, 33, 300}
    big = [c for c in LIN_CASES if c.k == 4160][0]
    assert fwd_slices(big.k, big.n1 + big.n2) == 64 and fwd_kslice(big.k, big.n1 + big.n2) == 128
