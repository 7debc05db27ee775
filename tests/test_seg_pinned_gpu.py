"""Every kernel variant of csrc/afan_seg.hip pinned ELEMENTWISE to float64: the bilinear resize (dense, channel slice, two-pass
separable backward), ce2d, the fused ce2d_upsampled, max pooling (general k / stride / pad with the position byte), global average
pooling, the pointwise classifier, linear_small and dropout.  Every kernel is called through the C ABI with ctypes, so that pixel
strides, pointer offsets, ws = NULL and idx = NULL are the test's choice.  The references are tests/seg_pinned_refs.py (float64,
written from the definitions; tests/test_seg_pinned_ref.py checks them against torch on the CPU).

Two checks per case:
  * exact: operands for which every partial sum is exact in fp32 in any order (resize: dyadic scales, integer values |x| <= 64;
    pooling: routing of integer gradients; pointwise / linear: ternary operands).  fp32 results must equal float64 bit for bit, bf16
    results must be the RNE bf16 of the float64 value.
  * rounding-aware: Gaussian operands; |got - float64| <= C * 2^-24 * S with S the same operation applied to absolute values and C
    the number of fp32 roundings counted from the kernel's expression (stated at each C_* below); a bf16 result must be the RNE
    bf16 of the float64 value, the other neighbour only where float64 lies within that noise of the rounding midpoint.
expf / logf give no exact route: ce2d is held to C_CE * 2^-24 * scale, C_CE = three times the worst ratio measured on an MI355X
over this table (*_MEASURED below, as the weight gradient of the pointwise layer).  Every test prints its figures
("SEGPIN <key> <ratio> <case>", run with -s) before it asserts.

Coverage: EXPECTED_VARIANTS lists every instantiation and capped grid the tables must reach; the host-side dispatch conditions are
restated here (vec_for, the slice entries' vector conditions, grid_for's caps: constants of the source, named below).
"""
import collections
import ctypes
import zlib

import numpy as np
import pytest
import torch

import seg_pinned_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF16: "bf16"}
DTC = {F32: 0, BF16: 1}
VEC = {F32: 4, BF16: 8}
ES = {F32: 4, BF16: 2}
NCHW, NHWC = 0, 1
LAY = {NCHW: "nchw", NHWC: "nhwc"}
U = R.U
SENTINEL = -777.0
ESHAPE = -3
# constants of csrc/afan_seg.hip: BLOCK; grid_for(total, 256, 4096) of maxpool / avgpool_bwd / ce2d_up_gather; grid_for(P, 256, 2048)
# of ce2d and dropout; pw_blocks' 1024 slices of PW_SLICE = 64 pixels; 4 * 64 channels per chunk of pointwise_dw_kernel
BLOCK = 256
CAP_4096 = 4096 * BLOCK
CAP_2048 = 2048 * BLOCK
PW_CAP_M = 1024 * 64
PW_CHUNK = 256

# ---- roundings counted from the kernels' expressions -----------------------------------------------------------------------------
# upsample_fwd_kernel: a.l0 * (b.l0 * p00 + b.l1 * p01) + a.l1 * (b.l0 * p10 + b.l1 * p11), built with -ffp-contract=off: four inner
# products, two inner sums, two outer products and the last sum round once each (9), but one tap passes through only 4 of them
# (product, row sum, row weight, last sum): 4 * 2^-24 * S to first order.  7 (the count of the contracted form plus the store, as
# the issue states it) covers that with room for the second-order terms; l0 = 1 - l1 is an fp32 value in the reference too.
C_RESIZE_FWD = 7
# backward: w = wy * wx rounds once, then one multiply-add per term: K_y * K_x terms + 2 (one-pass gather); the two-pass form takes
# K_x then K_y multiply-adds (never more).  K_* = the largest number of outputs an input feeds along an axis (R.resize_terms).
C_RESIZE_BWD_EXTRA = 2
# ce2d_up_kernel + gather: 16 + 16 multiply-adds of which at most K_y + K_x are non-zero, up to 4 tile partials: bounded by
# K_y * K_x + 2 + 4
C_FUSED_BWD_EXTRA = 6
# avgpool forward: the issue's bound, hw roundings of a sum whose S is mean |x|
# pointwise forward: a lane takes whole 16-byte pieces, VEC * ceil(ci / (4 VEC)) multiply-adds (bias = the start value), then two
# shuffle adds: pw_fwd_roundings(); dx: co multiply-adds
# linear_small forward: ceil(ci / 64) multiply-adds per lane + 6 butterfly adds; dx: ceil(co / 16) per wave + 16 adds of the fold;
# dw: n multiply-adds (+ 1 when added into dw)

# ---- measured constants: worst |kernel - float64| / (2^-24 * scale) over THIS table on an MI355X; each limit is three times it --------
# ce2d gradient: scale = grad_scale / count per element (worst: nchw-2x32x7x23-ign255-mixed); loss: scale = max(1, |loss|) (worst:
# nhwc-2x21x7x23-ign255-one_live)
CE_GRAD_MEASURED, CE_LOSS_MEASURED = 6.83, 2.34
C_CE_GRAD, C_CE_LOSS = 3.0 * CE_GRAD_MEASURED, 3.0 * CE_LOSS_MEASURED
# pointwise weight / bias gradient: scale = sum |dy x| / sum |dy| (64-pixel slices in fp32, slabs folded in two stages); worst: dw
# bf16 ci 256, db f32 ci 512
PW_DW_MEASURED, PW_DB_MEASURED = 1.98, 1.73
C_PW_DW, C_PW_DB = 3.0 * PW_DW_MEASURED, 3.0 * PW_DB_MEASURED


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _seed(case, salt):
    return (zlib.crc32(repr(case).encode()) * 31 + salt) % (1 << 31)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t, byte_off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_off)


class Report:
    def __init__(self, what):
        self.what, self.fails = what, []

    def expect(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def figure(self, key, value):
        print(f"SEGPIN {key} {value:.4f} {self.what}")

    def done(self):
        assert not self.fails, f"{self.what}:\n  " + "\n  ".join(self.fails[:12])


class Buf:
    """numel elements placed `off` elements into a larger sentinel-filled device buffer; nchw() / put() convert between the logical
    [N, C, H, W] CPU tensor and the buffer's memory order."""

    def __init__(self, shape, dt, layout, dev, off=0, vals=None, fill=SENTINEL):
        self.shape, self.layout, self.off, self.fill = tuple(shape), layout, off, fill
        self.numel = int(np.prod(shape))
        self.raw = torch.full((self.numel + 32,), fill, dtype=dt, device=dev)
        self.flat = self.raw[off:off + self.numel]
        if vals is not None:
            v = vals.permute(0, 2, 3, 1) if layout == NHWC else vals
            self.flat.copy_(v.reshape(-1).to(dt))

    def nchw(self):
        n, c, h, w = self.shape
        t = self.flat.cpu()
        return t.view(n, h, w, c).permute(0, 3, 1, 2) if self.layout == NHWC else t.view(n, c, h, w)

    def guard_ok(self):
        s = torch.full((1,), self.fill, dtype=self.raw.dtype, device=self.raw.device)
        return bool((self.raw[:self.off] == s).all()) and bool((self.raw[self.off + self.numel:] == s).all())


def _bf16_edges(got):
    """The closed real interval that rounds (to nearest, ties either way) to each bf16 element of got."""
    b = got.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag, neg = b & 0x7fff, (b >> 15) == 1
    val = lambda mm: (mm << 16).contiguous().view(torch.float32).double()
    v, up, dn = val(mag), val(mag + 1), val((mag - 1).clamp_min(0))
    hi_m = (v + up) / 2
    lo_m = torch.where(mag > 0, (v + dn) / 2, -up / 2)
    return torch.where(neg, -hi_m, lo_m), torch.where(neg, -lo_m, hi_m)


def check_window(rep, name, got, ref, noise):
    """got (bf16 / fp32 CPU tensor) must round from a real value within `noise` of ref (float64)."""
    noise = noise if torch.is_tensor(noise) else torch.full_like(ref, float(noise))
    rep.expect(bool(torch.isfinite(got.float()).all()), f"{name}: non-finite values")
    lo, hi = ref - noise, ref + noise
    if got.dtype == BF16:
        glo, ghi = _bf16_edges(got)
        bad = (glo > hi) | (ghi < lo)
    else:
        g = got.double()
        bad = (g > hi) | (g < lo)
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements outside the window; first at {i}: got {float(got[i])!r}, float64 "
                          f"{float(ref[i])!r} +- {float(noise.expand_as(ref)[i])!r}")


def check_exact(rep, name, got, ref):
    """ref (float64) is an fp32 value: fp32 got equals it bit for bit, bf16 got is its RNE rounding.  NaN matches NaN."""
    assert bool(((ref.float().double() == ref) | torch.isnan(ref)).all()), f"{name}: the float64 result is not an fp32 value"
    want = ref.float().to(got.dtype)
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    nb = int(bad.sum())
    if nb:
        i = tuple(bad.nonzero()[0].tolist())
        rep.expect(False, f"{name}: {nb} of {got.numel()} elements differ from float64; first at {i}: got {float(got[i])!r}, "
                          f"expected {float(want[i])!r}")


def ratio_of(got, ref, unit):
    """Worst distance between ref and the reals that round to got, in units of `unit`."""
    if got.dtype == BF16:
        glo, ghi = _bf16_edges(got)
        need = torch.maximum(glo - ref, ref - ghi).clamp_min(0.0)
    else:
        need = (got.double() - ref).abs()
    unit = unit.expand_as(need) if torch.is_tensor(unit) else torch.full_like(need, float(unit))
    pos = unit > 0
    if bool((need[~pos] > 0).any()):
        return float("inf")
    return float((need[pos] / unit[pos]).max()) if bool(pos.any()) else 0.0


def pw_fwd_roundings(dt, ci):
    return VEC[dt] * -(-ci // (4 * VEC[dt])) + 2


def vec_for(dt, c, byte_offsets):
    """vec_for<T> of the source: 16-byte vectors when the channel count divides and every given pointer is 16-byte aligned."""
    return VEC[dt] if c % VEC[dt] == 0 and all(o % 16 == 0 for o in byte_offsets) else 1


def q_(t, dt):
    return t.to(dt).double()


# ================================================================================================================== bilinear resize
RZ = collections.namedtuple("RZ", "kind dt layout n c hi wi ho wo off ld c0")


def _rz(kind, dt, layout, n, c, hi, wi, ho, wo, off=0, ld=0, c0=0):
    return RZ(kind, dt, layout, n, c, hi, wi, ho, wo, off, ld, c0)


# (n, hi, wi, ho, wo): non-square dyadic with n = 3 (plane = row / Ho), one source pixel, hi == ho, non-dyadic up, down-scaling
RZ_SHAPES = [(3, 5, 9, 20, 18), (1, 1, 1, 4, 2), (2, 7, 6, 7, 6), (2, 9, 9, 33, 33), (1, 17, 23, 40, 31), (1, 40, 31, 17, 23)]
RESIZE_CASES = []
for _dt in (F32, BF16):
    _cs = {F32: 6, BF16: 12}[_dt]                       # c % VEC != 0: the scalar channels-last kernels
    for _s in RZ_SHAPES:
        RESIZE_CASES += [_rz("dense", _dt, NCHW, _s[0], 2, *_s[1:]), _rz("dense", _dt, NHWC, _s[0], 8, *_s[1:]),
                         _rz("dense", _dt, NHWC, _s[0], _cs, *_s[1:]), _rz("dense", _dt, NHWC, _s[0], 8, *_s[1:], off=1)]
    # more than 256 threads per row in both directions (blockIdx.y > 0): Wi = 260 planes, Wi * C / VEC = 36 * 64 / VEC, 36 * 6
    RESIZE_CASES += [_rz("dense", _dt, NCHW, 1, 1, 2, 260, 4, 520), _rz("dense", _dt, NHWC, 1, 64, 3, 36, 6, 72),
                     _rz("dense", _dt, NHWC, 1, _cs, 3, 36, 6, 72)]
    # channel slices: (ld * es) % 16 == 0 with an aligned first channel (vectors; two-pass backward when ws is given), ld * es not a
    # multiple of 16 (scalar), first channel not 16-byte aligned (scalar), and the vector form with more than 256 threads per row
    for _s in (RZ_SHAPES[0], RZ_SHAPES[3]):
        RESIZE_CASES += [_rz("slice", _dt, NHWC, _s[0], 8, *_s[1:], ld=24, c0=8), _rz("slice", _dt, NHWC, _s[0], 8, *_s[1:], ld=22, c0=8),
                         _rz("slice", _dt, NHWC, _s[0], 8, *_s[1:], ld=24, c0=3)]
    RESIZE_CASES += [_rz("slice", _dt, NHWC, 1, 64, 3, 36, 6, 72, ld=96, c0=16), _rz("slice", _dt, NHWC, 1, 8, 3, 36, 6, 72, ld=24, c0=3)]


def rz_id(c):
    return f"{c.kind}-{DTN[c.dt]}-{LAY[c.layout]}-{c.n}x{c.c}x{c.hi}x{c.wi}-{c.ho}x{c.wo}" + (f"-off{c.off}" if c.off else "") + \
        (f"-ld{c.ld}c0{c.c0}" if c.ld else "")


def rz_vec(c):
    if c.layout == NCHW:
        return 1
    es = ES[c.dt]
    v = vec_for(c.dt, c.c, [c.off * es, (c.off + c.c0) * es])
    return 1 if (c.ld and (c.ld * es) % 16) else v


def rz_two_pass(c):
    """afan_upsample_bilinear_bwd_slice with a workspace: both passes when every access is a 16-byte vector."""
    es = ES[c.dt]
    return c.kind == "slice" and c.c % VEC[c.dt] == 0 and (c.ld * es) % 16 == 0 and (c.c0 * es) % 16 == 0


def rz_labels(c):
    v, d, lay = rz_vec(c), DTN[c.dt], LAY[c.layout]
    cv = c.c // v if c.layout == NHWC else 1
    wf = "|wide" if c.wo * cv > BLOCK else ""
    wb = "|wide" if c.wi * cv > BLOCK else ""
    out = {f"upsample_fwd|{d}|{lay}|v{v}{wf}", f"upsample_bwd|{d}|{lay}|v{v}{wb}"}
    if rz_two_pass(c):
        out.add(f"upsample_bwd_rows|{d}" + ("|wide" if c.wi * (c.c // VEC[c.dt]) > BLOCK else ""))
    return out


def _rz_fwd(lib, dev, c, x64):
    """Runs the forward entry of the case: (y [N, C, Ho, Wo] CPU, guards intact?)."""
    x = Buf((c.n, c.c, c.hi, c.wi), c.dt, c.layout, dev, c.off, x64)
    if c.kind == "dense":
        y = Buf((c.n, c.c, c.ho, c.wo), c.dt, c.layout, dev, c.off)
        rc = lib.afan_upsample_bilinear_fwd(P(x.flat), P(y.flat), DTC[c.dt], c.layout, c.n, c.c, c.hi, c.wi, c.ho, c.wo, _st())
        return rc, y.nchw(), y.guard_ok() and x.guard_ok()
    wide = Buf((c.n, c.ld, c.ho, c.wo), c.dt, NHWC, dev)
    rc = lib.afan_upsample_bilinear_fwd_slice(P(x.flat), P(wide.flat, c.c0 * ES[c.dt]), DTC[c.dt], c.n, c.c, c.hi, c.wi, c.ho, c.wo, c.ld, _st())
    full = wide.nchw()
    rest = torch.cat([full[:, :c.c0], full[:, c.c0 + c.c:]], 1)
    s = torch.full((1,), SENTINEL, dtype=c.dt)
    return rc, full[:, c.c0:c.c0 + c.c], wide.guard_ok() and bool((rest == s).all())


def _rz_bwd(lib, dev, c, dy64, ws):
    dx = Buf((c.n, c.c, c.hi, c.wi), c.dt, c.layout, dev, c.off)
    if c.kind == "dense":
        dy = Buf((c.n, c.c, c.ho, c.wo), c.dt, c.layout, dev, c.off, dy64)
        rc = lib.afan_upsample_bilinear_bwd(P(dy.flat), P(dx.flat), DTC[c.dt], c.layout, c.n, c.c, c.hi, c.wi, c.ho, c.wo, _st())
        return rc, dx.nchw(), dx.guard_ok()
    full = torch.full((c.n, c.ld, c.ho, c.wo), 3.0, dtype=torch.float64)          # (other channels: values that would show in a sum)
    full[:, c.c0:c.c0 + c.c] = dy64
    wide = Buf((c.n, c.ld, c.ho, c.wo), c.dt, NHWC, dev, 0, full)
    wsb = None
    if ws:
        wsb = torch.full((int(lib.afan_upsample_bilinear_bwd_workspace_floats(c.n, c.c, c.wi, c.ho)) + 4,), SENTINEL, dtype=F32, device=dev)
    rc = lib.afan_upsample_bilinear_bwd_slice(P(wide.flat, c.c0 * ES[c.dt]), P(dx.flat), DTC[c.dt], c.n, c.c, c.hi, c.wi, c.ho, c.wo, c.ld,
                                              P(wsb), _st())
    ok = dx.guard_ok() and (wsb is None or bool((wsb[-4:] == SENTINEL).all()))
    return rc, dx.nchw(), ok


@pytest.mark.parametrize("case", RESIZE_CASES, ids=rz_id)
def test_resize_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    rep = Report(f"afan_upsample_bilinear {rz_id(c)} expected vector width {rz_vec(c)}" + (" (two-pass with ws)" if rz_two_pass(c) else ""))
    g = torch.Generator().manual_seed(_seed(c, 1))
    in_shape, out_shape = (c.n, c.c, c.hi, c.wi), (c.n, c.c, c.ho, c.wo)
    runs = [False] + ([True] if R.dyadic(c.hi, c.ho) and R.dyadic(c.wi, c.wo) else [])
    ky, kx = R.resize_terms(c.hi, c.ho), R.resize_terms(c.wi, c.wo)
    uy = torch.from_numpy(R.axis_src_ulp(c.hi, c.ho)).view(1, 1, -1, 1)
    ux = torch.from_numpy(R.axis_src_ulp(c.wi, c.wo)).view(1, 1, 1, -1)
    for exact in runs:
        if exact:
            x64, dy64 = R.ints(in_shape, 64, g), R.ints(out_shape, 64, g)
            assert float(x64.abs().max()) <= 64 and float(dy64.abs().max()) <= 64
        else:
            x64, dy64 = q_(torch.randn(in_shape, generator=g), c.dt), q_(torch.randn(out_shape, generator=g), c.dt)
        tag = "exact" if exact else "gauss"
        ref, s, taps = R.resize_fwd(x64, c.ho, c.wo)
        rc, y, ok = _rz_fwd(lib, gpu, c, x64)
        rep.expect(rc == 0, f"forward returned {rc}")
        rep.expect(ok, f"forward {tag}: wrote outside its tensor / channel slice")
        if rc == 0:
            if exact:
                check_exact(rep, "forward exact", y, ref)
            else:
                check_window(rep, "forward", y, ref, C_RESIZE_FWD * U * s + (uy + ux) * taps)
        dref, sb = R.resize_bwd(dy64, c.hi, c.wi)
        tb = torch.einsum("oi,ncop,pj->ncij", torch.from_numpy((R.axis_matrix(c.hi, c.ho) != 0) * 1.0), dy64.abs(),
                          torch.from_numpy((R.axis_matrix(c.wi, c.wo) != 0) * 1.0))
        noise = (ky * kx + C_RESIZE_BWD_EXTRA) * U * sb + (float(uy.max()) + float(ux.max())) * tb
        for ws in ([False, True] if c.kind == "slice" else [False]):
            rc, dx, ok = _rz_bwd(lib, gpu, c, dy64, ws)
            nm = f"backward {tag}" + (" ws" if ws else "")
            rep.expect(rc == 0, f"{nm} returned {rc}")
            rep.expect(ok, f"{nm}: wrote outside its tensor / workspace")
            if rc == 0:
                if exact:
                    check_exact(rep, nm, dx, dref)
                else:
                    check_window(rep, nm, dx, dref, noise)
    rep.done()


# ====================================================================================================================== max pooling
MP = collections.namedtuple("MP", "dt layout n c hi wi k s p off")
MP_GEO = [(9, 11, 3, 2, 1), (8, 6, 2, 2, 0), (7, 7, 7, 1, 0), (11, 9, 5, 3, 2), (9, 9, 15, 1, 7), (1, 1, 3, 2, 1)]
MAXPOOL_CASES = []
for _dt in (F32, BF16):
    _cs = {F32: 6, BF16: 12}[_dt]
    for _g in MP_GEO:
        MAXPOOL_CASES += [MP(_dt, NCHW, 2, 3, *_g, 0), MP(_dt, NHWC, 2, 8, *_g, 0), MP(_dt, NHWC, 2, _cs, *_g, 0), MP(_dt, NHWC, 2, 8, *_g, 1)]
    # more work items than grid_for(total, 256, 4096) launches threads for, in both directions (2 x 2 / 1: input ~ output)
    _v = VEC[_dt]
    MAXPOOL_CASES += [MP(_dt, NCHW, 1, 3, 600, 600, 2, 1, 0, 0), MP(_dt, NHWC, 1, _cs, 300 * (12 // _cs), 300, 2, 1, 0, 0),
                      MP(_dt, NHWC, 1, _v, 1030, 1030, 2, 1, 0, 0)]


def mp_id(c):
    return f"{DTN[c.dt]}-{LAY[c.layout]}-{c.n}x{c.c}x{c.hi}x{c.wi}-k{c.k}s{c.s}p{c.p}" + (f"-off{c.off}" if c.off else "")


def mp_vec(c):
    return 1 if c.layout == NCHW else vec_for(c.dt, c.c, [c.off * ES[c.dt]])


def mp_labels(c):
    v, d, lay = mp_vec(c), DTN[c.dt], LAY[c.layout]
    ho, wo = R.pool_out(c.hi, c.k, c.s, c.p), R.pool_out(c.wi, c.k, c.s, c.p)
    cf = "|cap" if c.n * c.c * ho * wo // v > CAP_4096 else ""
    cb = "|cap" if c.n * c.c * c.hi * c.wi // v > CAP_4096 else ""
    return {f"maxpool_fwd|{d}|{lay}|v{v}{cf}", f"maxpool_bwd|{d}|{lay}|v{v}|scan{cb}", f"maxpool_bwd|{d}|{lay}|v{v}|idx{cb}"}


def pool_input(shape, dt, gen):
    """Post-ReLU values (ties at 0), a plane of -inf, NaNs at the first, a middle and the last position of windows."""
    x = q_(torch.randn(shape, generator=gen).clamp_min(0.0), dt).numpy()
    n, c, h, w = shape
    if c > 1:
        x[0, 1] = -np.inf
    if h >= 3 and w >= 3:
        x[0, 0, 0, 0] = np.nan
        x[-1, 0, h // 2, w // 2] = np.nan
        x[-1, 0, 1, 1] = np.nan
        x[-1, -1, -1, -1] = np.nan
    return x


@pytest.mark.parametrize("case", MAXPOOL_CASES, ids=mp_id)
def test_maxpool_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    rep = Report(f"afan_maxpool2d {mp_id(c)} expected vector width {mp_vec(c)}")
    g = torch.Generator().manual_seed(_seed(c, 2))
    shape = (c.n, c.c, c.hi, c.wi)
    ho, wo = R.pool_out(c.hi, c.k, c.s, c.p), R.pool_out(c.wi, c.k, c.s, c.p)
    oshape = (c.n, c.c, ho, wo)
    x64 = pool_input(shape, c.dt, g)
    yref, iref = R.maxpool_fwd(x64, c.k, c.s, c.p)
    yref_t = torch.from_numpy(yref)
    x = Buf(shape, c.dt, c.layout, gpu, c.off, torch.from_numpy(x64))
    geo = (DTC[c.dt], c.layout, c.n, c.c, c.hi, c.wi, c.k, c.s, c.p)
    idx = None
    for with_idx in (True, False):
        y = Buf(oshape, c.dt, c.layout, gpu, c.off)
        ib = Buf(oshape, torch.uint8, c.layout, gpu, 0, fill=201) if with_idx else None
        rc = lib.afan_maxpool2d_fwd(P(x.flat), P(y.flat), P(ib.flat) if ib else None, *geo, _st())
        nm = "forward" + (" idx" if with_idx else " idx=NULL")
        rep.expect(rc == 0, f"{nm} returned {rc}")
        if rc:
            rep.done()
        check_exact(rep, nm, y.nchw(), yref_t)
        rep.expect(y.guard_ok(), f"{nm}: wrote outside y")
        if ib is not None:
            idx = ib
            got_i = ib.nchw().numpy()
            bad = got_i != iref
            rep.expect(not bad.any(), f"{nm}: {int(bad.sum())} position bytes differ; first at {tuple(np.argwhere(bad)[0]) if bad.any() else ()}")
            rep.expect(ib.guard_ok(), f"{nm}: wrote outside idx")
    terms = None
    # (name, gradient, x given, idx given): re-scan with integer gradients, position bytes with Gaussian gradients, bytes alone
    for nm, exact, use_x, use_idx in (("backward scan", True, True, False), ("backward idx", False, True, True), ("backward idx x=NULL", True, False, True)):
        dy64 = R.ints(oshape, 3, g) if exact else q_(torch.randn(oshape, generator=g), c.dt)
        dref, sa, terms = R.maxpool_bwd(dy64.numpy(), iref, c.hi, c.wi, c.k, c.s, c.p)
        dy = Buf(oshape, c.dt, c.layout, gpu, c.off, dy64)
        dx = Buf(shape, c.dt, c.layout, gpu, c.off)
        rc = lib.afan_maxpool2d_bwd(P(dy.flat), P(x.flat) if use_x else None, P(idx.flat) if use_idx else None, P(dx.flat), *geo, _st())
        rep.expect(rc == 0, f"{nm} returned {rc}")
        if rc:
            continue
        rep.expect(dx.guard_ok(), f"{nm}: wrote outside dx")
        if exact:
            check_exact(rep, nm, dx.nchw(), torch.from_numpy(dref))
        else:       # at most `terms` gradients meet in one input: terms - 1 fp32 additions
            check_window(rep, nm, dx.nchw(), torch.from_numpy(dref), max(terms - 1, 0) * U * torch.from_numpy(sa))
    rep.done()


# ================================================================================================================== average pooling
AP_HW, AP_C, AP_N = (1, 15, 16, 17, 32, 33, 81), (8, 64, 72, 200), 3
AP_PAIRS = [(F32, F32), (BF16, F32), (BF16, BF16)]                 # (map, pooled side)
AVGPOOL_CASES = [(lay, pair) for lay in (NCHW, NHWC) for pair in AP_PAIRS]
AP_CAP_SHAPE = (3, 72, 4900)                                        # n * c * hw = 1 058 400 > 4096 * 256


def ap_labels(lay, pair, shapes):
    name = f"{DTN[pair[0]]}→{DTN[pair[1]]}"
    out = {f"avgpool_{LAY[lay]}|{name}"}
    for n, c, hw in shapes:
        out.add(f"avgpool_bwd|{LAY[lay]}|{name}" + ("|cap" if n * c * hw > CAP_4096 else ""))
    return out


def _ap_shapes():
    return [(AP_N, c, hw) for hw in AP_HW for c in AP_C] + [AP_CAP_SHAPE]


@pytest.mark.parametrize("lay,pair", AVGPOOL_CASES, ids=lambda v: LAY[v] if isinstance(v, int) else f"{DTN[v[0]]}-{DTN[v[1]]}")
def test_avgpool_pinned(pkg, gpu, lay, pair):
    lib = pkg._lib.load()
    dt, dp = pair
    pf = int(dp == F32 and dt == BF16)
    rep = Report(f"afan_avgpool {LAY[lay]} {DTN[dt]}→{DTN[dp]}")
    g = torch.Generator().manual_seed(_seed((lay, DTN[dt], DTN[dp]), 3))
    for n, c, hw in _ap_shapes():
        sh = f"{n}x{c}x{hw}"
        x64 = q_(torch.randn((n, c, hw, 1), generator=g) + 0.25, dt)
        x = Buf((n, c, hw, 1), dt, lay, gpu, 0, x64)
        y = Buf((n, c, 1, 1), dp, NCHW, gpu)
        rc = lib.afan_avgpool_fwd(P(x.flat), P(y.flat), DTC[dt], lay, n, c, hw, pf, _st())
        rep.expect(rc == 0, f"forward {sh} returned {rc}")
        ref, s = R.avgpool_fwd(x64[..., 0])
        if rc == 0:      # fp32 summation of hw terms: hw * 2^-24 * mean |x|; a bf16 pooled side adds its one RNE rounding (the window)
            check_window(rep, f"forward {sh}", y.nchw()[:, :, 0, 0], ref, hw * U * s)
            rep.expect(y.guard_ok(), f"forward {sh}: wrote outside y")
        # backward: dx = fl(dy * fl32(1 / hw)) broadcast, one product in fp32 rounded to the map's type: exact by construction
        dy64 = q_(torch.randn((n, c, 1, 1), generator=g), dp)
        dy = Buf((n, c, 1, 1), dp, NCHW, gpu, 0, dy64)
        dx = Buf((n, c, hw, 1), dt, lay, gpu)
        rc = lib.afan_avgpool_bwd(P(dy.flat), P(dx.flat), DTC[dt], lay, n, c, hw, pf, _st())
        rep.expect(rc == 0, f"backward {sh} returned {rc}")
        if rc == 0:
            inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(hw), dtype=F32)
            want = (dy64.float() * inv).to(dt).expand(n, c, hw, 1)
            got = dx.nchw()
            nb = int((got != want).sum())
            rep.expect(nb == 0, f"backward {sh}: {nb} of {got.numel()} elements differ from fl(dy * fl32(1 / hw))")
            rep.expect(dx.guard_ok(), f"backward {sh}: wrote outside dx")
    rep.done()


# ==================================================================================================================== cross-entropy
CE = collections.namedtuple("CE", "layout n c h w ignore mode")
CE_CASES = [CE(lay, 2, c, 7, 23, 255, "mixed") for lay in (NCHW, NHWC) for c in (1, 2, 21, 32)]
for _lay in (NCHW, NHWC):
    CE_CASES += [CE(_lay, 2, 21, 7, 23, 255, "all_ignored"), CE(_lay, 2, 21, 7, 23, 255, "one_live"), CE(_lay, 2, 21, 7, 23, -100, "mixed"),
                 CE(_lay, 2, 21, 7, 23, 255, "no_grad"), CE(_lay, 2, 21, 7, 23, 255, "pm80"),
                 # P = 524 588 > 2048 * 256 pixels: the second trip of the grid-stride loops (LDS re-staged in the channels-last kernel)
                 CE(_lay, 2, 3, 451, 582, 255, "mixed"), CE(_lay, 2, 3, 451, 582, 255, "bad_target_second_trip")]


def ce_id(c):
    return f"{LAY[c.layout]}-{c.n}x{c.c}x{c.h}x{c.w}-ign{c.ignore}-{c.mode}"


def ce_labels(c):
    return {f"ce2d|{LAY[c.layout]}" + ("|cap" if c.n * c.h * c.w > CAP_2048 else "")}


def ce_target(shape, c, ignore, mode, gen):
    t = torch.randint(0, c, shape, generator=gen)
    if mode == "all_ignored":
        t[:] = ignore
    elif mode == "one_live":
        keep = t[-1, -2, -3].item()
        t[:] = ignore
        t[-1, -2, -3] = keep
    else:
        t[torch.rand(shape, generator=gen) < 0.2] = ignore
    return t


def run_ce(lib, dev, layout, logits64, t, ignore, gs, want_grad=True):
    n, c, h, w = logits64.shape
    x = Buf((n, c, h, w), F32, layout, dev, 0, logits64)
    td = t.to(dev)
    ws = torch.zeros(int(lib.afan_ce2d_workspace_floats(n * h * w)), dtype=F32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=F32, device=dev)
    dl = Buf((n, c, h, w), F32, layout, dev) if want_grad else None
    rc = lib.afan_ce2d(P(x.flat), P(td), layout, n, c, h * w, ignore, gs, P(ws), P(loss), P(dl.flat) if dl else None, _st())
    return rc, loss.cpu().double()[0], dl


def check_ce(rep, nm, loss, dl, lref, gref, count, gs, loss_noise=0.0, grad_noise=None):
    lu = U * max(1.0, abs(float(lref)))
    rl = abs(float(loss) - float(lref)) / lu if np.isfinite(float(loss)) else float("inf")
    rep.figure(f"{nm}_loss", max(0.0, (abs(float(loss) - float(lref)) - loss_noise)) / lu if np.isfinite(float(loss)) else float("inf"))
    rep.expect(abs(float(loss) - float(lref)) <= C_CE_LOSS * lu + loss_noise, f"{nm} loss {float(loss)!r} vs float64 {float(lref)!r}: {rl:.2f} units of "
               f"2^-24 max(1, |loss|), limit {C_CE_LOSS}")
    if dl is not None:
        got = dl.nchw()
        unit = U * gs / count
        extra = torch.zeros_like(gref) if grad_noise is None else grad_noise
        rep.figure(f"{nm}_grad", float((((got.double() - gref).abs() - extra).clamp_min(0.0) / unit).max()))
        check_window(rep, f"{nm} gradient (C_CE {C_CE_GRAD} units of 2^-24 grad_scale / count)", got, gref, C_CE_GRAD * unit + extra)
        rep.expect(dl.guard_ok(), f"{nm}: wrote outside dlogits")


@pytest.mark.parametrize("case", CE_CASES, ids=ce_id)
def test_ce2d_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    rep = Report(f"afan_ce2d f32 {ce_id(c)}")
    g = torch.Generator().manual_seed(_seed(c, 4))
    shape = (c.n, c.c, c.h, c.w)
    if c.mode == "pm80":
        x64 = torch.where(torch.rand(shape, generator=g) < 0.5, 80.0, -80.0).double()
    else:
        x64 = q_(torch.randn(shape, generator=g) * 3.0, F32)
    t = ce_target((c.n, c.h, c.w), c.c, c.ignore, c.mode, g)
    gs = 0.7
    if c.mode == "bad_target_second_trip":
        assert c.n * c.h * c.w - 7 >= CAP_2048
        t.view(-1)[-7] = c.c                 # not the ignore index, not a class: the loss is poisoned
        rc, loss, dl = run_ce(lib, gpu, c.layout, x64, t, c.ignore, gs)
        rep.expect(rc == 0, f"returned {rc}")
        rep.expect(bool(torch.isnan(loss)), f"an out-of-range target in the second grid-stride trip left the loss at {float(loss)!r}")
        rep.expect(bool(torch.isfinite(dl.nchw()).all()), "non-finite gradient")
        rep.done()
        return
    lref, gref, count = R.ce2d(x64, t, c.ignore, gs)
    rc, loss, dl = run_ce(lib, gpu, c.layout, x64, t, c.ignore, gs, want_grad=c.mode != "no_grad")
    rep.expect(rc == 0, f"returned {rc}")
    if c.mode == "all_ignored":
        rep.expect(bool(torch.isnan(loss)), f"no live pixel: loss {float(loss)!r}, expected NaN")
        rep.expect(float(dl.nchw().abs().max()) == 0.0, "no live pixel: non-zero gradient")
    elif rc == 0:
        check_ce(rep, "ce2d", loss, dl, lref, gref, count, gs)
    rep.done()


# ------------------------------------------------------------------------------------------------- fused resize + cross-entropy
UP = collections.namedtuple("UP", "n c h w ho wo mode")
UP_CASES = [UP(3, 21, 1, 1, 4, 4, "mixed"),               # windows of 2
            UP(1, 32, 7, 7, 7, 7, "mixed"),               # windows of 8, one ragged tile
            UP(2, 1, 20, 17, 48, 40, "mixed"),            # windows of 8 / 8, ragged columns
            UP(1, 21, 9, 13, 33, 41, "last_tile_ignored"),  # windows of 6 / 7, ragged both ways
            UP(1, 21, 9, 13, 33, 41, "no_grad"), UP(2, 21, 9, 13, 33, 41, "one_live"),
            UP(3, 32, 105, 105, 315, 315, "mixed")]       # gather over 3 * 105 * 105 * 32 = 1 058 400 > 4096 * 256 elements
UP_DECLINED = [(33, 65), (65, 129), (40, 64), (16, 16), (33, 33)]


def up_id(c):
    return f"{c.n}x{c.c}x{c.h}x{c.w}-{c.ho}x{c.wo}-{c.mode}"


def up_labels(c):
    out = {"ce2d_up"}
    if c.mode != "no_grad":
        out.add("ce2d_up_gather" + ("|cap" if c.n * c.h * c.w * c.c > CAP_4096 else ""))
    return out


def fused_reference(x64, t, ignore, gs, extra_bwd):
    """Float64 loss and low-resolution gradient of cross-entropy on the resized logits, and the noise both may carry: the forward
    resize's bound on every interpolated logit (the loss and the soft-max are 2-Lipschitz in the largest logit error), C_CE on the
    full-resolution gradient, all of it carried through the adjoint, plus the adjoint's own summation."""
    n, c, h, w = x64.shape
    ho, wo = t.shape[1:]
    up, s, taps = R.resize_fwd(x64, ho, wo)
    uy = torch.from_numpy(R.axis_src_ulp(h, ho)).view(1, 1, -1, 1)
    ux = torch.from_numpy(R.axis_src_ulp(w, wo)).view(1, 1, 1, -1)
    nlog = (C_RESIZE_FWD * U * s + (uy + ux) * taps).amax(1, keepdim=True)
    lref, gup, count = R.ce2d(up, t, ignore, gs)
    if count == 0:
        return lref, torch.zeros_like(x64), 0, 0.0, torch.zeros_like(x64)
    live = (t != ignore)[:, None].double()
    nup = (C_CE_GRAD * U + 2.0 * nlog) * (gs / count) * live.expand_as(gup)
    dref, sb = R.resize_bwd(gup, h, w)
    k = R.resize_terms(h, ho) * R.resize_terms(w, wo) + extra_bwd
    noise = R.resize_bwd(nup, h, w)[0] + k * U * sb
    return lref, dref, count, 2.0 * float(nlog.max()), noise


def run_up(lib, dev, x64, t, ignore, gs, want_grad=True):
    n, c, h, w = x64.shape
    ho, wo = t.shape[1:]
    x = Buf((n, c, h, w), F32, NHWC, dev, 0, x64)
    td = t.to(dev)
    ws = torch.zeros(max(1, int(lib.afan_ce2d_upsampled_workspace_floats(n, c, h, w, ho, wo))), dtype=F32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=F32, device=dev)
    dl = Buf((n, c, h, w), F32, NHWC, dev)
    rc = lib.afan_ce2d_upsampled(P(x.flat), P(td), n, c, h, w, ho, wo, ignore, gs, P(ws), P(loss), P(dl.flat) if want_grad else None, _st())
    return rc, loss.cpu(), dl


@pytest.mark.parametrize("case", UP_CASES, ids=up_id)
def test_ce2d_upsampled_pinned(pkg, gpu, case):
    c, lib = case, pkg._lib.load()
    rep = Report(f"afan_ce2d_upsampled f32 nhwc {up_id(c)}")
    assert lib.afan_ce2d_upsampled_supported(c.c, c.h, c.w, c.ho, c.wo) == 1
    g = torch.Generator().manual_seed(_seed(c, 5))
    x64 = q_(torch.randn((c.n, c.c, c.h, c.w), generator=g) * 3.0, F32)
    t = ce_target((c.n, c.ho, c.wo), c.c, 255, c.mode, g)
    if c.mode == "last_tile_ignored":
        t[:, 32:, 32:] = 255
    gs = 0.7
    lref, dref, count, lnoise, noise = fused_reference(x64, t, 255, gs, C_FUSED_BWD_EXTRA)
    rc, loss, dl = run_up(lib, gpu, x64, t, 255, gs, want_grad=c.mode != "no_grad")
    rep.expect(rc == 0, f"returned {rc}")
    if rc == 0:
        if c.mode == "no_grad":
            rep.expect(bool((dl.raw == SENTINEL).all()), "dlogits = NULL: the buffer next to the inputs was written")
            dl = None
        check_ce(rep, "fused", loss.double()[0], dl, lref, dref, count, gs, lnoise, noise)
        if c.mode == "one_live":
            # one live pixel: the loss is that pixel's own term over a count of 1, no sum is regrouped: the header's "to the bit"
            xb = Buf(x64.shape, F32, NHWC, gpu, 0, x64)
            up = Buf((c.n, c.c, c.ho, c.wo), F32, NHWC, gpu)
            rc = lib.afan_upsample_bilinear_fwd(P(xb.flat), P(up.flat), 0, NHWC, c.n, c.c, c.h, c.w, c.ho, c.wo, _st())
            rc2, l3, _ = run_ce(lib, gpu, NHWC, up.nchw().double(), t, 255, gs)
            rep.expect(rc == 0 and rc2 == 0, "the three-kernel path failed")
            rep.expect(float(l3) == float(loss[0]), f"one live pixel: fused loss {float(loss[0])!r} != resize + ce2d {float(l3)!r}")
    rep.done()


def test_ce2d_upsampled_query_agrees_with_entry(pkg, gpu):
    """The host query against the entry point's return code: the entry point runs only where the query says yes, plus the few declined
    shapes of UP_DECLINED, which must return AFAN_ESHAPE and leave loss and gradient untouched."""
    lib = pkg._lib.load()
    rep = Report("afan_ce2d_upsampled_supported")
    g = torch.Generator().manual_seed(6)
    pairs = [(1, 4), (9, 33), (5, 7), (13, 41), (7, 7), (20, 48), (17, 40), (33, 129)] + UP_DECLINED
    for h, ho in pairs:
        q = lib.afan_ce2d_upsampled_supported(3, h, 5, ho, 20)
        x64 = q_(torch.randn((1, 3, h, 5), generator=g), F32)
        t = torch.randint(0, 3, (1, ho, 20), generator=g)
        if q or (h, ho) in UP_DECLINED:
            rc, loss, dl = run_up(lib, gpu, x64, t, 255, 1.0)
            rep.expect((rc == 0) == bool(q) and rc in (0, ESHAPE), f"{h}->{ho}: query {q}, entry point returned {rc}")
            if not q:
                rep.expect(float(loss[0]) == SENTINEL and bool((dl.raw == SENTINEL).all()), f"{h}->{ho}: a declined call wrote its outputs")
    # a grid of pairs: the query restated from the reference's index table (the source rows a 16-row output tile reads fit 8)
    for h in (1, 2, 5, 7, 8, 16, 17, 33, 40, 65):
        for ho in sorted({h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1, 3 * h, 4 * h - 3, 4 * h, 513}):
            if ho < h:
                continue
            i0 = R.axis_table(h, ho)[0]
            win = max(int(i0[min(y0 + 16, ho) - 1]) + 1 - int(i0[y0]) + 1 for y0 in range(0, ho, 16))
            rep.expect(lib.afan_ce2d_upsampled_supported(21, h, h, ho, ho) == int(win <= 8), f"{h}->{ho}: window {win}, query disagrees")
    rep.done()


@pytest.mark.parametrize("size", [65, 33])
def test_seg_criterion_falls_back_where_the_fused_kernel_declines(pkg, gpu, size):
    """33 -> 65 and 33 -> 33: the fused kernel declines (source window of a tile: 10 and 17 rows); the criterion resizes, then ce2d."""
    rep = Report(f"seg_criterion 2x21x33x33 -> {size}x{size}")
    g = torch.Generator().manual_seed(7 + size)
    x64 = q_(torch.randn((2, 21, 33, 33), generator=g) * 3.0, F32)
    t = ce_target((2, size, size), 21, 255, "mixed", g)
    logits = x64.float().to(gpu).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert not pkg.ops.ce2d_upsampled_ok(logits, (size, size))
    ce = pkg.deeplab.seg_criterion(torch.nn.CrossEntropyLoss(ignore_index=255))
    loss = ce(pkg.deeplab.LowResLogits(logits, (size, size)), t.to(gpu))
    loss.backward()
    lref, dref, count, lnoise, noise = fused_reference(x64, t, 255, 1.0, C_RESIZE_BWD_EXTRA)
    lu = U * max(1.0, abs(float(lref)))
    rep.figure("criterion_loss", abs(float(loss) - float(lref)) / lu)
    rep.expect(abs(float(loss) - float(lref)) <= C_CE_LOSS * lu + lnoise, f"loss {float(loss)!r} vs float64 {float(lref)!r}")
    check_window(rep, "low-resolution gradient", logits.grad.cpu().contiguous(), dref, C_CE_GRAD * U / count + noise)
    rep.done()


# ============================================================================================================== pointwise classifier
PW_CI, PW_CO, PW_M = (8, 64, 256, 264, 512), (1, 3, 21, 32), (1, 63, 64, 65)
PW_BIG_M = PW_CAP_M + 64 + 5                                    # more slices than pw_blocks launches workgroups, ragged last slice
POINTWISE_CASES = [(dt, ci) for dt in (F32, BF16) for ci in PW_CI] + [(F32, -8), (BF16, -8)]      # (-8: ci = 8 at PW_BIG_M)


def pw_shapes(ci):
    if ci < 0:
        return [(PW_BIG_M, -ci, 21)]
    return [(m, ci, co) for co in PW_CO for m in PW_M if ci * co * 4 <= 64 * 1024]


def pw_labels(dt, ci):
    d, out = DTN[dt], set()
    for m, cin, co in pw_shapes(ci):
        out |= {f"pointwise_fwd|{d}", f"pointwise_dx|{d}", f"pointwise_dw|{d}|chunks{-(-cin // PW_CHUNK)}" + ("|cap" if m > PW_CAP_M else "")}
    return out


@pytest.mark.parametrize("dt,ci", POINTWISE_CASES, ids=lambda v: DTN[v] if not isinstance(v, int) else f"ci{v}" if v > 0 else "ci8-slices-over-cap")
def test_pointwise_pinned(pkg, gpu, dt, ci):
    lib = pkg._lib.load()
    rep = Report(f"afan_pointwise x {DTN[dt]} ci {abs(ci)}")
    g = torch.Generator().manual_seed(_seed((DTN[dt], ci), 8))
    dev = gpu
    for k, (m, cin, co) in enumerate(pw_shapes(ci)):
        for exact in (True, False):
            sh = f"m {m} ci {cin} co {co} " + ("exact" if exact else "gauss")
            if exact:
                x64, w64, dy64 = R.ternary((m, cin), g), R.ternary((co, cin), g), R.ternary((m, co), g)
                b64, dw0, db0 = R.ints((co,), 3, g), R.ints((co, cin), 3, g), R.ints((co,), 3, g)
                assert R.products_exact(x64, w64.t()) and R.products_exact(dy64, w64) and R.products_exact(dy64.t(), x64)
            else:
                x64, w64, dy64 = q_(torch.randn((m, cin), generator=g), dt), q_(torch.randn((co, cin), generator=g), F32), q_(torch.randn((m, co), generator=g), F32)
                b64, dw0, db0 = q_(torch.randn(co, generator=g), F32), q_(torch.randn((co, cin), generator=g), F32), q_(torch.randn(co, generator=g), F32)
            use_b, use_db, acc = (k + exact) % 2 == 0, (k // 2 + exact) % 2 == 0, int((k + exact) % 3 == 0)
            xd, wd, dyd = x64.to(dt).to(dev), w64.float().to(dev), dy64.float().to(dev)
            bd = b64.float().to(dev) if use_b else None
            y = torch.full((m * co + 8,), SENTINEL, dtype=F32, device=dev)
            rc = lib.afan_pointwise_fwd(P(xd), DTC[dt], P(wd), P(bd), P(y), m, cin, co, _st())
            rep.expect(rc == 0, f"fwd {sh} returned {rc}")
            ref, s = R.pointwise_fwd(x64, w64, b64 if use_b else None)
            if rc == 0:
                got = y[:m * co].cpu().view(m, co)
                rep.expect(bool((y[m * co:] == SENTINEL).all()), f"fwd {sh}: wrote past y")
                check_exact(rep, f"fwd {sh}", got, ref) if exact else check_window(rep, f"fwd {sh}", got, ref, pw_fwd_roundings(dt, cin) * U * s)
            dref, sdx, wref, sdw, bref, sdb = R.pointwise_bwd(dy64, x64, w64)
            dx = torch.full((m * cin + 8,), SENTINEL, dtype=dt, device=dev)
            rc = lib.afan_pointwise_bwd_dx(P(dyd), P(wd), P(dx), DTC[dt], m, cin, co, _st())
            rep.expect(rc == 0, f"dx {sh} returned {rc}")
            if rc == 0:
                got = dx[:m * cin].cpu().view(m, cin)
                rep.expect(bool((dx[m * cin:].float() == torch.tensor(SENTINEL).to(dt).float()).all()), f"dx {sh}: wrote past dx")
                check_exact(rep, f"dx {sh}", got, dref) if exact else check_window(rep, f"dx {sh}", got, dref, co * U * sdx)
            ws = torch.zeros(int(lib.afan_pointwise_workspace_floats(m, cin, co)), dtype=F32, device=dev)
            dw, db = dw0.float().to(dev), (db0.float().to(dev) if use_db else None)
            rc = lib.afan_pointwise_bwd_dw(P(dyd), P(xd), DTC[dt], P(dw), P(db), m, cin, co, P(ws), acc, _st())
            rep.expect(rc == 0, f"dw {sh} returned {rc}")
            if rc == 0:
                wref2, bref2 = (wref + dw0, bref + db0) if acc else (wref, bref)
                if exact:
                    check_exact(rep, f"dw {sh} accumulate {acc}", dw.cpu(), wref2)
                    if use_db:
                        check_exact(rep, f"db {sh} accumulate {acc}", db.cpu(), bref2)
                else:       # (added into dw: one more rounding of the sum)
                    rep.figure("pw_dw", ratio_of(dw.cpu(), wref2, U * (sdw + acc * wref2.abs())))
                    check_window(rep, f"dw {sh} accumulate {acc} (C {C_PW_DW})", dw.cpu(), wref2, C_PW_DW * U * sdw + acc * U * wref2.abs())
                    if use_db:
                        rep.figure("pw_db", ratio_of(db.cpu(), bref2, U * (sdb + acc * bref2.abs())))
                        check_window(rep, f"db {sh} accumulate {acc} (C {C_PW_DB})", db.cpu(), bref2, C_PW_DB * U * sdb + acc * U * bref2.abs())
    rep.done()


# ===================================================================================================================== linear_small
LIN_N, LIN_CI, LIN_CO = (1, 2, 3, 4, 5, 8, 9, 16), (1, 63, 64, 65, 2048), (1, 3, 5, 256)
LDX_WAVES = 16


def lin_bwd_fits(n, co):
    """The host's LDS check of afan_linear_small_bwd: (n * co + 16 * n * 64) floats within 64 KiB."""
    return (n * co + LDX_WAVES * n * 64) * 4 <= 64 * 1024


def lin_labels(n):
    nn = 2 if n <= 2 else 4 if n <= 4 else 8 if n <= 8 else 16
    out = {f"linear_small_fwd<{nn}>"}
    if any(lin_bwd_fits(n, co) for co in LIN_CO):
        out |= {"linear_small_dx", "linear_small_dw"}
    return out


@pytest.mark.parametrize("n", LIN_N)
def test_linear_small_pinned(pkg, gpu, n):
    lib = pkg._lib.load()
    rep = Report(f"afan_linear_small f32 rows {n}")
    g = torch.Generator().manual_seed(_seed(("lin", n), 9))
    dev = gpu
    k = 0
    for ci in LIN_CI:
        for co in LIN_CO:
            for exact in (True, False):
                k += 1
                sh = f"n {n} ci {ci} co {co} " + ("exact" if exact else "gauss")
                if exact:
                    x64, w64, dy64, dw0 = R.ternary((n, ci), g), R.ternary((co, ci), g), R.ternary((n, co), g), R.ints((co, ci), 3, g)
                    assert R.products_exact(x64, w64.t()) and R.products_exact(dy64, w64) and R.products_exact(dy64.t(), x64)
                else:
                    x64, w64, dy64, dw0 = (q_(torch.randn(s_, generator=g), F32) for s_ in ((n, ci), (co, ci), (n, co), (co, ci)))
                xd, wd, dyd = x64.float().to(dev), w64.float().to(dev), dy64.float().to(dev)
                y = torch.full((n * co + 8,), SENTINEL, dtype=F32, device=dev)
                rc = lib.afan_linear_small_fwd(P(xd), P(wd), P(y), n, ci, co, _st())
                rep.expect(rc == 0, f"fwd {sh} returned {rc}")
                ref, s = R.pointwise_fwd(x64, w64, None)
                if rc == 0:
                    got = y[:n * co].cpu().view(n, co)
                    rep.expect(bool((y[n * co:] == SENTINEL).all()), f"fwd {sh}: wrote past y")
                    check_exact(rep, f"fwd {sh}", got, ref) if exact else check_window(rep, f"fwd {sh}", got, ref, (-(-ci // 64) + 6) * U * s)
                dref, sdx, wref, sdw, _, _ = R.pointwise_bwd(dy64, x64, w64)
                acc = k % 2
                dx = torch.full((n * ci + 8,), SENTINEL, dtype=F32, device=dev)
                dw = dw0.float().to(dev)
                if not lin_bwd_fits(n, co):
                    rc = lib.afan_linear_small_bwd(P(dyd), P(xd), P(wd), P(dx), P(dw), n, ci, co, acc, _st())
                    rep.expect(rc == ESHAPE and bool((dx == SENTINEL).all()), f"bwd {sh}: past the LDS check, returned {rc}")
                    continue
                rc1 = lib.afan_linear_small_bwd(P(dyd), P(xd), P(wd), P(dx), None, n, ci, co, acc, _st())       # dw = NULL
                rc2 = lib.afan_linear_small_bwd(P(dyd), P(xd), P(wd), None, P(dw), n, ci, co, acc, _st())       # dx = NULL
                rep.expect(rc1 == 0 and rc2 == 0, f"bwd {sh} returned {rc1}, {rc2}")
                if rc1 == 0 and rc2 == 0:
                    gdx, gdw = dx[:n * ci].cpu().view(n, ci), dw.cpu()
                    rep.expect(bool((dx[n * ci:] == SENTINEL).all()), f"dx {sh}: wrote past dx")
                    wref2 = wref + dw0 if acc else wref
                    if exact:
                        check_exact(rep, f"dx {sh}", gdx, dref)
                        check_exact(rep, f"dw {sh} accumulate {acc}", gdw, wref2)
                    else:
                        check_window(rep, f"dx {sh}", gdx, dref, (-(-co // LDX_WAVES) + LDX_WAVES) * U * sdx)
                        check_window(rep, f"dw {sh} accumulate {acc}", gdw, wref2, n * U * sdw + acc * U * wref2.abs())
    # just past the 64 KiB check: 8 rows fit up to co = 1024
    assert lin_bwd_fits(8, 1024) and not lin_bwd_fits(8, 1025)
    if n == 8:
        z = torch.zeros(8 * 1025 + 8, dtype=F32, device=dev)
        rep.expect(lib.afan_linear_small_bwd(P(z), P(z), P(z), P(z), None, 8, 1, 1025, 0, _st()) == ESHAPE, "n 8 co 1025 was not declined")
    rep.done()


# ========================================================================================================================== dropout
DROPOUT_CASES = [(dt, mode, n) for dt in (F32, BF16) for mode in ("mask", "seed") for n in (1000, CAP_2048 + 300)]


def do_labels(dt, mode, n):
    return {f"dropout|{DTN[dt]}|{mode}" + ("|cap" if n > CAP_2048 else "")}


@pytest.mark.parametrize("dt,mode,n", DROPOUT_CASES, ids=lambda v: DTN.get(v, str(v)) if not isinstance(v, (int, str)) else str(v))
def test_dropout_pinned(pkg, gpu, dt, mode, n):
    lib = pkg._lib.load()
    rep = Report(f"afan_dropout {DTN[dt]} {mode} n {n}")
    g = torch.Generator().manual_seed(_seed((DTN[dt], mode, n), 10))
    x64 = q_(torch.randn(n, generator=g) + 3.0, dt)            # (no zeros: the mask shows in y)
    xd = x64.to(dt).to(gpu)
    y = torch.full((n + 8,), SENTINEL, dtype=dt, device=gpu)
    sent = torch.tensor(SENTINEL).to(dt).float()
    if mode == "mask":
        for p in (0.5, 0.1):
            mask = (torch.rand(n, generator=g) >= p).to(torch.uint8)
            rc = lib.afan_dropout(P(xd), P(y), DTC[dt], n, p, P(mask.to(gpu)), None, None, 0, _st())
            rep.expect(rc == 0, f"p {p} returned {rc}")
            want = R.dropout(x64, p, mask).to(dt)
            rep.expect(torch.equal(y[:n].cpu(), want), f"p {p}: y is not fl(x * fl32(1 / (1 - p))) under the mask")
            rep.expect(bool((y[n:].float() == sent).all()), "wrote past y")
        rc = lib.afan_dropout(P(xd), P(y), DTC[dt], n, 0.0, None, None, None, 0, _st())         # p = 0: the identity, no state needed
        rep.expect(rc == 0 and torch.equal(y[:n], xd), f"p = 0 without a state: returned {rc} or changed x")
    else:
        p = 0.3
        state = torch.tensor([0x1234567], dtype=torch.int64, device=gpu)
        used = torch.zeros(1, dtype=torch.int64, device=gpu)
        rc = lib.afan_dropout(P(xd), P(y), DTC[dt], n, p, None, P(state), P(used), 1, _st())
        rep.expect(rc == 0, f"forward returned {rc}")
        kept = (y[:n].float() != 0).cpu()
        rep.expect(int(used.cpu()[0]) == 0x1234567 and int(state.cpu()[0]) != 0x1234567, "the forward did not publish / advance its seed")
        want = R.dropout(x64, p, kept.to(torch.uint8)).to(dt)
        rep.expect(torch.equal(y[:n].cpu(), want), "kept elements are not fl(x * fl32(1 / (1 - p)))")
        gd = q_(torch.randn(n, generator=g) + 3.0, dt).to(dt).to(gpu)
        dx = torch.full((n + 8,), SENTINEL, dtype=dt, device=gpu)
        rc = lib.afan_dropout(P(gd), P(dx), DTC[dt], n, p, None, None, P(used), 0, _st())     # the backward: the mask from `used`
        rep.expect(rc == 0, f"backward returned {rc}")
        rep.expect(torch.equal((dx[:n].float() != 0).cpu(), kept), "the backward's mask differs from the forward's")
        rep.expect(bool((dx[n:].float() == sent).all()) and bool((y[n:].float() == sent).all()), "wrote past its output")
        rep.expect(abs(float(kept.double().mean()) - (1 - p)) < 0.05, "keep rate far from 1 - p")
    rep.done()


# ========================================================================================================================= coverage
def _dense_variants(name, extra=("",)):
    return [f"{name}|{d}|{lay}|v{v}{e}" for d, vv in (("f32", 4), ("bf16", 8)) for lay, v in (("nchw", 1), ("nhwc", vv), ("nhwc", 1)) for e in extra]


EXPECTED_VARIANTS = sorted(
    _dense_variants("upsample_fwd", ("", "|wide")) + _dense_variants("upsample_bwd", ("", "|wide")) +
    [f"upsample_bwd_rows|{d}{e}" for d in ("f32", "bf16") for e in ("", "|wide")] +
    _dense_variants("maxpool_fwd", ("", "|cap")) + _dense_variants("maxpool_bwd", ("|scan", "|idx", "|scan|cap", "|idx|cap")) +
    [f"avgpool_{lay}|{p}" for lay in ("nchw", "nhwc") for p in ("f32→f32", "bf16→f32", "bf16→bf16")] +
    [f"avgpool_bwd|{lay}|{p}{e}" for lay in ("nchw", "nhwc") for p in ("f32→f32", "bf16→f32", "bf16→bf16") for e in ("", "|cap")] +
    ["ce2d|nchw", "ce2d|nchw|cap", "ce2d|nhwc", "ce2d|nhwc|cap", "ce2d_up", "ce2d_up_gather", "ce2d_up_gather|cap"] +
    [f"pointwise_{k}|{d}" for k in ("fwd", "dx") for d in ("f32", "bf16")] +
    [f"pointwise_dw|{d}|{e}" for d in ("f32", "bf16") for e in ("chunks1", "chunks2", "chunks1|cap")] +
    ["linear_small_fwd<2>", "linear_small_fwd<4>", "linear_small_fwd<8>", "linear_small_fwd<16>", "linear_small_dx", "linear_small_dw"] +
    [f"dropout|{d}|{m}{e}" for d in ("f32", "bf16") for m in ("mask", "seed") for e in ("", "|cap")])


def table_variants():
    got = set()
    for c in RESIZE_CASES:
        got |= rz_labels(c)
    for c in MAXPOOL_CASES:
        got |= mp_labels(c)
    for lay, pair in AVGPOOL_CASES:
        got |= ap_labels(lay, pair, _ap_shapes())
    for c in CE_CASES:
        got |= ce_labels(c)
    for c in UP_CASES:
        got |= up_labels(c)
    for dt, ci in POINTWISE_CASES:
        got |= pw_labels(dt, ci)
    for n in LIN_N:
        got |= lin_labels(n)
    for case in DROPOUT_CASES:
        got |= do_labels(*case)
    return got


def test_table_reaches_every_instantiation():
    """Pure Python: every table row mapped to the variants it reaches by the restated dispatch conditions.  The set must be exactly
    EXPECTED_VARIANTS: every AFAN_SEG_DISPATCH instantiation of resize and max pooling, the two-pass backward, the (T, TP) pairs of the
    average pool, every linear_small_fwd<NN>, both channel chunks of pointwise_dw_kernel - and for every kernel with a capped grid a
    row past the cap ("|cap": a second grid-stride trip; resize: "|wide", blockIdx.y > 0)."""
    got = table_variants()
    assert sorted(got) == EXPECTED_VARIANTS, f"missing {sorted(set(EXPECTED_VARIANTS) - got)}, unexpected {sorted(got - set(EXPECTED_VARIANTS))}"
    # the fused kernel's window extremes and declined shapes are in the tables
    assert (1, 4) in {(c.h, c.ho) for c in UP_CASES} and (7, 7) in {(c.h, c.ho) for c in UP_CASES}
