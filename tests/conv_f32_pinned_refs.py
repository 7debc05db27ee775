"""Float64 references of the general fp32-arithmetic convolutions (csrc/afan_conv_f32.hip: afan_conv_fwd / afan_conv_dgrad /
afan_conv_wgrad), written from the definition with loops over the taps and slicing (no library convolution), with the scale S (the
same operation on absolute values, plus |bias|) and the per-element count of products whose operands lie inside the image (a masked
product adds an exact zero and rounds nothing).  The case table, the operand generators and the host-side dispatch restated with the
source's constants named live here too: tests/test_conv_f32_pinned_gpu.py holds the kernels to these, tests/test_conv_f32_pinned_ref.py
checks them on the CPU against torch in float64.  Nothing here reads the kernels or ops.py."""
import collections
import functools
import types
import zlib

import numpy as np

U = 2.0 ** -24                      # half an ulp of 1.0f: the unit of one fp32 rounding
NCHW, NHWC = 0, 1                   # AFAN_NCHW / AFAN_NHWC: activations; for weights KCRS / KRSC memory
F32, BF16 = 0, 1                    # AFAN_F32 / AFAN_BF16
ES = {F32: 4, BF16: 2}
TN = {F32: "f32", BF16: "bf16"}

# ---- constants of csrc/afan_conv_f32.hip ------------------------------------------------------------------------------------------
BK = 16                             # reduction elements (forward / dgrad) or pixels (wgrad) per K-step
BM = 128                            # row tile (pixels) of forward / dgrad
TILE_SMALL, TILE_MID, TILE_BIG = 32, 64, 128       # launch_tile's BN and wgrad_plan's bm: co <= 32 / <= 64 / else
WG_BN = 128                         # column tile (taps x ci) of the weight gradient
WG_TARGET = 1024                    # workgroups wgrad_plan aims at
WG_MIN_STEPS = 8                    # at least 8 K-steps per slice
WG_MAX_SLICES = 256
MAXT = 49

Case = collections.namedtuple("Case", "n hi wi ci co k stride pad dil")

# the issue's rows: the smallest shapes at which each mechanism can still go wrong
CASES = [Case(*c) for c in [
    (2, 5, 7, 3, 16, 3, 1, 1, 1),           # 3-channel stem: both operands scalar, K = 27 (a tail step), one partial row tile, 16 of 32 columns
    (3, 9, 7, 8, 40, 3, 1, 1, 1),           # BN = 64 with 40 columns, two row tiles with the second partial, K = 72
    (2, 6, 6, 20, 136, 1, 1, 0, 1),         # BN = 128 with a second column tile of 8, K = 20
    (1, 9, 11, 4, 33, 7, 2, 3, 1),          # 7x7 stride 2: 49 taps (MAXT), four parity classes of different sizes
    (2, 9, 7, 12, 24, 1, 2, 0, 1),          # 1x1 stride 2 on an odd map: classes without a tap must write zeros
    (2, 8, 6, 8, 8, 3, 2, 1, 2),            # stride 2 with dilation 2: all taps fall into one parity class
    (1, 13, 11, 8, 12, 3, 1, 6, 6),         # atrous reach larger than the map
    (1, 7, 5, 5, 7, 5, 1, 2, 1),            # nothing aligned
    (2, 1, 1, 36, 20, 1, 2, 0, 1),          # 1-pixel map at stride 2: skipped classes
    (4, 1, 1, 64, 10, 1, 1, 0, 1),          # linear layer as a 1x1 convolution
    (1, 4, 4, 4, 8, 3, 1, 64, 64),          # the dilation limit
    (1, 3, 3, 4, 4, 3, 1, 127, 1),          # the padding limit, the `short` tap offsets
    (2, 33, 35, 4, 16, 3, 1, 1, 1),         # weight-gradient plan: P = 2310, 17 slices of 9 steps, the last of 1 step with 6 pixels
    (1, 300, 1, 5, 21, 1, 1, 0, 1),         # the linear layer re-read as a weight gradient: few columns, long reduction
    (2, 128, 128, 3, 16, 3, 1, 1, 1),       # the 256-slice cap: one tile, 2048 steps
    # added to reach a variant: the input gradient's BN = 128 (ci > 64) with the weight rows along the lanes (b_rows = 1)
    (1, 3, 2, 68, 8, 1, 1, 0, 1),
]]
PLAN_ROW = 12
OPS = ("fwd", "dgrad", "wgrad")
KINDS = ("exact", "gauss32", "gauss16")
LAYOUT_PAIRS = [(lay, wl) for lay in (NHWC, NCHW) for wl in (NHWC, NCHW)]
MISALIGNED = (0, 1, 2, 3)           # bit 0: the first operand starts one element late, bit 1: the second; any bit: the output too


def case_id(c):
    return f"{c.n}x{c.hi}x{c.wi}x{c.ci}-co{c.co}-k{c.k}s{c.stride}p{c.pad}d{c.dil}"


def out_dim(i, k, stride, pad, dil):
    return (i + 2 * pad - dil * (k - 1) - 1) // stride + 1


def out_hw(c):
    return out_dim(c.hi, c.k, c.stride, c.pad, c.dil), out_dim(c.wi, c.k, c.stride, c.pad, c.dil)


# ------------------------------------------------------------------------------------------------------------------ references
def _span(n_in, n_out, stride, off):
    """Output indices o in [0, n_out) whose input index o * stride + off lies in [0, n_in): (slice of outputs, slice of inputs, count)."""
    o0 = max(0, -(off // stride))
    o1 = min(n_out - 1, (n_in - 1 - off) // stride)
    if o1 < o0:
        return None
    cnt = o1 - o0 + 1
    i0 = o0 * stride + off
    return slice(o0, o1 + 1), slice(i0, i0 + (cnt - 1) * stride + 1, stride), cnt


def _taps(k, stride, pad, dil, hi, wi, ho, wo):
    for r in range(k):
        for s in range(k):
            a, b = _span(hi, ho, stride, r * dil - pad), _span(wi, wo, stride, s * dil - pad)
            if a is not None and b is not None:
                yield r, s, a, b


def _fwd(x, w, stride, pad, dil):
    n, ci, hi, wi = x.shape
    co, k = w.shape[0], w.shape[2]
    ho, wo = out_dim(hi, k, stride, pad, dil), out_dim(wi, k, stride, pad, dil)
    y, cnt = np.zeros((n, co, ho, wo)), np.zeros((ho, wo))
    for r, s, (oh, ih, _), (ow, iw, _) in _taps(k, stride, pad, dil, hi, wi, ho, wo):
        y[:, :, oh, ow] += np.einsum("nchw,oc->nohw", x[:, :, ih, iw], w[:, :, r, s])
        cnt[oh, ow] += ci
    return y, cnt


def fwd(x, w, b, stride, pad, dil):
    """y = conv2d(x [N,Ci,Hi,Wi], w [Co,Ci,k,k]) + b: (y, S, products per output element [Ho,Wo])."""
    y, cnt = _fwd(x, w, stride, pad, dil)
    s, _ = _fwd(np.abs(x), np.abs(w), stride, pad, dil)
    if b is not None:
        y = y + b[None, :, None, None]
        s = s + np.abs(b)[None, :, None, None]
    return y, s, cnt


def _dgrad(dy, w, in_hw, stride, pad, dil):
    n, co, ho, wo = dy.shape
    ci, k = w.shape[1], w.shape[2]
    hi, wi = in_hw
    dx, cnt = np.zeros((n, ci, hi, wi)), np.zeros((hi, wi))
    for r, s, (oh, ih, _), (ow, iw, _) in _taps(k, stride, pad, dil, hi, wi, ho, wo):
        dx[:, :, ih, iw] += np.einsum("nohw,oc->nchw", dy[:, :, oh, ow], w[:, :, r, s])
        cnt[ih, iw] += co
    return dx, cnt


def dgrad(dy, w, in_hw, stride, pad, dil):
    """dx of y = conv2d(x, w): (dx [N,Ci,Hi,Wi], S, products per input element [Hi,Wi])."""
    dx, cnt = _dgrad(dy, w, in_hw, stride, pad, dil)
    return dx, _dgrad(np.abs(dy), np.abs(w), in_hw, stride, pad, dil)[0], cnt


def _wgrad(x, dy, k, stride, pad, dil):
    n, ci, hi, wi = x.shape
    co, ho, wo = dy.shape[1:]
    dw, cnt = np.zeros((co, ci, k, k)), np.zeros((k, k))
    for r, s, (oh, ih, ch), (ow, iw, cw) in _taps(k, stride, pad, dil, hi, wi, ho, wo):
        dw[:, :, r, s] = np.einsum("nohw,nchw->oc", dy[:, :, oh, ow], x[:, :, ih, iw])
        cnt[r, s] = n * ch * cw
    return dw, cnt


def wgrad(x, dy, k, stride, pad, dil):
    """dw of y = conv2d(x, w): (dw [Co,Ci,k,k], S, pixel products per tap [k,k])."""
    dw, cnt = _wgrad(x, dy, k, stride, pad, dil)
    return dw, _wgrad(np.abs(x), np.abs(dy), k, stride, pad, dil)[0], cnt


# ------------------------------------------------------------------------------------------------------------------ operands
def _bf16_round(a):
    """float64 -> the nearest bf16 value (ties to even), as float64."""
    b = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def _draw(rng, shape, kind):
    if kind == "exact":             # sparse integers in {-2..2}: every product and every partial sum is an integer
        return (rng.randint(-2, 3, size=shape) * (rng.random_sample(shape) < 0.5)).astype(np.float64)
    g = rng.standard_normal(shape).astype(np.float32).astype(np.float64)
    return _bf16_round(g) if kind == "gauss16" else g


@functools.lru_cache(maxsize=None)
def problem(idx, kind):
    """Operands (float64 arrays holding fp32 / bf16 values, logical NCHW / KCRS order) and the three references of row idx.
    exact: sparse integers, integer bias in [-4, 4], integer gradient to accumulate into; gauss32: fp32 Gaussians with a bias;
    gauss16: bf16-representable Gaussians, no bias (both storages hold the same values)."""
    c = CASES[idx]
    rng = np.random.RandomState(zlib.crc32(repr((tuple(c), kind)).encode()) % (1 << 31))
    ho, wo = out_hw(c)
    p = types.SimpleNamespace(case=c, kind=kind)
    p.x, p.w = _draw(rng, (c.n, c.ci, c.hi, c.wi), kind), _draw(rng, (c.co, c.ci, c.k, c.k), kind)
    p.dy = _draw(rng, (c.n, c.co, ho, wo), kind)
    p.b = {"exact": rng.randint(-4, 5, size=c.co).astype(np.float64), "gauss32": _draw(rng, (c.co,), "gauss32"), "gauss16": None}[kind]
    p.g0 = rng.randint(-4, 5, size=(c.co, c.ci, c.k, c.k)).astype(np.float64) if kind == "exact" else _draw(rng, (c.co, c.ci, c.k, c.k), "gauss32")
    geo = (c.stride, c.pad, c.dil)
    p.y, p.y_s, p.y_cnt = fwd(p.x, p.w, p.b, *geo)
    p.dx, p.dx_s, p.dx_cnt = dgrad(p.dy, p.w, (c.hi, c.wi), *geo)
    p.dw, p.dw_s, p.dw_cnt = wgrad(p.x, p.dy, c.k, *geo)
    return p


# ------------------------------------------------------------------------------------------------------------------ dispatch
def tile_of(cols):
    """launch_tile's BN / wgrad_plan's bm: co <= 32 -> 32, co <= 64 -> 64, else 128."""
    return TILE_SMALL if cols <= TILE_SMALL else TILE_MID if cols <= TILE_MID else TILE_BIG


def act_strides(layout, c, h, w):
    """Element strides (sN, sH, sW, sC) of a dense activation tensor."""
    return (h * w * c, w * c, c, 1) if layout == NHWC else (c * h * w, w, 1, h * w)


def vec_ok(misaligned, c, strides):
    """vec_ok of the source: 4-element pieces along the channels: unit channel stride, c % 4 == 0, the base aligned to 4 elements
    and every other stride a multiple of 4."""
    sn, sh, sw, sc = strides
    return sc == 1 and c % 4 == 0 and not misaligned and sn % 4 == 0 and sh % 4 == 0 and sw % 4 == 0


def wgrad_plan(pixels, co, ncols):
    """wgrad_plan of the source: (bm, slices, K-steps per slice)."""
    bm = tile_of(co)
    tiles = -(-co // bm) * -(-ncols // WG_BN)
    steps = -(-pixels // BK)
    s = -(-WG_TARGET // tiles)
    s = min(s, steps // WG_MIN_STEPS)
    s = min(max(s, 1), WG_MAX_SLICES)
    sps = -(-steps // s)
    return bm, -(-steps // sps), sps


def workspace_floats(c):
    ho, wo = out_hw(c)
    return wgrad_plan(c.n * ho * wo, c.co, c.k * c.k * c.ci)[1] * c.co * c.k * c.k * c.ci


def _v(flag):
    return "vec" if flag else "scalar"


def variant_of(case, op, dtype, layout, w_layout, misaligned, accumulate=0):
    """The kernels one call launches and the run-time lane flags of their scalar staging, as labels.  misaligned: bit 0 the first
    operand (x; dy of the input gradient), bit 1 the second (w; dy of the weight gradient) starts one element past a 16-byte
    boundary."""
    c, t = case, TN[dtype]
    ho, wo = out_hw(c)
    m1, m2 = bool(misaligned & 1), bool(misaligned & 2)
    out = set()
    if op == "fwd":
        av = vec_ok(m1, c.ci, act_strides(layout, c.ci, c.hi, c.wi))
        w_sc = 1 if w_layout == NHWC else c.k * c.k                    # KCRS: consecutive ci are k * k apart (1 for a 1x1)
        bv = w_sc == 1 and c.ci % 4 == 0 and not m2                     # bv of afan_conv_fwd
        bn, b_rows = tile_of(c.co), 0
    elif op == "dgrad":
        av = vec_ok(m1, c.co, act_strides(layout, c.co, ho, wo))
        bv = False                                                      # the weight rows (ci) are never the reduction index
        bn, b_rows = tile_of(c.ci), 1
    else:
        av = vec_ok(m2, c.co, act_strides(layout, c.co, ho, wo))         # A = dy
        bv = vec_ok(m1, c.ci, act_strides(layout, c.ci, c.hi, c.wi))     # B = x
        bm = wgrad_plan(c.n * ho * wo, c.co, c.k * c.k * c.ci)[0]
        lanes_k = 1 if layout == NCHW else 0                            # a_k = b_k: lanes along the pixels
        out.add(f"wgrad_f32_kernel<{t},{bm},A {_v(av)},B {_v(bv)}>")
        if not av:
            out.add(f"wgrad_f32_kernel<{t},{bm}>|a_k={lanes_k}")
        if not bv:
            out.add(f"wgrad_f32_kernel<{t}>|b_k={lanes_k}")
        out.add(f"wgrad_f32_reduce_kernel|accumulate={int(accumulate)}")
        return out
    a_rows = 1 if layout == NCHW else 0
    out.add(f"conv_f32_kernel<{t},{bn},A {_v(av)},B {_v(bv)}>")
    if not av:
        out.add(f"conv_f32_kernel<{t}>|a_rows={a_rows}")
    if not bv:
        out.add(f"conv_f32_kernel<{t},{bn}>|b_rows={b_rows}")
    return out


_T, _TILES, _VV = ("f32", "bf16"), (TILE_SMALL, TILE_MID, TILE_BIG), ("vec", "scalar")
EXPECTED_VARIANTS = sorted(
    [f"conv_f32_kernel<{t},{bn},A {a},B {b}>" for t in _T for bn in _TILES for a in _VV for b in _VV] +
    [f"conv_f32_kernel<{t}>|a_rows={f}" for t in _T for f in (0, 1)] +
    [f"conv_f32_kernel<{t},{bn}>|b_rows={f}" for t in _T for bn in _TILES for f in (0, 1)] +
    [f"wgrad_f32_kernel<{t},{bm},A {a},B {b}>" for t in _T for bm in _TILES for a in _VV for b in _VV] +
    [f"wgrad_f32_kernel<{t},{bm}>|a_k={f}" for t in _T for bm in _TILES for f in (0, 1)] +
    [f"wgrad_f32_kernel<{t}>|b_k={f}" for t in _T for f in (0, 1)] +
    ["wgrad_f32_reduce_kernel|accumulate=0", "wgrad_f32_reduce_kernel|accumulate=1"])


def calls(kind):
    """(dtype, layout, w_layout, misaligned) of every call the GPU test makes for one row, operation and operand kind."""
    return [(dt, lay, wl, mis) for dt in ((F32,) if kind == "gauss32" else (F32, BF16)) for lay, wl in LAYOUT_PAIRS for mis in MISALIGNED]


def table_variants():
    got = set()
    for c in CASES:
        for op in OPS:
            for kind in KINDS:
                for dt, lay, wl, mis in calls(kind):
                    for acc in ((0, 1) if op == "wgrad" and kind == "exact" else (0,)):
                        got |= variant_of(c, op, dt, lay, wl, mis, acc)
    return got
