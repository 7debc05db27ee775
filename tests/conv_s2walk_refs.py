"""The stride-2 pair-form input gradient (afan_conv_dgrad_sc_nhwc_bf16, plain form) restated on the CPU, and the operand cases of
test_conv_s2walk_gpu.py.

  dx[n, 2h'+ph, 2w'+pw, :] = sum over the class's taps (a, b) of dy[n, h'+(ph+1-a)/2, w'+(pw+1-b)/2, :] * wt10[:, a*3+b, :]
                             (+ dy_sc[n, h', w', :] * wt10[:, 9, :] in class (0, 0); dy pixels outside the image are zero)

`restate` forms every (tap slot, 64-channel chunk) partial product exactly in float64 and then adds the partials of one dx element in
a GIVEN order: in float64 (the definition), or in float32 with one rounding per addition and a final rounding to bf16 (what a kernel
that keeps one fp32 accumulator per element does, at the granularity at which the two routes could differ: which tap and which chunk
comes next).  Tensors are channels-last: dy, dy_sc [n, hi/2, wi/2, co], wt10 [ci, 10, co], dx [n, hi, wi, ci]; hi, wi even.
"""
import torch

BF16 = torch.bfloat16


def slot_class(s):
    """tap slot -> (ph, pw, dh, dw): the output-parity class it feeds and the dy shift it reads at (slot 9: the projection)."""
    if s == 9:
        return 0, 0, 0, 0
    a, b = divmod(s, 3)
    ph, pw = (a + 1) & 1, (b + 1) & 1
    return ph, pw, (ph + 1 - a) // 2, (pw + 1 - b) // 2


def class_slots(ph, pw):
    return [s for s in range(10) if slot_class(s)[:2] == (ph, pw)]


def kernel_order(ph, pw, chunks):
    """the tiled kernels' K order: chunk-outer, tap-inner (slots ascending, the projection last in class (0, 0))"""
    return [(s, q) for q in range(chunks) for s in class_slots(ph, pw)]


def tap_outer_order(ph, pw, chunks):
    return [(s, q) for s in class_slots(ph, pw) for q in range(chunks)]


def reversed_order(ph, pw, chunks):
    return kernel_order(ph, pw, chunks)[::-1]


def restate(dy, dy_sc, wt10, order=kernel_order, fp32=False):
    n, hg, wg, co = dy.shape
    ci = wt10.shape[0]
    assert co % 64 == 0 and wt10.shape == (ci, 10, co) and dy_sc.shape == dy.shape
    chunks = co // 64
    dyp = torch.zeros(n, hg + 1, wg + 1, co, dtype=torch.float64)
    dyp[:, :hg, :wg] = dy.double()
    scd, w = dy_sc.double(), wt10.double()
    dx = torch.zeros(n, 2 * hg, 2 * wg, ci, dtype=torch.float32 if fp32 else torch.float64)
    for ph in range(2):
        for pw in range(2):
            acc = torch.zeros(n, hg, wg, ci, dtype=torch.float32 if fp32 else torch.float64)
            for s, q in order(ph, pw, chunks):
                _, _, dh, dw = slot_class(s)
                src = scd if s == 9 else dyp[:, dh:dh + hg, dw:dw + wg]
                part = torch.einsum("nyxc,ic->nyxi", src[..., q * 64:(q + 1) * 64], w[:, s, q * 64:(q + 1) * 64])
                acc = (acc.double() + part).float() if fp32 else acc + part
            dx[:, ph::2, pw::2] = acc
    return dx.to(BF16) if fp32 else dx


# ---- operands -----------------------------------------------------------------------------------------------------------------
def _rand(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def order_visible(n, hg, wg, ci, g):
    """co = 128.  Magnitudes alternate 2^8 / 2^-8 across taps and chunks: a dy pixel (y, x) is large in chunk q iff y + x + q is even
    (dy_sc: odd), so the taps of a class, which read pixels one step apart, alternate, and so do the two chunks of one tap.  Large
    pixels all carry one channel pattern, and the weights are paired (slot 8 = -slot 0, 6 = -2; slots 5 / 7 / 9 = minus slots 3 / 1 / 4
    with the chunks exchanged) so that the large partials of an interior element cancel exactly: what is left is the small partials,
    whose low bits an fp32 accumulator keeps or drops depending on whether a large partial was in it when they arrived."""
    co = 128
    u = (1.0 + torch.randint(0, 128, (64,), generator=g).double() / 128.0).repeat(2)       # bf16 mantissas
    y, x, q = torch.arange(hg).view(1, hg, 1, 1), torch.arange(wg).view(1, 1, wg, 1), (torch.arange(co) // 64).view(1, 1, 1, co)
    big = ((y + x + q) % 2 == 0).expand(n, hg, wg, co)
    small = torch.randn(n, hg, wg, co, generator=g).double() * 2.0 ** -8
    dy = torch.where(big, (u * 2.0 ** 8).expand(n, hg, wg, co), small).to(BF16)
    small = torch.randn(n, hg, wg, co, generator=g).double() * 2.0 ** -8
    dy_sc = torch.where(~big, (u * 2.0 ** 8).expand(n, hg, wg, co), small).to(BF16)
    w = _rand((ci, 10, co), g, 0.25)
    swap = torch.cat([torch.arange(64, 128), torch.arange(0, 64)])
    w[:, 8], w[:, 6] = -w[:, 0], -w[:, 2]
    w[:, 5], w[:, 7], w[:, 9] = -w[:, 3][:, swap], -w[:, 1][:, swap], -w[:, 4][:, swap]
    return dy, dy_sc, w.contiguous()


def operand_cases(n, hi, wi, ci, co, seed):
    """(name, dy, dy_sc, wt10) on the CPU, one by one"""
    hg, wg = hi // 2, wi // 2
    g = torch.Generator().manual_seed(seed)
    dy, sc, w = _rand((n, hg, wg, co), g), _rand((n, hg, wg, co), g), _rand((ci, 10, co), g, 0.125)
    yield "random", dy, sc, w
    for s in range(10):                                   # the tap-to-shift table, one slot at a time
        w1 = torch.zeros_like(w)
        w1[:, s] = w[:, s]
        yield f"slot{s}", dy, sc, w1
    w1 = w.clone()
    w1[:, :9] = 0
    yield "projection-only", dy, sc, w1
    w1 = w.clone()
    w1[:, 9] = 0
    yield "3x3-only", dy, sc, w1
    pixels = [(0, 0, 0), (0, 0, wg - 1), (n - 1, hg - 1, 0), (n - 1, hg - 1, wg - 1), (n // 2, hg // 2, wg // 2)]
    for k, (i, y, x) in enumerate(dict.fromkeys(pixels)):  # border validity; nothing leaks across images
        hot = torch.zeros_like(dy)
        hot[i, y, x] = dy[i, y, x]
        yield f"dy-onehot{k}", hot, torch.zeros_like(sc), w
        yield f"sc-onehot{k}", torch.zeros_like(dy), hot, w
    if co == 128:
        yield ("order-visible",) + order_visible(n, hg, wg, ci, g)
