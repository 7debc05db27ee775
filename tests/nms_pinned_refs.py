"""The definition and the case tables for the proposal NMS of csrc/afan_det.hip: nms_mask_kernel<BATCHED>, nms_scan_kernel<BATCHED>,
nms_compact_kernel and rpn_rows_kernel behind afan_nms, afan_nms_top and afan_rpn_proposals (tests/test_nms_pinned_gpu.py holds the
kernels to this module through the C ABI; tests/test_nms_pinned_ref.py checks the module itself on the CPU).  numpy only; nothing here
imports the package.

THE REFERENCE.  Greedy NMS over boxes in score order, every value a single correctly rounded np.float32 operation in the order of the
reference (Detection/support/src/cuda/nms.cu:14-21,49, nms_cpu.cpp:62):
    area  = (x2 - x1 + 1) * (y2 - y1 + 1)
    inter = fmax(fmin(r) - fmax(l) + 1, 0) * fmax(fmin(b) - fmax(t) + 1, 0)          (np.fmax / np.fmin: a quiet NaN yields the other operand)
    u     = (sa + sb) - inter
    v     = inter / u
    struck: v > t (inclusive = 0), v >= t (inclusive = 1)
The library is built with -ffp-contract=off and fp32 division is correctly rounded, so the kernel's decision is this one for EVERY input,
bit for bit: there is no tolerance and no exempted pair in this module or in the two test modules.  Two things are kept out of the
tables, because what the hardware does with them depends on the kernel's float mode and no definition settles it: signalling NaNs (the
only NaN used is 0x7fc00000) and subnormal intermediates.

LISTS live in POSITION space (row i = the box with the i-th best score); `deal` turns a list into what an entry is given, boxes by
original index and the order, under the identity or a permutation without fixed points.  The reference's survivors are positions; a
plain call returns their original indices ascending, a max_keep call the same through the end of the 64-box block in which the bound
is reached (`top_expect`), the proposal layer the rows in score order with zero rows behind (`proposal_expect`).

PLANTED LATTICES have a survivor list known by hand.  Position i owns the cell at ((i % 256) * 100, (i // 256) * 100) and holds the
41 x 41 pixel box [x, y, x + 40, y + 40]: disjoint from every other cell's.  A victim is its striker shifted 4 px in x: IoU
37 * 41 / (2 * 1681 - 1517) = 1517 / 1845 = 0.822.  The box 8 px from the striker has IoU 1353 / 2009 = 0.673 with it and 0.822 with the
victim.  At t = 0.7 the chain A -> B -> C keeps A, strikes B and keeps C: C survives only if the kernel strikes by KEPT rows, B dies only
if the one path from A's block to B's block works.  The survivors of a planted list are "every position but the B's" — stated by the
planner, not computed — and tests/test_nms_pinned_ref.py holds the reference and the C oracle to that statement.

STRUCTURE.  Every block distance the tables use is derived from the scan's constants, parsed from the source: k = column block - row
block is settled by the scanner for k <= SC_D (k = 0 the diagonal recurrence, 1 .. SC_D the transposed band tiles) and by the workers for
k >= FAR = SC_D + 1, who read SC_RC kept rows per trip and 3 x W64 column blocks per stretch (the second stretch starts at distance
FAR + 3 * W64) through a ring of SC_KW keep words, block p on worker p mod SC_NW; the prefetchers fill a ring of SC_R slots.
"""
import collections
import functools
import os
import re

import numpy as np

F = np.float32
I64 = np.int64
OK, EALIGN, ESHAPE, ENULL = 0, -2, -3, -4            # include/afan_hip.h
QNAN = np.array([0x7fc00000], np.uint32).view(F)[0]
T7 = F(0.7)
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cv_a-fan_amd", "csrc", "afan_det.hip")


# ================================================================================================================ the scan's constants
def _constants():
    src = open(SOURCE).read()
    c = {}
    for name in ("W64", "SC_P", "SC_G", "SCAN_WAVES", "SC_KW", "SC_RC", "CP_THREADS", "RPN_MAX_B"):
        c[name] = int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    for name in ("SC_D", "SC_R"):
        assert re.search(rf"constexpr int {name} = AFAN_{name};", src), name
        c[name] = int(re.search(rf"#define AFAN_{name} (\d+)", src).group(1))
    assert "constexpr int SC_NW = SCAN_WAVES - 1 - SC_P;" in src and "const int jf = p + SC_D + 1;" in src
    assert "j0 += 3 * W64" in src and "if (cb - rb <= SC_D)" in src
    return c


K = _constants()
W64, SC_D, SC_R, SC_P, SC_G, SCAN_WAVES, SC_KW, SC_RC, CP_THREADS, RPN_MAX_B = (K[k] for k in (
    "W64", "SC_D", "SC_R", "SC_P", "SC_G", "SCAN_WAVES", "SC_KW", "SC_RC", "CP_THREADS", "RPN_MAX_B"))
SC_NW = SCAN_WAVES - 1 - SC_P
FAR = SC_D + 1
STRETCH = 3 * W64                                    # column blocks a worker covers per stretch
FAR2 = FAR + STRETCH                                 # the first distance of a worker's second stretch
BIG_BLOCKS = FAR2 + 3                                # 208 blocks = 13 312 boxes: the largest list of the tables
assert (W64, SC_NW, FAR, BIG_BLOCKS) == (64, 12, 13, 208) and SC_KW > SC_D + 2 and SC_R >= SC_P * SC_G
MAX_N = 1 << 24                                      # nms_impl's cap
LDS_N = (64 * 1024 // 8) * W64                       # 524 288: the most boxes whose column blocks' words fit the scan's LDS


def workspace_bytes(n):
    cb = (n + W64 - 1) // W64
    return 0 if n <= 0 else n * cb * 8 + ((n + 7) & ~7) + cb * (SC_D + 1) * W64 * 8


def rpn_workspace_bytes(b, n):
    cb = (n + W64 - 1) // W64
    return 0 if b <= 0 or n <= 0 else b * (n * cb * 8 + cb * (SC_D + 1) * W64 * 8 + ((n + 7) & ~7))


# ======================================================================================================================= the reference
def area(b):
    return (b[..., 2] - b[..., 0] + F(1)) * (b[..., 3] - b[..., 1] + F(1))


def pair_terms(a, sa, b, sb):
    """(inter, u, v) of box(es) a against box(es) b, one numpy operation per rounding."""
    with np.errstate(all="ignore"):
        left, right = np.fmax(a[..., 0], b[..., 0]), np.fmin(a[..., 2], b[..., 2])
        top, bottom = np.fmax(a[..., 1], b[..., 1]), np.fmin(a[..., 3], b[..., 3])
        w, h = np.fmax(right - left + F(1), F(0)), np.fmax(bottom - top + F(1), F(0))
        inter = w * h
        u = (sa + sb) - inter
        v = inter / u
    assert inter.dtype == u.dtype == v.dtype == F
    return inter, u, v


def over(v, t, inclusive):
    with np.errstate(invalid="ignore"):
        return (v >= F(t)) if inclusive else (v > F(t))


def greedy(pos_boxes, t, inclusive):
    """kept[i] of the boxes in score order."""
    b = np.ascontiguousarray(pos_boxes, F)
    n = len(b)
    with np.errstate(all="ignore"):
        sa = area(b)
    struck = np.zeros(n, bool)
    for i in range(n - 1):
        if not struck[i]:
            struck[i + 1:] |= over(pair_terms(b[i], sa[i], b[i + 1:], sa[i + 1:])[2], t, inclusive)
    return ~struck


def shortcut(inter, u, t):
    """iou_over's division-free test restated: (decided, hit).  Where decided, hit is the answer in BOTH modes."""
    t = F(t)
    with np.errstate(all="ignore"):
        q = t * u
        sane = bool(t >= F(1e-3) and t <= F(1)) & (u >= F(1)) & (u <= F(1e30))
        hit = sane & (inter > q * F(1.000002))
        miss = sane & (inter < q * F(0.999998))
    return hit | miss, hit, sane


def ulps(a, b):
    """b - a in units of fp32 neighbours (finite, same-sign operands)."""
    return np.asarray(b, F).view(np.int32).astype(np.int64) - np.asarray(a, F).view(np.int32).astype(np.int64)


# ================================================================================================================ lists and their deals
class L:
    """A list in position space.  kept: the hand-stated survivors (bool by position) or None; t / modes: how afan_nms runs it."""

    def __init__(self, name, pos, kept=None, t=T7, modes=(0, 1), perm=False, note=""):
        self.name, self.pos, self.hand, self.t, self.modes, self.perm, self.note = name, np.ascontiguousarray(pos, F), kept, F(t), modes, perm, note
        self.n = len(self.pos)
        self._ref = {}

    def kept(self, inclusive=0, t=None):
        key = (int(inclusive), F(self.t if t is None else t).tobytes())
        if key not in self._ref:
            self._ref[key] = greedy(self.pos, self.t if t is None else t, inclusive)
            self._ref[key].setflags(write=False)
        return self._ref[key]

    def __repr__(self):
        return self.name


def deal(lst, perm=None, extra=0):
    """(boxes by original index [n + extra, 4], order [n + extra]): the identity, or a permutation in which no original index is its
    position.  The `extra` entries behind the list (order longer than pre_n) are copies of the list's first boxes: a kernel that
    looked at them would strike with them."""
    perm = lst.perm if perm is None else perm
    n, a = lst.n, lst.n + extra
    pos = np.concatenate([lst.pos, lst.pos[np.arange(extra) % max(n, 1)]]) if extra else lst.pos
    if not perm or a < 2:
        return pos.copy(), np.arange(a, dtype=I64)
    sigma = np.random.default_rng(1000 + a).permutation(a)
    order = np.empty(a, I64)
    order[sigma] = np.roll(sigma, -1)                                               # one random a-cycle: no fixed point
    assert not (order == np.arange(a)).any()
    boxes = np.empty((a, 4), F)
    boxes[order] = pos
    return boxes, order.astype(I64)


def plain_expect(order, kept):
    """afan_nms: the survivors' original indices, ascending."""
    return np.sort(order[:len(kept)][kept])


def top_expect(kept, max_keep):
    """afan_nms_top: (positions reported, the block the scan stops in): everything through the end of the 64-box block in which the
    kept count reaches max_keep (>=); max_keep of 0 or above 2^31 - 1: unbounded."""
    n = len(kept)
    cb = (n + W64 - 1) // W64
    cum = np.cumsum(kept)
    stop = cb - 1
    if 0 < max_keep <= 0x7fffffff:
        ends = cum[np.minimum(np.arange(1, cb + 1) * W64, n) - 1]
        hit = np.flatnonzero(ends >= max_keep)
        stop = int(hit[0]) if len(hit) else cb - 1
    return np.flatnonzero(kept[:(stop + 1) * W64]), stop


def proposal_expect(boxes, order, kept, top_n):
    """afan_rpn_proposals for one list: (rows [top_n, 4], kept count)."""
    pos = np.flatnonzero(kept)[:top_n]
    rows = np.zeros((top_n, 4), F)
    rows[:len(pos)] = boxes[order[pos]]
    return rows, len(pos)


# ============================================================================================================== the planted lattices
FAR_Y = F(100 * 400)                                  # a row of cells no lattice of the tables reaches


def cell(i):
    i = np.asarray(i)
    x, y = ((i % 256) * 100).astype(F), ((i // 256) * 100).astype(F)
    return np.stack([x, y, x + F(40), y + F(40)], axis=-1)


def shifted(b, px):
    return b + np.array([px, 0, px, 0], F)


class Planner:
    """A lattice of n disjoint boxes into which chains are planted; states the survivors."""

    def __init__(self, n):
        self.n, self.pos, self.used, self.struck, self.plants = n, cell(np.arange(n)), set(), [], []

    def blocks(self):
        return (self.n + W64 - 1) // W64

    def free(self, block, after=-1, lane=None):
        """The first unused position of `block` behind position `after` (from `lane` on), or None."""
        lo = max(block * W64 + (lane or 0), after + 1)
        for p in range(lo, min((block + 1) * W64, self.n)):
            if p not in self.used:
                return p
        return None

    def chain(self, a, d_ab, d_bc=None, lane=None):
        """A at position a (unused), B in the block d_ab behind A's, C (if d_bc is given) d_bc blocks behind B's.  Returns False, and
        plants nothing, where the list is too short."""
        if a in self.used or a >= self.n:
            return False
        b = self.free(a // W64 + d_ab, a, lane)
        if b is None:
            return False
        c = None
        if d_bc is not None:
            self.used.add(b)
            c = self.free(b // W64 + d_bc, b, lane)
            self.used.discard(b)
            if c is None:
                return False
        self.used |= {a, b} | ({c} if c is not None else set())
        self.pos[b] = shifted(self.pos[a], 4)
        if c is not None:
            self.pos[c] = shifted(self.pos[a], 8)
        self.struck.append(b)
        self.plants.append((a, b, c))
        return True

    def kept(self):
        k = np.ones(self.n, bool)
        k[self.struck] = False
        return k

    def done(self, name, **kw):
        lst = L(name, self.pos, self.kept(), **kw)
        lst.plants = list(self.plants)
        return lst


D6 = collections.OrderedDict([("same", 0), ("band1", 1), ("bandD", SC_D), ("far1", FAR), ("farNW", FAR + SC_NW), ("far2nd", FAR2)])
# the block distances of the issue's CPU experiment, by the constants
DISTANCES = (0, 1, SC_D, FAR, FAR + 1, FAR + SC_NW, SC_KW - 1, SC_KW, SC_KW + 1, 100, FAR2, FAR2 + 1)


@functools.lru_cache(maxsize=None)
def chain_lattice(n=BIG_BLOCKS * W64, perm=False):
    """Every (A -> B distance) x (B -> C distance) of D6 that the list's length allows, all A in block 0; then every distance of
    DISTANCES from block 0 with C one block behind B."""
    p = Planner(n)
    planted = []
    lane = 44 if n >= W64 else 0                                    # B's and C's from lane 44 on: the A's before them keep block 0's front
    for (na, dab) in D6.items():
        for (nc, dbc) in D6.items():
            a = p.free(0)
            if a is not None and a < lane and p.chain(a, dab, dbc, lane=lane):
                planted.append((na, nc))
    for d in DISTANCES:
        a = p.free(0)
        if a is not None and a < lane:
            p.chain(a, d, 1, lane=lane)
    lst = p.done(f"chains-n{n}" + ("-perm" if perm else ""), perm=perm)
    lst.pairs = planted
    if perm:
        lst._ref = chain_lattice(n)._ref                            # the same positions: one reference run
    return lst


@functools.lru_cache(maxsize=None)
def block_count_list(cb, last):
    """cb blocks, the last of `last` boxes.  A's in block 0; a B in every block the list has (lane 0 of the last one, which may be its
    only box), a C one block behind wherever that block has room."""
    n = (cb - 1) * W64 + last
    p = Planner(n)
    targets = list(range(1, cb)) if cb <= W64 // 2 else sorted({d for d in DISTANCES if 0 < d < cb} | {cb - 2, cb - 1})
    a = 0
    for d in reversed(targets):                                     # the last block first: its lane 0 belongs to a B
        if p.chain(a, d, 1) or p.chain(a, d):
            a += 1
    if cb == 1 and n >= 3:
        p.chain(0, 0, 0)
    return p.done(f"blocks-cb{cb}-last{last}")


BLOCK_COUNTS = (1, 2, SC_R, SC_R + 1, SC_D, FAR, FAR + 1, SC_KW, SC_KW + 1, BIG_BLOCKS)
LASTS = (W64, 1, W64 - 1)
FAN_D = FAR + 7


@functools.lru_cache(maxsize=None)
def fan(n=(FAN_D + 1) * W64, single=False):
    """All 64 boxes of block 0 kept, each with one victim in block FAN_D: W64 / SC_RC trips of the worker's kept-row loop.  single:
    one victim only, that of the kept row of rank SC_RC — the first row of the second trip."""
    p = Planner(n)
    for lane in ([SC_RC] if single else range(W64)):
        assert p.chain(lane, FAN_D, None, lane=lane)
    assert all(b == FAN_D * W64 + a for a, b, _ in p.plants)
    return p.done(f"fan-n{n}" + ("-rank%d" % SC_RC if single else ""))


@functools.lru_cache(maxsize=None)
def chain_in_block(start):
    """start lattice boxes, then 64 boxes each 4 px from its predecessor: 32 rounds of the diagonal recurrence when start = 0, the same
    chain across a block boundary when start = 32; kept and struck alternate."""
    n = start + W64
    pos = cell(np.arange(n))
    kept = np.ones(n, bool)
    for k in range(W64):
        pos[start + k] = np.array([4 * k, FAR_Y, 4 * k + 40, FAR_Y + 40], F)
        kept[start + k] = k % 2 == 0
    return L(f"chain64-at{start}", pos, kept)


@functools.lru_cache(maxsize=None)
def struck_striker():
    """A in block 0, B FAR + 2 blocks on (struck through a far tile), C a further FAR blocks on: B's row must not strike."""
    p = Planner((2 * FAR + 3) * W64 - 5)
    assert p.chain(3, FAR + 2, FAR, lane=17)
    return p.done("struck-striker-far-far")


@functools.lru_cache(maxsize=None)
def identical(n):
    kept = np.zeros(n, bool)
    kept[0] = True
    return L(f"identical-n{n}", np.tile(cell(5), (n, 1)), kept)


@functools.lru_cache(maxsize=None)
def disjoint(n):
    return L(f"disjoint-n{n}", cell(np.arange(n)), np.ones(n, bool))


DISJOINT_N = (1, 63, 64, 65, CP_THREADS - 1, CP_THREADS, CP_THREADS + 1, 2 * CP_THREADS + 1)
NAN_SLOTS = ((0,), (1,), (2,), (3,), (0, 1, 2, 3))


def nan_box(b, slots):
    b = np.array(b, F)
    b[list(slots)] = QNAN
    return b


@functools.lru_cache(maxsize=None)
def nan_lattice(n=3 * W64):
    """A 3-block lattice with chains across it and NaN boxes at lanes 0, 31 and 63 of block 1: each is kept (its area is NaN: never
    struck) and strikes nothing — the neighbours of each, planted 4 px from where it would be, stay."""
    p = Planner(n)
    kept_extra = []
    for k, lane in enumerate((0, 31, 63)):
        q = W64 + lane
        p.used.add(q)
        p.pos[q] = nan_box(p.pos[q], NAN_SLOTS[(k + 1) * 2 % 5])
        v = p.free(2, lane=lane)                                     # would be its victim were the NaN a number
        p.used.add(v)
        p.pos[v] = shifted(cell(q), 4)
        kept_extra.append(v)
    assert p.chain(1, 1, 1) and p.chain(2, 2) and p.chain(5, 0, 2)
    lst = p.done(f"nan-lattice-n{n}")
    lst.nan_at = [W64, W64 + 31, W64 + 63]
    return lst


# ================================================================================================================= the mixed tables
@functools.lru_cache(maxsize=None)
def integer_set():
    """The 700 integer boxes of tests/test_det_gpu.py::test_nms_thresholds_on_exact_ties, in score order."""
    rng = np.random.default_rng(5)
    n = 700
    xy = rng.integers(0, 24, (n, 2)).astype(F)
    wh = rng.integers(0, 12, (n, 2)).astype(F)
    boxes = np.concatenate([xy, xy + wh], axis=1)
    scores = rng.permutation(n).astype(F) / n
    return np.ascontiguousarray(boxes[np.argsort(-scores, kind="stable")])


TIE_Q = (F(1) / F(2), F(1) / F(4), F(1) / F(3), F(2) / F(3), F(3) / F(4))
TIE_T = tuple(np.nextafter(q, F(s)) for q in TIE_Q for s in (2, -2))


@functools.lru_cache(maxsize=None)
def clustered(kind, n=2000):
    """n boxes around n / 10 centres, so that about a tenth survive at t = 0.5: quarter-pixel coordinates, or arbitrary floats."""
    rng = np.random.default_rng({"quarter": 71, "float": 72}[kind])
    m = n // 10
    centre = rng.uniform(0, 3000, (m, 2))
    size = rng.uniform(30, 120, (m, 2))
    who = rng.integers(0, m, n)
    c = centre[who] + rng.normal(0, 2.5, (n, 2))
    s = size[who] * np.exp(rng.normal(0, 0.06, (n, 2)))
    b = np.concatenate([c - s / 2, c + s / 2], axis=1)
    if kind == "quarter":
        b = np.round(b * 4) / 4
    return L(f"clustered-{kind}-n{n}", b.astype(F), None, t=F(0.5))


@functools.lru_cache(maxsize=None)
def mixed_lists():
    ints = integer_set()
    out = [L(f"int700-t{float(t)!r}", ints, None, t=t) for t in TIE_T]
    out += [clustered("quarter"), clustered("float"), L("clustered-float-n2000-t0.7", clustered("float").pos, None, t=T7)]
    return tuple(out)


# ================================================================================================================== every list table
@functools.lru_cache(maxsize=None)
def list_cases():
    """Every list afan_nms is run on.  The 208-block lists run in mode 0 only (their reference takes most of a second each)."""
    out = [chain_lattice(), chain_lattice(perm=True), chain_lattice((2 * FAR + 3) * W64 - 27), chain_lattice((2 * FAR + 3) * W64 - 27, True)]
    out += [block_count_list(cb, last) for cb in BLOCK_COUNTS for last in LASTS]
    out += [fan(), fan(single=True), chain_in_block(0), chain_in_block(W64 // 2), struck_striker(), identical(FAR * W64 + 5), nan_lattice()]
    out += [disjoint(n) for n in DISJOINT_N]
    out += list(mixed_lists())
    for lst in out:
        if lst.n > 4096:
            lst.modes = (0,)
    names = [lst.name for lst in out]
    assert len(set(names)) == len(names)
    return tuple(out)


# ============================================================================================================ the pair-decision table
Pair = collections.namedtuple("Pair", "kind a b t")             # a: the better-scored box.  Run with inclusive both ways.


def _fractions(qmax=12):
    return [(p, q) for q in range(1, qmax + 1) for p in range(1, q + 1) if np.gcd(p, q) == 1]


def _three(t):
    t = F(t)
    return (t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf)))


def _search(rng, t, rel, want, tries=40):
    """Pairs of arbitrary-float boxes whose quotient v sits at t * (1 + rel): b's right edge is bisected over its fp32 neighbours (at
    most 32 halvings) between "barely overlapping" and "a's own right edge".  Returns (a [m, 4], b [m, 4], their 17 neighbours)."""
    A, Bs = [], []
    target = F(np.float64(t) * (1.0 + rel))
    for _ in range(tries):
        m = 4 * want
        a1 = rng.uniform(0, 900, (m, 2))
        aw = rng.uniform(20, 300, (m, 2))
        a = np.concatenate([a1, a1 + aw], axis=1).astype(F)
        b = a.copy()
        b[:, 0] += (rng.uniform(0, 0.2, m) * aw[:, 0]).astype(F)
        b[:, 1] += (rng.normal(0, 0.08, m) * aw[:, 1]).astype(F)
        b[:, 3] += (rng.normal(0, 0.08, m) * aw[:, 1]).astype(F)
        sa = area(a)

        def v_at(x2):
            bb = b.copy()
            bb[:, 2] = x2
            return pair_terms(a, sa, bb, area(bb))[2]

        lo, hi = b[:, 0].copy(), a[:, 2].copy()
        ok = (lo > 0) & (hi > lo) & (v_at(lo) < target) & (v_at(hi) > target)
        lo_i, hi_i = lo.view(np.int32).astype(np.int64), hi.view(np.int32).astype(np.int64)
        for _ in range(32):
            mid = ((lo_i + hi_i) // 2).astype(np.int32).view(F)
            up = v_at(mid) >= target
            hi_i = np.where(up, mid.view(np.int32), hi_i)
            lo_i = np.where(up, lo_i, mid.view(np.int32))
        for k in range(-8, 9):
            bb = b.copy()
            bb[:, 2] = (hi_i + k).astype(np.int32).view(F)
            A.append(a[ok])
            Bs.append(bb[ok])
        if sum(len(x) for x in A) >= 17 * want:
            break
    return np.concatenate(A), np.concatenate(Bs)


NONINT_T = (F(0.3), F(0.5), F(0.7))
NONINT_PER = 700                                     # per threshold and per kind: 3 x 700 near pairs, 3 x 700 at the three distances


@functools.lru_cache(maxsize=None)
def nonint_pairs():
    rng = np.random.default_rng(20240)
    out = []
    for t in NONINT_T:
        a, b = _search(rng, t, 0.0, NONINT_PER)
        v = pair_terms(a, area(a), b, area(b))[2]
        near = np.flatnonzero(np.abs(ulps(F(t), v)) <= 4)
        near = near[rng.permutation(len(near))[:NONINT_PER]]
        assert len(near) == NONINT_PER, len(near)
        out += [Pair("near", a[i], b[i], t) for i in near]
        for rel in (1e-6, 3e-6, 1e-5):
            for sign in (1, -1):
                a, b = _search(rng, t, sign * rel, NONINT_PER // 6 + 1)
                v = pair_terms(a, area(a), b, area(b))[2].astype(np.float64)
                d = np.abs(v / np.float64(t) - 1.0)
                good = np.flatnonzero((d > rel * 0.8) & (d < rel * 1.25))
                good = good[rng.permutation(len(good))[:NONINT_PER // 6 + 1]]
                assert len(good) == NONINT_PER // 6 + 1, (float(t), rel, sign, len(good))
                out += [Pair(f"rel{rel:g}", a[i], b[i], t) for i in good]
    return tuple(out)


INSANE_T = (F(0), F(-0.0), F(1e-4), np.nextafter(F(1e-3), F(0)), F(1e-3), F(1), np.nextafter(F(1), F(2)), F(2), F(-1), F(np.inf), QNAN)


@functools.lru_cache(maxsize=None)
def pair_table():
    b = lambda *v: np.array(v, F)
    out = []
    # quotient ties: a = q x h pixels, b = its first p columns: inter = p h, u = q h, IoU exactly p / q
    for k, (p, q) in enumerate(_fractions()):
        h = (1, 3, 7)[k % 3]
        for t in _three(F(p) / F(q)):
            out.append(Pair(f"tie{p}/{q}", b(0, 0, q - 1, h - 1), b(0, 0, p - 1, h - 1), t))
    out += [Pair("identical", b(3, 4, 20, 30), b(3, 4, 20, 30), t) for t in (F(1), np.nextafter(F(1), F(0)))]
    # thresholds outside [1e-3, 1] (the wave always divides) and on its edges
    for t in INSANE_T:
        out += [Pair("t-overlap", b(0, 0, 9, 9), b(0, 0, 9, 19), t), Pair("t-disjoint", b(0, 0, 9, 9), b(50, 50, 59, 59), t),
                Pair("t-identical", b(0, 0, 9, 9), b(0, 0, 9, 9), t)]
    # unions either side of 1e30f (the `sane` term), t on and beside the quotient; areas that overflow
    for hgt in (F(9.99e14), F(1.001e15)):
        pa, pb = b(0, 0, 1e15, hgt), b(0, 0, 1e15, hgt / F(2))
        v = pair_terms(pa, area(pa), pb, area(pb))[2]
        out += [Pair("u-1e30", pa, pb, t) for t in _three(v)]
    out += [Pair("overflow", b(0, 0, 1e20, 1e20), b(0, 0, 1e20, 1e20), t) for t in (F(0.5), F(0))]
    out += [Pair("overflow-one", b(0, 0, 1e20, 1e20), b(0, 0, 10, 10), t) for t in (F(0.5), F(0))]
    out += [Pair("overflow-one", b(0, 0, 10, 10), b(0, 0, 1e20, 1e20), F(0.5))]
    # negative coordinates
    out += [Pair("negative", b(-50, -30, -10, -5), b(-40, -20, 0, 5), t) for t in (F(0.3), F(0.5))]
    out += [Pair("negative", b(-9, -9, 0, 0), b(-9, -9, 0, 10), t) for t in _three(F(100) / F(200))]
    # degenerate extents
    deg = {"zero": b(5, 5, 5, 9), "area0": b(5, 5, 4, 9), "neg1": b(5, 5, 2, 9), "neg2": b(5, 5, 2, 2)}
    for name, d in deg.items():
        for t in (F(0.5), F(0), F(1e-3)):
            out += [Pair(name + "-self", d, d, t), Pair(name + "-first", d, b(3, 3, 8, 9), t), Pair(name + "-second", b(3, 3, 8, 9), d, t)]
    # NaN coordinates: one slot, all four; the NaN box first and second
    for slots in NAN_SLOTS:
        nb = nan_box(b(0, 0, 9, 9), slots)
        for t in (F(0.5), F(0)):
            out += [Pair("nan-first", nb, b(0, 0, 9, 10), t), Pair("nan-second", b(0, 0, 9, 10), nb, t), Pair("nan-both", nb, nb, t)]
    return tuple(out) + nonint_pairs()


def pair_decisions(pairs, inclusive):
    """struck[k]: the second box of pair k is struck."""
    a, bb = np.stack([p.a for p in pairs]), np.stack([p.b for p in pairs])
    t = np.array([p.t for p in pairs], F)
    with np.errstate(all="ignore"):
        v = pair_terms(a, area(a), bb, area(bb))[2]
        return (v >= t) if inclusive else (v > t)


def pairs_by_threshold(pairs, per=RPN_MAX_B):
    """[(t, [indices])]: the pairs that share a threshold's bits, at most `per` to a group (afan_rpn_proposals: one list per pair)."""
    groups = collections.OrderedDict()
    for k, p in enumerate(pairs):
        groups.setdefault(F(p.t).tobytes(), []).append(k)
    return [(pairs[idx[0]].t, idx[i:i + per]) for idx in groups.values() for i in range(0, len(idx), per)]


# =========================================================================================================== afan_nms_top's arguments
def top_cases(lst):
    """max_keep values for a list in score order: 1, the kept count at the end of two blocks exactly, one more, one less, beyond the
    total, and 2^31 (unbounded)."""
    kept = lst.kept(0)
    cum = np.cumsum(kept)
    cb = (lst.n + W64 - 1) // W64
    out = [1]
    for blk in sorted({0, min(FAR, cb - 2)}):
        e = int(cum[(blk + 1) * W64 - 1])
        out += [e, e + 1, e - 1]
    out += [int(cum[-1]) + 5, 1 << 31]
    return [m for m in dict.fromkeys(out) if m > 0]


# ======================================================================================================= afan_rpn_proposals' batches
@functools.lru_cache(maxsize=None)
def batch_lists(n):
    """Five different lists of one length: a chain lattice, the fan, the all-identical list, an all-disjoint one, a lattice with NaN
    boxes."""
    return (chain_lattice(n), fan(n), identical(n), disjoint(n), nan_lattice(n))


RPN_N = (2 * FAR + 3) * W64 - 27                     # 1 829 boxes: 29 blocks, a ragged last one


def rpn_top_ns(lists):
    """top_n below, equal to and above the survivors of the batch's first list, cutting inside a block, and 0."""
    s = int(lists[0].kept(0).sum())
    return (s - 3, s, s + 9, W64 + 7, 0)
