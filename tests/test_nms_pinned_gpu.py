"""The proposal NMS of csrc/afan_det.hip — nms_mask_kernel<BATCHED>, nms_scan_kernel<BATCHED>, nms_compact_kernel, rpn_rows_kernel —
called through the C ABI (afan_nms, afan_nms_top, afan_rpn_proposals) and held BIT FOR BIT to the definition of
tests/nms_pinned_refs.py (numpy, np.float32, one operation per rounding; tests/test_nms_pinned_ref.py checks it on the CPU against the C
oracle, the reference's golden list and the hand-stated survivors of every planted list).  No comparison here has a tolerance and no
pair is exempt: survivors, counts, rows and flags are compared as integers and bit patterns.

Conventions (those of tests/test_update_pinned_gpu.py, whose Buf this module uses): every buffer is its own allocation with a 256-byte
guard band on both sides, pre-filled with the byte 0xA5, guard bands checked after every call; inputs are checked unwritten; keep_out
behind count_out[0] still holds the fill; count_out is exactly 8 bytes; the workspace is exactly afan_nms_workspace_bytes(n) /
afan_rpn_proposals_workspace_bytes(b, n).  EVERY case runs twice, over a workspace filled with 0xFF and with 0x00: a mask or band word
that is read without having been written strikes everything under one fill and nothing under the other, and both runs must equal the
reference.  The 2-box lists of the pair table run back to back into slots of shared allocations (each slot its own 256 bytes of guard)
and are read back once; afan_rpn_proposals runs them again, 64 pairs to a call, under the BATCHED templates.  padded lies in front of
as many bytes of slack as the list has candidates, so a row written past top_n lands in the test's own memory and is seen.  Each case
prints "NMSPIN <entry> <case>" (run with -s).

On an MI355X every case passes with the kernels as they were: no fix was needed.  The module's cases and time are in DESIGN.md section 5.
"""
import ctypes

import numpy as np
import pytest
import torch

import nms_pinned_refs as R
from test_update_pinned_gpu import GUARD, Buf, P, SENT, _st

pytestmark = pytest.mark.gpu

F, I64 = R.F, R.I64
FILLS = (0xFF, 0x00)


class Report:
    def __init__(self, entry, case):
        self.what, self.fails, self.bufs, self.inputs = f"{entry} {case}", [], [], []
        print(f"NMSPIN {entry} {case}")

    def buf(self, dev, nbytes, init=None, fill=None):
        b = Buf(dev, int(nbytes), 0, init)
        if fill is not None and nbytes:
            b.raw[b.lo:b.lo + b.n].fill_(fill)
        self.bufs.append(b)
        return b

    def inp(self, dev, a):
        a = np.ascontiguousarray(a)
        b = self.buf(dev, a.nbytes, a)
        self.inputs.append((b, a.copy()))
        return b

    def expect(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def rc(self, got, want=R.OK):
        self.expect(got == want, f"returned {got}, expected {want}")

    def same(self, name, got, want):
        """Integers, or fp32 rows as bit patterns."""
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.dtype == F:
            got, want = got.view(np.uint32), want.astype(F).view(np.uint32)
        if got.shape != want.shape:
            return self.expect(False, f"{name}: {got.shape} values, expected {want.shape}")
        bad = np.flatnonzero(got.ravel() != want.ravel())
        if len(bad):
            self.expect(False, f"{name}: {len(bad)} of {want.size} differ, first at {bad[0]}: got {got.ravel()[bad[0]]}, expected {want.ravel()[bad[0]]}")

    def fill(self, name, raw):
        self.expect(bool((np.ascontiguousarray(raw).view(np.uint8) == SENT).all()), f"{name}: written where the entry must leave the buffer alone")

    def done(self):
        for k, (b, a) in enumerate(self.inputs):
            self.expect(np.array_equal(b.get(np.uint8), a.reshape(-1).view(np.uint8)), f"input {k} was written")
        for k, b in enumerate(self.bufs):
            self.expect(b.guards_ok(), f"the guard band of buffer {k} was written")
        assert not self.fails, f"{self.what}:\n  " + "\n  ".join(self.fails[:12])


def cf(t):
    return ctypes.c_float(float(t))


def run_nms(rep, lib, dev, bb, bo, n, t, inclusive, fill, max_keep=None):
    """One call over a fresh workspace of exactly the stated size, keep_out and count_out.  -> (keep [n] int64 raw, count, workspace)."""
    nbytes = lib.afan_nms_workspace_bytes(n)
    rep.expect(nbytes == R.workspace_bytes(n), f"afan_nms_workspace_bytes({n}) = {nbytes}")
    ws, bk, bc = rep.buf(dev, nbytes, fill=fill), rep.buf(dev, 8 * n), rep.buf(dev, 8)
    if max_keep is None:
        rep.rc(lib.afan_nms(P(bb), P(bo), n, cf(t), inclusive, P(ws), P(bk), P(bc), _st()))
    else:
        rep.rc(lib.afan_nms_top(P(bb), P(bo), n, cf(t), inclusive, P(ws), P(bk), P(bc), max_keep, _st()))
    return bk.get(I64), int(bc.get(I64)[0]), ws


def check_keep(rep, tag, keep, count, want):
    rep.expect(count == len(want), f"{tag}: count {count}, expected {len(want)}")
    if count == len(want):
        rep.same(f"{tag}: survivors", keep[:count], want)
        rep.fill(f"{tag}: keep_out behind the count", keep[count:])


# ============================================================================================================================ afan_nms
@pytest.mark.parametrize("lst", R.list_cases(), ids=repr)
def test_nms_lists_pinned(pkg, gpu, lst):
    lib, rep = pkg._lib.load(), Report("afan_nms", repr(lst))
    boxes, order = R.deal(lst)
    bb, bo = rep.inp(gpu, boxes), rep.inp(gpu, order)
    for inclusive in lst.modes:
        want = R.plain_expect(order, lst.kept(inclusive))
        for fill in FILLS:
            keep, count, _ = run_nms(rep, lib, gpu, bb, bo, lst.n, lst.t, inclusive, fill)
            check_keep(rep, f"inclusive {inclusive} fill {fill:#04x}", keep, count, want)
    rep.done()


class Slots:
    """count slots of nbytes each in one allocation, 256 bytes of 0xA5 in front of the first and (at least) behind every one."""

    def __init__(self, dev, count, nbytes, fill=None, init=None):
        self.count, self.nbytes = count, nbytes
        self.stride = (nbytes + GUARD + 255) // 256 * 256
        self.raw = torch.full((GUARD + count * self.stride,), SENT, dtype=torch.uint8, device=dev)
        body = self.raw[GUARD:].view(count, self.stride)
        if fill is not None:
            body[:, :nbytes] = fill
        if init is not None:
            body[:, :nbytes] = torch.from_numpy(np.ascontiguousarray(init).reshape(count, -1).view(np.uint8)).to(dev)
        self.base = self.raw.data_ptr() + GUARD

    def p(self, k):
        return ctypes.c_void_p(self.base + k * self.stride)

    def read(self):
        """(data [count, nbytes] uint8, every guard byte intact)."""
        h = self.raw.cpu().numpy()
        body = h[GUARD:].reshape(self.count, self.stride)
        return np.ascontiguousarray(body[:, :self.nbytes]), bool((h[:GUARD] == SENT).all() and (body[:, self.nbytes:] == SENT).all())


def pair_arrays(pairs):
    """boxes by original index [m, 2, 4] and orders [m, 2]: every second pair swapped, so that its original index is not its position."""
    boxes = np.stack([np.stack([p.a, p.b]) for p in pairs]).astype(F)
    order = np.tile(np.arange(2, dtype=I64), (len(pairs), 1))
    boxes[1::2], order[1::2] = boxes[1::2, ::-1].copy(), order[1::2, ::-1].copy()
    return boxes, order


@pytest.mark.parametrize("inclusive", (0, 1))
def test_nms_pair_table_pinned(pkg, gpu, inclusive):
    lib, rep = pkg._lib.load(), Report("afan_nms", f"pair-table-inclusive{inclusive}")
    pairs = R.pair_table()
    m = len(pairs)
    struck = R.pair_decisions(pairs, inclusive)
    boxes, order = pair_arrays(pairs)
    nws = lib.afan_nms_workspace_bytes(2)
    rep.expect(nws == R.workspace_bytes(2), "workspace bytes")
    sb, so = Slots(gpu, m, 32, init=boxes), Slots(gpu, m, 16, init=order)
    for fill in FILLS:
        ws, sk, sc = Slots(gpu, m, nws, fill=fill), Slots(gpu, m, 16), Slots(gpu, m, 8)
        st = _st()
        for k, p in enumerate(pairs):
            rc = lib.afan_nms(sb.p(k), so.p(k), 2, cf(p.t), inclusive, ws.p(k), sk.p(k), sc.p(k), st)
            if rc != R.OK:
                rep.rc(rc)
        keep, ok_k = sk.read()
        count, ok_c = sc.read()
        rep.expect(ok_k and ok_c and ws.read()[1], f"fill {fill:#04x}: a guard band of keep_out, count_out or the workspace was written")
        keep, count = keep.view(I64), count.view(I64)[:, 0]
        rep.same(f"fill {fill:#04x}: counts", count, 2 - struck.astype(I64))
        want = np.where(struck[:, None], np.stack([order[:, 0], np.full(m, int(np.array([SENT] * 8, np.uint8).view(I64)[0]))], axis=1),
                        np.tile(np.arange(2, dtype=I64), (m, 1)))
        bad = np.flatnonzero((keep != want).any(axis=1))
        rep.expect(not len(bad), f"fill {fill:#04x}: {len(bad)} pairs differ, first {pairs[bad[0]] if len(bad) else None}: "
                                 f"keep_out {keep[bad[0]].tolist() if len(bad) else None}")
    for s, a in ((sb, boxes), (so, order)):
        data, ok = s.read()
        rep.expect(ok and np.array_equal(data, a.reshape(m, -1).view(np.uint8)), "an input was written")
    rep.done()


# ======================================================================================================================== afan_nms_top
TOP_LISTS = (R.chain_lattice(), R.chain_lattice(R.RPN_N), R.clustered("quarter"), R.clustered("float"))


@pytest.mark.parametrize("lst", TOP_LISTS, ids=repr)
def test_nms_top_pinned(pkg, gpu, lst):
    """Boxes in score order (the identity order: a flag's index is its position)."""
    lib, rep = pkg._lib.load(), Report("afan_nms_top", repr(lst))
    n, cb = lst.n, (lst.n + R.W64 - 1) // R.W64
    order = np.arange(n, dtype=I64)
    bb, bo = rep.inp(gpu, lst.pos), rep.inp(gpu, order)
    kept = lst.kept(0)
    total = int(kept.sum())
    for max_keep in R.top_cases(lst):
        want, stop = R.top_expect(kept, max_keep)
        for fill in FILLS:
            tag = f"max_keep {max_keep} fill {fill:#04x}"
            keep, count, ws = run_nms(rep, lib, gpu, bb, bo, n, lst.t, 0, fill, max_keep)
            check_keep(rep, tag, keep, count, want)
            first = min(max_keep, total)
            rep.same(f"{tag}: the first survivors", keep[:first], np.flatnonzero(kept)[:first])
            flags = ws.get(np.uint8)[n * cb * 8:n * cb * 8 + n]
            rep.same(f"{tag}: flags through block {stop}", flags[:(stop + 1) * R.W64] != 0, kept[:(stop + 1) * R.W64])
            rep.expect(not flags[(stop + 1) * R.W64:].any(), f"{tag}: a flag behind block {stop} is set")
    stops = {R.top_expect(kept, m)[1] for m in R.top_cases(lst)}
    rep.expect(len(stops) >= 4 and cb - 1 in stops and 0 in stops, f"the table itself: stop blocks {sorted(stops)}")
    rep.done()


# ================================================================================================================== afan_rpn_proposals
def run_rpn(rep, lib, dev, bb, bo, B, a, pre_n, t, top_n, fill, slack):
    """-> (padded [B, top_n, 4] fp32, kept [B])"""
    n = min(a, pre_n)
    nbytes = lib.afan_rpn_proposals_workspace_bytes(B, n)
    rep.expect(nbytes == R.rpn_workspace_bytes(B, n), f"afan_rpn_proposals_workspace_bytes({B}, {n}) = {nbytes}")
    ws, bk = rep.buf(dev, nbytes, fill=fill), rep.buf(dev, 8 * B)
    bp = rep.buf(dev, 16 * B * top_n + slack) if top_n else None
    rep.rc(lib.afan_rpn_proposals(P(bb), P(bo), B, a, pre_n, cf(t), top_n, P(ws), P(bp), P(bk), _st()))
    if not top_n:
        return np.zeros((B, 0, 4), F), bk.get(I64)
    raw = bp.get(np.uint8)
    rep.fill("the slack behind padded", raw[16 * B * top_n:])
    return raw[:16 * B * top_n].view(F).reshape(B, top_n, 4), bk.get(I64)


@pytest.mark.parametrize("shape", ("a>pre_n", "a<pre_n", "a==pre_n"))
@pytest.mark.parametrize("B", (1, 3, R.RPN_MAX_B))
def test_rpn_proposals_batches_pinned(pkg, gpu, B, shape):
    """A batch of different lists, every second one under a permutation of its original indices."""
    lib, rep = pkg._lib.load(), Report("afan_rpn_proposals", f"B{B}-{shape}")
    n = R.RPN_N
    lists = R.batch_lists(n)
    extra = 11 if shape == "a>pre_n" else 0
    a, pre_n = n + extra, n + (100 if shape == "a<pre_n" else 0)
    dealt = {(i, perm): R.deal(lst, perm=perm, extra=extra) for i, lst in enumerate(lists) for perm in (False, True)}
    which = [(k % len(lists), k % 2 == 1) for k in range(B)]
    boxes, order = np.stack([dealt[w][0] for w in which]), np.stack([dealt[w][1] for w in which])
    bb, bo = rep.inp(gpu, boxes), rep.inp(gpu, order)
    for top_n in R.rpn_top_ns(lists):
        want = [R.proposal_expect(boxes[k], order[k], lists[w[0]].kept(0), top_n) for k, w in enumerate(which)]
        for fill in FILLS:
            tag = f"top_n {top_n} fill {fill:#04x}"
            rows, kept = run_rpn(rep, lib, gpu, bb, bo, B, a, pre_n, R.T7, top_n, fill, 16 * n)
            rep.same(f"{tag}: kept", kept, [w[1] for w in want])
            rep.same(f"{tag}: padded", rows, np.stack([w[0] for w in want]))
    rep.done()


def test_rpn_proposals_largest_list_pinned(pkg, gpu):
    lib, rep = pkg._lib.load(), Report("afan_rpn_proposals", "B1-208-blocks")
    lst = R.chain_lattice(perm=True)
    boxes, order = R.deal(lst)
    bb, bo = rep.inp(gpu, boxes[None]), rep.inp(gpu, order[None])
    for top_n in (R.W64 * R.FAR + 9, lst.n + 3):
        rows_w, kept_w = R.proposal_expect(boxes, order, lst.kept(0), top_n)
        for fill in FILLS:
            rows, kept = run_rpn(rep, lib, gpu, bb, bo, 1, lst.n, lst.n, lst.t, top_n, fill, 16 * lst.n)
            rep.same(f"top_n {top_n} fill {fill:#04x}: kept", kept, [kept_w])
            rep.same(f"top_n {top_n} fill {fill:#04x}: padded", rows[0], rows_w)
    rep.done()


def test_rpn_proposals_pair_table_pinned(pkg, gpu):
    """The pair test a second time, under the BATCHED templates: up to 64 pairs of one threshold per call, inclusive = 0."""
    lib, rep = pkg._lib.load(), Report("afan_rpn_proposals", "pair-table")
    pairs = R.pair_table()
    struck = R.pair_decisions(pairs, 0)
    boxes, order = pair_arrays(pairs)
    groups = R.pairs_by_threshold(pairs)
    rep.expect(sum(len(idx) for _, idx in groups) == len(pairs) and max(len(idx) for _, idx in groups) == R.RPN_MAX_B, "the table itself: the groups")
    for t, idx in groups:
        B = len(idx)
        bb, bo = rep.inp(gpu, boxes[idx]), rep.inp(gpu, order[idx])
        pos = np.stack([boxes[k][order[k]] for k in idx])                                 # rows in score order
        pos[struck[idx], 1] = 0
        for fill in FILLS:
            rows, kept = run_rpn(rep, lib, gpu, bb, bo, B, 2, 2, t, 2, fill, 32)
            rep.same(f"t {float(t)!r} fill {fill:#04x}: kept", kept, 2 - struck[idx].astype(I64))
            rep.same(f"t {float(t)!r} fill {fill:#04x}: padded", rows, pos)
    rep.done()


# ========================================================================================================================== refusals
def test_nms_refusals(pkg, gpu):
    lib, rep = pkg._lib.load(), Report("afan_nms / afan_nms_top", "refusals")
    n = 70
    boxes, order = R.deal(R.disjoint(n))
    bb, bo = rep.inp(gpu, boxes), rep.inp(gpu, order)
    ws, bk, bc = rep.buf(gpu, R.workspace_bytes(n) + 8), rep.buf(gpu, 8 * n), rep.buf(gpu, 8)
    t = cf(0.7)
    for bad_n in (-1, R.MAX_N + 1, R.LDS_N + 1):
        rep.rc(lib.afan_nms(P(bb), P(bo), bad_n, t, 0, P(ws), P(bk), P(bc), _st()), R.ESHAPE)
        rep.rc(lib.afan_nms_top(P(bb), P(bo), bad_n, t, 0, P(ws), P(bk), P(bc), 5, _st()), R.ESHAPE)
    rep.rc(lib.afan_nms_top(P(bb), P(bo), n, t, 0, P(ws), P(bk), P(bc), -1, _st()), R.ESHAPE)
    args = [P(bb), P(bo), n, t, 0, P(ws), P(bk), P(bc), _st()]
    for slot in (0, 1, 5, 6, 7):
        rep.rc(lib.afan_nms(*[None if i == slot else v for i, v in enumerate(args)]), R.ENULL)
    rep.rc(lib.afan_nms(P(bb), P(bo), n, t, 0, P(ws, 4), P(bk), P(bc), _st()), R.EALIGN)
    rep.expect(ws.untouched() and bk.untouched() and bc.untouched(), "written on a refusal")
    # n = 0: a zero count and nothing else
    rep.rc(lib.afan_nms(None, None, 0, t, 0, None, None, P(bc), _st()))
    rep.rc(lib.afan_nms(P(bb), P(bo), 0, t, 0, P(ws), P(bk), P(bc), _st()))
    rep.same("n = 0: count", bc.get(I64), [0])
    rep.expect(ws.untouched() and bk.untouched(), "n = 0: written besides the count")
    rep.done()


def test_rpn_proposals_refusals(pkg, gpu):
    lib, rep = pkg._lib.load(), Report("afan_rpn_proposals", "refusals")
    n, B, top = 70, 2, 8
    boxes, order = R.deal(R.disjoint(n))
    bb, bo = rep.inp(gpu, np.stack([boxes, boxes])), rep.inp(gpu, np.stack([order, order]))
    ws, bp, bk = rep.buf(gpu, R.rpn_workspace_bytes(B, n) + 8), rep.buf(gpu, 16 * B * top + 16), rep.buf(gpu, 8 * B)
    t = cf(0.7)
    call = lambda **kw: lib.afan_rpn_proposals(*[kw.get(k, v) for k, v in (("boxes", P(bb)), ("order", P(bo)), ("b", B), ("a", n), ("pre_n", n), ("t", t),
                                                                           ("top_n", top), ("ws", P(ws)), ("padded", P(bp)), ("kept", P(bk)), ("st", _st()))])
    for kw in ({"a": -1}, {"pre_n": -1}, {"b": -1}, {"b": R.RPN_MAX_B + 1}, {"top_n": -1}, {"a": R.MAX_N + 1, "pre_n": R.MAX_N + 1},
               {"a": R.LDS_N + 1, "pre_n": R.LDS_N + 1}):
        rep.rc(call(**kw), R.ESHAPE)
    for name in ("boxes", "order", "ws", "padded", "kept"):
        rep.rc(call(**{name: None}), R.ENULL)
    rep.rc(call(ws=P(ws, 4)), R.EALIGN)
    rep.rc(call(padded=P(bp, 8)), R.EALIGN)
    rep.rc(call(boxes=P(bb, 8)), R.EALIGN)
    rep.expect(ws.untouched() and bp.untouched() and bk.untouched(), "written on a refusal")
    # top_n = 0 with padded NULL: the counts alone
    rep.rc(call(top_n=0, padded=None))
    rep.same("top_n = 0: kept", bk.get(I64), [0, 0])
    rep.expect(bp.untouched(), "top_n = 0: padded written")
    rep.done()
