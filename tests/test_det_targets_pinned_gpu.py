"""Every export of csrc/afan_det_targets.hip and csrc/afan_det_eval.hip — the detection targets, the sampling, the four losses with
their gradients, the per-class NMS and its pack — called through the C ABI and held to the references of tests/det_targets_pinned_refs.py
(numpy, from the definitions; tests/test_det_targets_pinned_ref.py checks them on the CPU).  What is a chain of single fp32 operations
is held BIT FOR BIT: IoUs and with them labels and assignments in both modes, the tie pass, the lists, the gathered rows and their
linear target columns, decode + clip wherever expf's value is known (expf(0) = 1, overflow, underflow), the whole per-class NMS on
such inputs, the pack, the small entries, and the smooth-L1 side of the exact loss table.  Decode with real exponentials, the log
target columns, ce, sl1 and the four gradient tensors are held ELEMENTWISE to float64 inside |got - f64| <= C * 2^-24 * S with the C
counted in det_targets_pinned_refs's docstring; no constant is fitted, no element is exempt.

Conventions (those of tests/test_update_pinned_gpu.py, whose Buf this module uses): every buffer is its own allocation with a 256-byte
guard band on both sides, pre-filled with the byte 0xA5, guard bands checked after every call; inputs are checked unwritten; what an
entry leaves alone (list entries behind the counts, NMS rows behind a list's count, everything on a refusal) still holds the fill;
return codes are checked.  Each case prints "DTPIN <export> <case>" and, for windowed quantities, the worst |got - f64| / bound (run
with -s).  norm arguments are host pointers (the entries read them on the host).

On an MI355X every case passes after two kernel fixes the tables asked for (a NaN coordinate through the two clips; a NaN of either
sign above everything in the per-ground-truth maximum): DESIGN.md section 5.  Worst ratios: decode 0.34, log targets 0.33, ce 0.03, sl1
0.05, u_logits 0.07, u_deltas 0.21, d_logits 0.17, d_deltas 0.16.  The module's 310 cases take 4.1 s in all, the slowest 0.3 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import det_targets_pinned_refs as R
from test_update_pinned_gpu import Buf, P, SENT, _st

pytestmark = pytest.mark.gpu

F, I64, U = R.F, R.I64, R.U


class Report:
    def __init__(self, export, case):
        self.what, self.fails, self.bufs, self.inputs = f"{export} {case}", [], [], []
        print(f"DTPIN {export} {case}")

    def buf(self, dev, nbytes, init=None):
        b = Buf(dev, int(nbytes), 0, init)
        self.bufs.append(b)
        return b

    def inp(self, dev, a):
        """A device copy of an input array, checked unwritten at the end."""
        a = np.ascontiguousarray(a)
        b = self.buf(dev, a.nbytes, a)
        self.inputs.append((b, a.copy()))
        return b

    def expect(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def rc(self, got, want=R.OK):
        self.expect(got == want, f"returned {got}, expected {want}")

    def f32(self, name, got, want):
        i = R.same_f32(got, want)
        if i is not None:
            g, w = np.asarray(got, F).ravel(), np.asarray(want, F).ravel()
            self.expect(False, f"{name}: first difference at {i} of {g.size}: got {g[i]!r} ({g[i:i + 1].view(np.uint32)[0]:#010x}), "
                               f"expected {w[i]!r} ({w[i:i + 1].view(np.uint32)[0]:#010x})")

    def i64(self, name, got, want):
        got, want = np.asarray(got, I64).ravel(), np.asarray(want, I64).ravel()
        bad = np.flatnonzero(got != want) if got.size == want.size else [0]
        if got.size != want.size or len(bad):
            self.expect(False, f"{name}: {len(bad)} of {want.size} differ, first at {bad[0]}: got {got[bad[0]] if got.size == want.size else got.size}, "
                               f"expected {want[bad[0]] if got.size == want.size else want.size}")

    def win(self, name, got, ref, bound):
        ok, ratio, i = R.window(got, ref, bound)
        print(f"    {name}: worst |got - f64| / bound = {ratio:.3f} over {np.size(ref)}")
        if not ok:
            g, r, b = np.ravel(got), np.ravel(ref), np.ravel(bound)
            self.expect(False, f"{name}: element {i} of {g.size}: got {g[i]!r}, float64 {r[i]!r}, bound {b[i]!r} (worst ratio {ratio:.3f})")

    def fill(self, name, raw_bytes):
        self.expect(bool((np.asarray(raw_bytes).view(np.uint8) == SENT).all()), f"{name}: written where the entry must leave the buffer alone")

    def done(self):
        for k, (b, a) in enumerate(self.inputs):
            self.expect(np.array_equal(b.get(np.uint8), a.reshape(-1).view(np.uint8)), f"input {k} was written")
        for k, b in enumerate(self.bufs):
            self.expect(b.guards_ok(), f"the guard band of buffer {k} was written")
        assert not self.fails, f"{self.what}:\n  " + "\n  ".join(self.fails[:12])


def cid(c):
    return "-".join(f"{k}{v}" if not isinstance(v, str) else v for k, v in c._asdict().items())


def host(a):
    return None if a is None else np.ascontiguousarray(a, F).ctypes.data_as(ctypes.c_void_p)


# ================================================================================================================ afan_box_decode_clip
@pytest.mark.parametrize("case", R.DECODE_CASES, ids=cid)
def test_decode_clip_pinned(pkg, gpu, case):
    lib, rep = pkg._lib.load(), Report("afan_box_decode_clip", cid(case))
    src, t = R.decode_inputs(case)
    bs, bt, bo = rep.inp(gpu, src), rep.inp(gpu, t), rep.buf(gpu, 16 * case.n)
    rep.rc(lib.afan_box_decode_clip(P(bs), P(bt), P(bo), case.n, R.RIGHT, R.BOTTOM, _st()))
    got = bo.get(F).reshape(case.n, 4)
    want, known = R.decode_clip_f32(src, t, R.RIGHT, R.BOTTOM)
    rep.expect(case.kind != "dyadic" or bool(known.all()), "the table itself: every row of the dyadic table is known bit for bit")
    rep.f32("rows with a known exponential", got[known], want[known])
    ref, S = R.decode_clip_f64(src, t, R.RIGHT, R.BOTTOM)
    rep.win("boxes", got, ref, R.C_DECODE * U * S)
    if case.kind == "specials":
        rep.expect(bool(np.isnan(ref).any()), "the table itself: NaN rows are present")
    rep.done()


# ===================================================================================================================== afan_box_assign
def run_assign(rep, lib, dev, mode, boxes, gt, cls):
    B, N, G = boxes.shape[0], boxes.shape[1], gt.shape[1]
    bb = rep.inp(dev, boxes)
    bg = rep.inp(dev, gt) if G else None
    bc = rep.inp(dev, cls) if G and mode == 1 else None
    bl, ba = rep.buf(dev, 8 * B * N), rep.buf(dev, 8 * B * N)
    ws = rep.buf(dev, 4 * B * G) if G and mode == 0 else None
    rc = lib.afan_box_assign(P(bb), P(bg), B, N, G, mode, R.LO, R.HI, P(bc), P(bl), P(ba), P(ws), _st())
    return rc, bl, ba


@pytest.mark.parametrize("case", R.ASSIGN_CASES, ids=cid)
def test_box_assign_pinned(pkg, gpu, case):
    lib, rep = pkg._lib.load(), Report("afan_box_assign", cid(case))
    boxes, gt, cls, _ = R.assign_inputs(case)
    rc, bl, ba = run_assign(rep, lib, gpu, case.mode, boxes, gt, cls)
    rep.rc(rc)
    labels, assign = R.box_assign(boxes, gt, case.mode, R.LO, R.HI, cls)
    rep.i64("labels", bl.get(I64), labels)
    rep.i64("assign", ba.get(I64), assign)
    rep.done()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("kind", ("exact", "gauss"))
def test_box_assign_above_the_lds_cap_agrees_with_its_truncation(pkg, gpu, mode, kind):
    """G = 1025 (global atomics only) against the same data cut to G = 1024 (the LDS merge): wherever the reference's decisions agree,
    the kernel's do."""
    lib, rep = pkg._lib.load(), Report("afan_box_assign", f"mode{mode}-{kind}-1025-vs-1024")
    c = R.AC(mode, 3, 300, R.MAX_G_LDS + 1, kind)
    boxes, gt, cls, _ = R.assign_inputs(c)
    out, ref = [], []
    for g in (R.MAX_G_LDS + 1, R.MAX_G_LDS):
        rc, bl, ba = run_assign(rep, lib, gpu, mode, boxes, np.ascontiguousarray(gt[:, :g]), np.ascontiguousarray(cls[:, :g]))
        rep.rc(rc)
        out.append((bl.get(I64).reshape(3, 300), ba.get(I64).reshape(3, 300)))
        ref.append(R.box_assign(boxes, gt[:, :g], mode, R.LO, R.HI, cls[:, :g]))
    for k, name in enumerate(("labels", "assign")):
        same = ref[0][k] == ref[1][k]
        rep.expect(same.mean() > 0.9, "the table itself: the last ground truth changes few decisions")
        rep.i64(name, out[0][k][same], out[1][k][same])
    rep.done()


def test_box_assign_batch_limit(pkg, gpu):
    lib, rep = pkg._lib.load(), Report("afan_box_assign", "B65535-and-65536")
    for mode in (0, 1):
        c = R.AC(mode, 65535, 1, 1, "gauss")
        boxes, gt, cls, _ = R.assign_inputs(c)
        rc, bl, ba = run_assign(rep, lib, gpu, mode, boxes, gt, cls)
        rep.rc(rc)
        labels, assign = R.box_assign(boxes, gt, mode, R.LO, R.HI, cls)
        rep.expect(len(np.unique(labels)) > 1, "the table itself: more than one label")
        rep.i64("labels", bl.get(I64), labels)
        rep.i64("assign", ba.get(I64), assign)
        big = np.concatenate([boxes, boxes[:1]]), np.concatenate([gt, gt[:1]]), np.concatenate([cls, cls[:1]])
        rc, bl, ba = run_assign(rep, lib, gpu, mode, *big)
        rep.rc(rc, R.ESHAPE)
        rep.expect(bl.untouched() and ba.untouched(), "B = 65536: written on a refusal")
    rep.done()


# ================================================================================================================== afan_sample_lists
@pytest.mark.parametrize("case", R.LISTS_CASES, ids=cid)
def test_sample_lists_pinned(pkg, gpu, case):
    lib, rep = pkg._lib.load(), Report("afan_sample_lists", cid(case))
    labels, M = R.lists_inputs(case), case.M
    bl = rep.inp(gpu, labels) if M else None
    bf, bb = (rep.buf(gpu, 8 * M), rep.buf(gpu, 8 * M)) if M else (None, None)
    bc = rep.buf(gpu, 16)
    rep.rc(lib.afan_sample_lists(P(bl), M, P(bf), P(bb), P(bc), _st()))
    fg, bg = R.sample_lists(labels)
    rep.i64("counts", bc.get(I64), [len(fg), len(bg)])
    if M:
        rep.i64("fg", bf.get(I64)[:len(fg)], fg)
        rep.i64("bg", bb.get(I64)[:len(bg)], bg)
        rep.fill("fg behind its count", bf.get(I64)[len(fg):])
        rep.fill("bg behind its count", bb.get(I64)[len(bg):])
    rep.done()


# ================================================================================================================= afan_sample_gather
@pytest.mark.parametrize("case", R.GATHER_CASES, ids=cid)
def test_sample_gather_pinned(pkg, gpu, case):
    lib, rep = pkg._lib.load(), Report("afan_sample_gather", cid(case))
    boxes, gt, assign, labels, fg, bg, pos = R.gather_inputs(case)
    S = case.S
    ins = [rep.inp(gpu, a) for a in (fg, bg, pos, boxes, gt, assign, labels)]
    bsel, bbox, blab, bdel, bbat = rep.buf(gpu, 8 * S), rep.buf(gpu, 16 * S), rep.buf(gpu, 8 * S), rep.buf(gpu, 16 * S), rep.buf(gpu, 8 * S)
    rep.rc(lib.afan_sample_gather(P(ins[0]), P(ins[1]), P(ins[2]), S, P(ins[3]), P(ins[4]), P(ins[5]), P(ins[6]), case.N, case.G,
                                  P(bsel), P(bbox), P(blab), P(bdel), P(bbat), _st()))
    sel, ob, ol, obat, lin, logs, s_log, equal = R.sample_gather(fg, bg, pos, boxes, gt, assign, labels)
    rep.expect(bool((pos >= 0).any()) or S == 1, "the table itself: foreground positions")
    rep.expect(bool((pos < 0).any()) or S == 1, "the table itself: background positions")
    rep.expect(int(obat[-1]) == case.B - 1, "the table itself: a sample of the last image")
    rep.i64("sel", bsel.get(I64), sel)
    rep.i64("labels", blab.get(I64), ol)
    rep.i64("batch", bbat.get(I64), obat)
    rep.f32("boxes", bbox.get(F), ob)
    got = bdel.get(F).reshape(S, 4)
    rep.f32("target columns 0-1", got[:, :2], lin)
    rep.win("target columns 2-3", got[:, 2:], logs, R.C_LOG * U * s_log)
    if S > 1:
        rep.expect(bool(equal.any()), "the table itself: rows with equal extents")
    rep.f32("target columns 2-3 at equal extents (logf(1) = 0)", got[:, 2:][equal], np.zeros(int(equal.sum()), F))
    rep.done()


# ===================================================================================================== afan_det_loss_fwd, afan_det_loss_bwd
@pytest.mark.parametrize("case", R.LOSS_CASES, ids=cid)
def test_det_loss_pinned(pkg, gpu, case):
    lib, c = pkg._lib.load(), case
    rep = Report("afan_det_loss_fwd/bwd", cid(c))
    x = R.loss_inputs(c)
    S, B, C, K, Rr = c.S, c.B, c.C, c.K, x["R"]
    bl, bd = rep.inp(gpu, x["logits"]), rep.inp(gpu, x["deltas"])
    brow = rep.inp(gpu, x["rows"]) if x["rows"] is not None else None
    blab, bgd, bbat = rep.inp(gpu, x["labels"]), rep.inp(gpu, x["gt_deltas"]), rep.inp(gpu, x["batch"])
    bce, bsl, bsave = rep.buf(gpu, 4 * B), rep.buf(gpu, 4 * B), rep.buf(gpu, 4 * (4 * S + S * C + 2 * B))
    norm = None if x["norm"] is None else np.ascontiguousarray(x["norm"], F)
    rep.rc(lib.afan_det_loss_fwd(P(bl), P(bd), P(brow), P(blab), P(bgd), P(bbat), S, B, C, K, float(x["beta"]), host(norm), P(bce), P(bsl),
                                 P(bsave), _st()))
    f = R.det_loss_f64(x["logits"], x["deltas"], x["rows"], x["labels"], x["gt_deltas"], x["batch"], B, C, K, x["beta"], x["norm"])
    save = bsave.get(F)
    u_d, u_l, den = save[:4 * S].reshape(S, 4), save[4 * S:4 * S + S * C].reshape(S, C), save[4 * S + S * C:].reshape(B, 2)
    c_ce = np.array([R.c_ce(C, int(ch)) for ch in f["chain"]], np.float64)
    c_sl = np.array([R.c_sl1(int(ch)) for ch in f["chain"]], np.float64)
    rep.win("ce", bce.get(F), f["ce"], c_ce * U * f["s_ce"] + R.TINY)
    rep.win("sl1", bsl.get(F), f["sl"], c_sl * U * f["s_sl"] + R.TINY)
    rep.win("u_logits", u_l, f["ul"], R.c_u_logits(C) * U * f["s_ul"] + R.TINY)
    rep.win("u_deltas", u_d, f["u"], R.C_U_DELTAS * U * f["s_u"] + R.TINY)
    rep.f32("denominators", den, f["denom"])
    if B == 3:
        rep.expect(bool(np.isnan(f["ce"][1])) and f["denom"][2, 1] < 1, "the table itself: an image without samples, one without foreground")
    if c.kind == "exact":
        sl32, u32, dd32 = R.sl1_exact_f32(x["deltas"], x["rows"], x["labels"], x["gt_deltas"], x["batch"], B, K, x["beta"], x["g_sl"], Rr)
        rep.f32("sl1 of the exact table", bsl.get(F), sl32)
        rep.f32("u_deltas of the exact table", u_d, u32)
    # the backward, d_deltas behind d_logits in one allocation (one fill) and in its own (two)
    bgce, bgsl = rep.inp(gpu, x["g_ce"]), rep.inp(gpu, x["g_sl"])
    dl, s_dl, own_l, dd, s_dd, own_d, kc = R.det_loss_bwd_f64(f, x["g_ce"], x["g_sl"], x["labels"], x["batch"], C, K, Rr)
    floor = R.TINY * max(1.0, float(kc.max()) if kc.size else 1.0)
    for layout in ("joint", "split"):
        if layout == "joint":
            both = rep.buf(gpu, 4 * Rr * C + 16 * Rr * K)
            pl, pd = both.p(), both.p(4 * Rr * C)
        else:
            b1, b2 = rep.buf(gpu, 4 * Rr * C), rep.buf(gpu, 16 * Rr * K)
            pl, pd = b1.p(), b2.p()
        rep.rc(lib.afan_det_loss_bwd(P(bgce), P(bgsl), P(bsave), P(brow), P(blab), P(bbat), S, B, C, K, Rr, pl, pd, _st()))
        if layout == "joint":
            raw = both.get(F)
            g_l, g_d = raw[:Rr * C].reshape(Rr, C), raw[Rr * C:].reshape(Rr, K, 4)
        else:
            g_l, g_d = b1.get(F).reshape(Rr, C), b2.get(F).reshape(Rr, K, 4)
        rep.expect(not g_l[~own_l].view(np.uint32).any(), f"{layout}: d_logits is not exactly zero outside the sampled rows")
        rep.expect(not g_d[~own_d].view(np.uint32).any(), f"{layout}: d_deltas is not exactly zero outside the sampled rows and classes")
        rep.win(f"{layout} d_logits", g_l, dl, R.c_d_logits(C) * U * s_dl + floor)
        rep.win(f"{layout} d_deltas", g_d, dd, R.C_D_DELTAS * U * s_dd + floor)
        if c.kind == "exact":
            rep.f32(f"{layout} d_deltas of the exact table", g_d, dd32)
    rep.done()


def test_det_loss_refusals(pkg, gpu):
    lib, rep = pkg._lib.load(), Report("afan_det_loss_fwd/bwd", "refusals")
    z = rep.buf(gpu, 256)
    out = [rep.buf(gpu, 64) for _ in range(3)]
    for (S, B, C, K) in ((-1, 1, 2, 1), (1, 0, 2, 1), (1, 1, 0, 1), (1, 1, 3, 2)):
        rep.rc(lib.afan_det_loss_fwd(P(z), P(z), None, P(z), P(z), P(z), S, B, C, K, 1.0, None, P(out[0]), P(out[1]), P(out[2]), _st()), R.ESHAPE)
        rep.rc(lib.afan_det_loss_bwd(P(z), P(z), P(z), None, P(z), P(z), S, B, C, K, 1, P(out[0]), P(out[1]), _st()), R.ESHAPE)
    rep.rc(lib.afan_det_loss_fwd(P(z), P(z), None, P(z), P(z), P(z), 1, 1, 2, 1, 1.0, None, None, P(out[1]), P(out[2]), _st()), R.ENULL)
    rep.expect(all(o.untouched() for o in out) and z.untouched(), "written on a refusal")
    rep.done()


# ==================================================================================================== afan_det_class_nms, afan_det_pack
def test_det_class_nms_supported_pinned(pkg):
    lib = pkg._lib.load()
    print("DTPIN afan_det_class_nms_supported table")
    for n, c in R.TABLES["afan_det_class_nms_supported"]:
        assert lib.afan_det_class_nms_supported(n, c) == int(1 <= n <= R.MAX_N and 2 <= c <= R.MAX_C), (n, c)


@pytest.mark.parametrize("case", R.NMS_CASES, ids=cid)
def test_det_class_nms_and_pack_pinned(pkg, gpu, case):
    lib, rep = pkg._lib.load(), Report("afan_det_class_nms + afan_det_pack", cid(case))
    prop, t, probs, min_prob = R.nms_inputs(case)
    B, N, C = case.B, case.N, case.C
    L = B * (C - 1)
    bp, bt, bpr = rep.inp(gpu, prop), rep.inp(gpu, t), rep.inp(gpu, probs)
    bob, bop, bcn = rep.buf(gpu, 16 * L * N), rep.buf(gpu, 4 * L * N), rep.buf(gpu, 8 * L)
    rep.rc(lib.afan_det_class_nms(P(bp), P(bt), P(bpr), host(R.NMS_NORM), B, N, C, R.RIGHT, R.BOTTOM, R.NMS_THRESH, min_prob, P(bob), P(bop), P(bcn), _st()))
    ob, op, counts, known = R.det_class_nms(prop, t, probs, R.NMS_NORM, R.RIGHT, R.BOTTOM, R.NMS_THRESH, min_prob)
    rep.expect(bool(known.all()), "the table itself: every box is known bit for bit")
    got_c = bcn.get(I64)
    rep.i64("counts", got_c, counts)
    wr = np.arange(N)[None, :] < counts[:, None]
    gb, gp = bob.get(F).reshape(L, N, 4), bop.get(F).reshape(L, N)
    rep.f32("boxes", gb[wr], ob[wr])
    rep.f32("probabilities", gp[wr], op[wr])
    rep.fill("boxes behind the counts", gb[~wr])
    rep.fill("probabilities behind the counts", gp[~wr])
    if case.kind == "ties" and N > 2 and C > 2:
        rep.expect(counts[0] == 0 and counts.max() > 0, "the table itself: an empty list")
    if case.kind == "nan":
        rep.expect(bool(np.isnan(ob[0, 0, [0, 2]]).all()), "the table itself: a NaN box")
    # the pack of the kernel's own lists
    total = int(counts.sum())
    bfb, bfp = rep.buf(gpu, 16 * total), rep.buf(gpu, 4 * total)
    if np.array_equal(got_c, counts):                                       # (the counts place the writes: only the expected ones are sent on)
        rep.rc(lib.afan_det_pack(P(bob), P(bop), P(bcn), L, N, P(bfb), P(bfp), _st()))
        fb, fp, w = R.det_pack(ob, op, counts, total)
        rep.expect(bool(w.all()), "the table itself: the pack is dense")
        rep.f32("flat boxes", bfb.get(F), fb)
        rep.f32("flat probabilities", bfp.get(F), fp)
    rep.done()


@pytest.mark.parametrize("n,c", [(R.MAX_N + 1, 2), (4, R.MAX_C + 1), (0, 2), (4, 1)])
def test_det_class_nms_refusals(pkg, gpu, n, c):
    lib, rep = pkg._lib.load(), Report("afan_det_class_nms", f"refused-N{n}-C{c}")
    ins = [rep.buf(gpu, 16 * max(n, 1) * max(c, 1)) for _ in range(3)]
    outs = [rep.buf(gpu, 16 * max(n, 1) * max(c, 1)) for _ in range(3)]
    rep.rc(lib.afan_det_class_nms(P(ins[0]), P(ins[1]), P(ins[2]), host(R.NMS_NORM), 1, n, c, R.RIGHT, R.BOTTOM, R.NMS_THRESH, 0.1,
                                  P(outs[0]), P(outs[1]), P(outs[2]), _st()), R.ESHAPE)
    rep.expect(all(o.untouched() for o in outs), "written on a refusal")
    rep.done()


@pytest.mark.parametrize("case", R.PACK_CASES, ids=cid)
def test_det_pack_pinned(pkg, gpu, case):
    lib, rep = pkg._lib.load(), Report("afan_det_pack", cid(case))
    boxes, probs, counts, total = R.pack_inputs(case)
    fb, fp, w = R.det_pack(boxes, probs, counts, total)                     # (asserts that every write of the table is in range)
    bb, bp, bc = rep.inp(gpu, boxes), rep.inp(gpu, probs), rep.inp(gpu, counts)
    bfb, bfp = rep.buf(gpu, 16 * total), rep.buf(gpu, 4 * total)
    rep.rc(lib.afan_det_pack(P(bb), P(bp), P(bc), case.L, case.N, P(bfb), P(bfp), _st()))
    gb, gp = bfb.get(F).reshape(total, 4), bfp.get(F)
    rep.f32("flat boxes", gb[w], fb[w])
    rep.f32("flat probabilities", gp[w], fp[w])
    rep.fill("rows no list owns", gb[~w])
    rep.fill("probabilities no list owns", gp[~w])
    rep.rc(lib.afan_det_pack(P(bb), P(bp), P(bc), case.L, 0, P(bfb), P(bfp), _st()), R.ESHAPE)
    rep.done()


# ======================================================================================================================== small entries
@pytest.mark.parametrize("case", R.PROPOSAL_ROWS_CASES, ids=cid)
def test_proposal_rows_pinned(pkg, gpu, case):
    lib, rep, c = pkg._lib.load(), Report("afan_proposal_rows", cid(case)), case
    cand, keep = R.proposal_rows_inputs(c)
    bc = rep.inp(gpu, cand[:c.n_cand]) if c.n_cand else None
    bk = rep.inp(gpu, keep[:c.n_keep]) if c.n_keep else None
    bn = rep.inp(gpu, np.array([c.count], I64))
    br, bkept = rep.buf(gpu, 16 * c.P), rep.buf(gpu, 8)
    rep.rc(lib.afan_proposal_rows(P(bc), c.n_cand, P(bk), c.n_keep, P(bn), c.P, P(br), P(bkept), _st()))
    rows, kept = R.proposal_rows(cand, c.n_cand, keep, c.n_keep, c.count, c.P)
    rep.f32("rows", br.get(F), rows)
    rep.i64("kept", bkept.get(I64), [kept])
    rep.done()


@pytest.mark.parametrize("case", R.LABELS_LIMIT_CASES, ids=cid)
def test_labels_limit_pinned(pkg, gpu, case):
    lib, rep, c = pkg._lib.load(), Report("afan_labels_limit", cid(case)), case
    labels = np.random.default_rng(c.B + c.N).integers(-1, 21, (c.B, c.N)).astype(I64)
    bl, bk = rep.buf(gpu, labels.nbytes, labels), rep.inp(gpu, np.array(c.kept, I64))
    rep.rc(lib.afan_labels_limit(P(bl), c.B, c.N, P(bk), len(c.kept), _st()))
    rep.i64("labels", bl.get(I64), R.labels_limit(labels, c.kept))
    rep.rc(lib.afan_labels_limit(P(bl), c.B, c.N, P(bk), 0, _st()), R.ESHAPE)
    rep.done()


@pytest.mark.parametrize("n,kind", R.SUM_CASES, ids=lambda v: str(v))
def test_sum_scalars_pinned(pkg, gpu, n, kind):
    lib, rep = pkg._lib.load(), Report("afan_sum_scalars_f32", f"{n}-{kind}")
    v = R.sum_inputs(n, kind)
    b = [rep.inp(gpu, np.array([x], F)) for x in v] + [None] * (4 - n)
    out = rep.buf(gpu, 4)
    rep.rc(lib.afan_sum_scalars_f32(P(b[0]), P(b[1]), P(b[2]), P(b[3]), P(out), _st()))
    rep.f32("sum", out.get(F), [R.sum_scalars(*v)])
    if kind == "order":
        rep.expect(R.sum_scalars(*v) != F(F(v[0] + v[3]) + F(v[1] + v[2])), "the table itself: the order of the additions shows")
    out2 = rep.buf(gpu, 4)
    rep.rc(lib.afan_sum_scalars_f32(P(b[0]), P(b[1]), None, P(b[0]), P(out2), _st()), R.ENULL)                 # d without c
    rep.expect(out2.untouched(), "written on a refusal")
    rep.done()


# the export each test above calls (tests/test_det_targets_pinned_ref.py holds this, the tables and the two sources' exports in step)
CALLED = {
    "afan_box_decode_clip": test_decode_clip_pinned, "afan_box_assign": test_box_assign_pinned, "afan_sample_lists": test_sample_lists_pinned,
    "afan_sample_gather": test_sample_gather_pinned, "afan_det_loss_fwd": test_det_loss_pinned, "afan_det_loss_bwd": test_det_loss_pinned,
    "afan_sum_scalars_f32": test_sum_scalars_pinned, "afan_proposal_rows": test_proposal_rows_pinned, "afan_labels_limit": test_labels_limit_pinned,
    "afan_det_class_nms_supported": test_det_class_nms_supported_pinned, "afan_det_class_nms": test_det_class_nms_and_pack_pinned,
    "afan_det_pack": test_det_pack_pinned,
}
