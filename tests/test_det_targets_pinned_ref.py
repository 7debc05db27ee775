"""The references of tests/det_targets_pinned_refs.py (what tests/test_det_targets_pinned_gpu.py holds the detection target, sampling,
loss and class-NMS kernels to) checked on the CPU: the fp32 restatements bit for bit against the tensor-operation forms of
tests/det_torch_ref.py run on CPU tensors, the float64 losses and gradients against torch autograd in float64, the NMS restatement
against the C oracle on tie-free lists and against hand-computed lists on tied ones, the exactly constructible IoUs at their values,
the planted rows of the exact tables at the labels the rules give them by hand, and the coverage of the two sources' exports."""
import inspect
import os

import numpy as np
import pytest
import torch

import det_targets_pinned_refs as R
import det_torch_ref as T
from conftest import ROOT, ptr

F, I64 = R.F, R.I64


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def same_bits(a, b):
    return R.same_f32(a, b) is None


# ========================================================================================================================== coverage
def test_every_export_of_the_two_sources_has_a_table_and_a_gpu_test(pkg):
    import test_det_targets_pinned_gpu as G
    exports = []
    for src in R.SOURCES:
        with open(os.path.join(ROOT, src)) as fh:
            exports += R.exports_of(fh.read())
    assert len(exports) == len(set(exports)) == 12, exports
    assert set(exports) <= set(pkg._lib.SIGNATURES), set(exports) - set(pkg._lib.SIGNATURES)
    assert set(exports) == set(R.TABLES) == set(G.CALLED), set(exports) ^ set(R.TABLES) ^ set(G.CALLED)
    for name in exports:
        assert len(R.TABLES[name]) > 0, name
        assert f"lib.{name}(" in inspect.getsource(G), name
        assert G.CALLED[name].__name__.startswith("test_") and getattr(G, G.CALLED[name].__name__) is G.CALLED[name], name


# ============================================================================================================================== IoUs
def test_the_exactly_constructible_ious():
    b = lambda *v: np.array(v, F)
    assert R.iou_cont(b(0, 0, 4, 1), b(0, 0, 1, 1)) == F(0.25)
    assert R.iou_cont(b(0, 0, 2, 1), b(0, 0, 1, 1)) == F(0.5)
    assert R.iou_cont(b(0, 0, 3, 1), b(0, 0, 4, 1)) == F(0.75)
    assert R.iou_cont(b(0, 0, 1, 1), b(5, 5, 6, 6)) == F(0) and np.isnan(R.iou_cont(b(0, 0, 0, 0), b(0, 0, 0, 0)))
    # with the + 1: [0,0,1,0] has area 2, [0,0,3,0] area 4, intersection 2: 2 / 4
    assert R.iou_incl(b(0, 0, 1, 0), b(0, 0, 3, 0)) == F(0.5) and R.iou_incl(b(0, 0, 0, 0), b(0, 0, 0, 0)) == F(1)
    assert R.iou_incl(b(0, 0, 0, 0), b(1, 0, 1, 0)) == F(0)            # adjacent pixels: w = 0 - 1 + 1 = 0


@pytest.mark.parametrize("kind", ("exact", "gauss"))
def test_iou_restatement_has_the_bits_of_the_tensor_form(kind):
    boxes, gt, _, _ = R.assign_inputs(R.AC(0, 3, 257, 1025, kind))
    want = T.box_iou(tt(boxes), tt(gt)).numpy()
    assert same_bits(R.iou_cont(boxes[:, :, None, :], gt[:, None, :, :]), want)


def test_first_max_is_torch_max():
    v = np.array([[1, 3, 3, 2], [1, np.nan, 5, np.nan], [np.nan, 1, 2, 3], [0, 0, 0, 0], [-1, -np.inf, -1, -2]], F)
    val, arg = torch.from_numpy(v).max(dim=1)
    got_v, got_a = R.first_max(v)
    assert got_a.tolist() == arg.tolist() == [1, 1, 0, 0, 0] and same_bits(got_v, val.numpy())


# ======================================================================================================================== assignment
@pytest.mark.parametrize("shape", [(3, 257, 3), (3, 300, 1025), (1, 513, 1), (1, 1, 1)], ids=str)
@pytest.mark.parametrize("kind", ("exact", "gauss"))
def test_assignment_restatement_equals_the_tensor_forms(shape, kind):
    """det_torch_ref writes the reference's thresholds (0.3 / 0.7 and 0.5) into its functions: the restatement is run with those here,
    and with the tables' dyadic 0.25 / 0.75 against the same functions' steps restated inline."""
    boxes, gt, cls, _ = R.assign_inputs(R.AC(0, *shape, kind))
    lab, asg = R.box_assign(boxes, gt, 0, 0.3, 0.7)
    tl, ta = T.anchor_labels(tt(boxes), tt(gt))
    assert np.array_equal(lab, tl.numpy()) and np.array_equal(asg, ta.numpy())
    lab, asg = R.box_assign(boxes, gt, 1, 0.5, 9.0, cls)
    tl, ta = T.proposal_labels(tt(boxes), tt(gt), tt(cls))
    assert np.array_equal(lab, tl.numpy()) and np.array_equal(asg, ta.numpy())
    # the tables' thresholds
    ious = T.box_iou(tt(boxes), tt(gt))
    amax, aarg = ious.max(dim=2)
    gmax, _ = ious.max(dim=1)
    want = torch.full(amax.shape, -1, dtype=torch.long)
    want[amax < R.LO] = 0
    want[((ious > 0) & (ious == gmax.unsqueeze(1))).any(dim=2)] = 1
    want[amax >= R.HI] = 1
    lab, asg = R.box_assign(boxes, gt, 0, R.LO, R.HI)
    assert np.array_equal(lab, want.numpy()) and np.array_equal(asg, aarg.numpy())


def test_no_ground_truth():
    lab, asg = R.box_assign(np.zeros((2, 5, 4), F), np.zeros((2, 0, 4), F), 0, R.LO, R.HI)
    assert (lab == -1).all() and (asg == 0).all()


@pytest.mark.parametrize("G", (1024, 1025))
def test_the_planted_rows_of_the_exact_table_get_the_labels_the_rules_give_by_hand(G):
    c = R.AC(0, 3, 300, G, "exact")
    boxes, gt, cls, plan = R.assign_inputs(c)
    lab0, asg = R.box_assign(boxes, gt, 0, R.LO, R.HI, cls)
    lab1, _ = R.box_assign(boxes, gt, 1, R.LO, R.HI, cls)
    ious = R.iou_cont(boxes[0][:, None, :], gt[0][None, :, :])
    a, b, d, e, z = (plan[k][2] for k in "ABDEZ")
    ga, gb, gc, gd, ge, gz = (plan[k][1] for k in ("A", "B", "C", "D", "E", "Z"))
    assert [float(ious[i, ga]) for i in a] == [0.25, 0.5, 1.0] and [float(ious[i, gb]) for i in b] == [0.75, 1.0]
    # exactly on lo: not background; exactly on hi: foreground by >= (it is not its ground truth's best: the identical box is)
    assert lab0[0, a].tolist() == [-1, -1, 1] and lab0[0, b].tolist() == [1, 1]
    assert lab1[0, a].tolist() == [cls[0, ga]] * 3 and lab1[0, b].tolist() == [cls[0, gb]] * 2
    # the disjoint ground truth: best IoU exactly 0, and background boxes exist (the v > 0 guard)
    assert float(ious[:, gc].max()) == 0.0 and (lab0[0] == 0).sum() > 10
    # the tying pair, in different workgroups, foreground by the tie alone
    assert d[1] - d[0] > R.TB and float(ious[d[0], gd]) == float(ious[d[1], gd]) == 0.5 == float(ious[:, gd].max()) and lab0[0, d].tolist() == [1, 1]
    # duplicate ground truths: the first wins
    assert (gt[0, ge] == gt[0, plan["E2"][1]]).all() and asg[0, e[0]] == ge < plan["E2"][1]
    # 0 / 0: the NaN takes the assignment, the label stays -1 in both modes
    assert np.isnan(ious[z[0], gz]) and asg[0, z[0]] == gz and lab0[0, z[0]] == -1 and lab1[0, z[0]] == -1
    # the NaN box: no label, and no tie label anywhere in its image
    bn, _, (n,) = plan["nan"]
    assert lab0[bn, n] == -1 and lab1[bn, n] == -1 and not ((lab0[bn] == 1) & (R.first_max(R.iou_cont(boxes[bn][:, None], gt[bn][None]))[0] < F(R.HI))).any()


# ========================================================================================================================== sampling
@pytest.mark.parametrize("case", R.LISTS_CASES, ids=str)
def test_lists_are_nonzero(case):
    labels = R.lists_inputs(case)
    fg, bg = R.sample_lists(labels)
    t = tt(labels)
    assert np.array_equal(fg, (t > 0).nonzero().view(-1).numpy()) and np.array_equal(bg, (t == 0).nonzero().view(-1).numpy())
    if case.kind == "all_fg":
        assert len(fg) == case.M and len(bg) == 0
    if case.kind == "all_ignored":
        assert len(fg) == len(bg) == 0


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=str)
def test_gather_restatement_equals_the_tensor_form(case):
    boxes, gt, assign, labels, fg, bg, pos = R.gather_inputs(case)
    sel, ob, ol, obat, lin, logs, s_log, equal = R.sample_gather(fg, bg, pos, boxes, gt, assign, labels)
    want_sel = np.where(pos >= 0, fg[np.maximum(pos, 0)], bg[np.maximum(-pos - 1, 0)])
    assert np.array_equal(sel, want_sel) and np.array_equal(obat, sel // case.N)
    src = tt(boxes).view(-1, 4)[tt(sel)]
    dst = tt(gt)[tt(obat), tt(assign).view(-1)[tt(sel)]]
    d32 = T.box_deltas(src, dst).numpy()
    assert same_bits(ob, src.numpy()) and same_bits(lin, d32[:, :2])
    d64 = T.box_deltas(src.double(), dst.double()).numpy()
    assert np.allclose(logs, d64[:, 2:], rtol=1e-13, atol=1e-15)
    assert (d32[:, 2:][equal] == 0).all() and (logs[equal] == 0).all()
    ok, ratio, _ = R.window(d32[:, 2:], logs, R.C_LOG * R.U * s_log)    # the CPU's own logf sits inside the counted window
    assert ok, ratio


# ============================================================================================================================ decode
@pytest.mark.parametrize("case", R.DECODE_CASES, ids=str)
def test_decode_restatements_against_the_tensor_form(case):
    src, t = R.decode_inputs(case)
    got, known = R.decode_clip_f32(src, t, R.RIGHT, R.BOTTOM)
    want = T.box_clip(T.box_apply(tt(src), tt(t)), R.RIGHT, R.BOTTOM).numpy()
    assert same_bits(got[known], want[known])
    ref, S = R.decode_clip_f64(src, t, R.RIGHT, R.BOTTOM)
    ok, ratio, _ = R.window(want, ref, R.C_DECODE * R.U * S)
    assert ok, ratio
    if case.kind == "dyadic":
        assert known.all() and same_bits(got, ref.astype(F)) and (ref == ref.astype(F)).all()
    if case.kind == "specials":
        nan = np.isnan(want)
        assert known[0] and nan[0, [0, 2]].all() and not nan[0, [1, 3]].any(), "a NaN transformer stays NaN through the reference's clamp"
        if case.n > 1:
            assert nan[1, [0, 2]].all() and np.isfinite(src[1]).all() and np.isfinite(t[1]).all(), "inf * 0 from finite inputs"


# ============================================================================================================================ losses
@pytest.mark.parametrize("case", [c for c in R.LOSS_CASES if c.S in (1, 257, 600)], ids=str)
def test_float64_losses_and_gradients_are_torch_autograd(case):
    c, x = case, R.loss_inputs(case)
    f = R.det_loss_f64(x["logits"], x["deltas"], x["rows"], x["labels"], x["gt_deltas"], x["batch"], c.B, c.C, c.K, x["beta"], x["norm"])
    bw = R.det_loss_bwd_f64(f, x["g_ce"], x["g_sl"], x["labels"], x["batch"], c.C, c.K, x["R"])
    logits, deltas = tt(x["logits"]).double().requires_grad_(True), tt(x["deltas"]).double().requires_grad_(True)
    lab, r = tt(x["labels"]), tt(f["rows"])
    tg = tt(x["gt_deltas"]).double()
    if x["norm"] is not None:
        tg = (tg - tt(x["norm"][:4]).double()) / tt(x["norm"][4:]).double()
    ce, sl = T.per_image_losses(logits[r], deltas[r, 0 if c.K == 1 else lab], lab, tg, c.B, tt(x["batch"]), float(x["beta"]))
    has = ~torch.isnan(ce)
    assert np.array_equal(np.isnan(f["ce"]), ~has.numpy())
    assert np.allclose(f["ce"][has.numpy()], ce[has].detach().numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(f["sl"], sl.detach().numpy(), rtol=1e-12, atol=1e-14)
    ((ce[has] * tt(x["g_ce"]).double()[has]).sum() + (sl * tt(x["g_sl"]).double()).sum()).backward()
    # (the inf of a -inf logit is excluded from autograd's comparison: its gradient there is nan in torch and 0 by the definition p - onehot)
    fin = np.isfinite(x["logits"]).all(axis=1)
    assert np.allclose(bw[0][fin], logits.grad.numpy()[fin], rtol=1e-11, atol=1e-14)
    assert np.allclose(bw[3], deltas.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert (bw[0][~bw[2]] == 0).all() and (bw[3][~bw[5]] == 0).all()
    # every S dominates its value
    assert (f["s_ul"] >= np.abs(f["ul"])).all() and (f["s_u"] >= np.abs(f["u"])).all()
    if c.kind == "exact":
        sl32, u32, dd32 = R.sl1_exact_f32(x["deltas"], x["rows"], x["labels"], x["gt_deltas"], x["batch"], c.B, c.K, x["beta"], x["g_sl"], x["R"])
        assert (u32.astype(np.float64) == f["u"]).all() and np.allclose(sl32, f["sl"], rtol=2 ** -23)
        assert c.S == 1 or {-1.0, -0.5, 0.0, 0.5, 1.0} <= set(u32.ravel().tolist()), "e / beta and both saturated signs"
        assert np.allclose(dd32, bw[3], rtol=2 ** -22, atol=0)


def test_beta_edges_of_the_gaussian_table():
    x = R.loss_inputs(R.LSC(257, 1, 21, 21, 1.0 / 9, "null", "null", "gauss"))
    e = x["deltas"][3, x["labels"][3]] - x["gt_deltas"][3]
    assert x["labels"][3] != 0 and abs(abs(float(e[0])) - float(x["beta"])) <= 2 ** -24 and float(e[2]) == 0.0


# ====================================================================================================================== NMS and pack
@pytest.mark.parametrize("n", (2, 257, 2048))
def test_greedy_nms_is_the_c_oracle_on_tie_free_lists(c_oracle, n):
    prop, t, probs, _ = R.nms_inputs(R.NC(1, n, 2, "gauss"))
    boxes, _ = R.decode_clip_f32(prop[0], t[0, :, 1] * R.NMS_NORM[4:] + R.NMS_NORM[:4], R.RIGHT, R.BOTTOM)
    p = probs[0, :, 1]
    assert len(np.unique(p)) == n
    order = np.argsort(-p, kind="stable").astype(I64)
    keep, scratch = np.zeros(n, I64), np.zeros(n, np.uint8)
    k = c_oracle.oracle_nms(ptr(np.ascontiguousarray(boxes)), ptr(order), n, R.NMS_THRESH, 0, ptr(keep), ptr(scratch))
    assert R.greedy_nms(boxes, order, R.NMS_THRESH).tolist() == keep[:k].tolist() and 0 < k and (k < n or n == 2)


def test_class_nms_on_tied_lists_by_hand():
    """Four proposals, two classes, identity transformers.  Boxes 0 and 2 are identical, 1 overlaps them by 11 x 11 / (121 + 121 + ... ),
    3 is far away.  Equal probabilities: ascending index decides."""
    prop = np.array([[[0, 0, 10, 10], [0, 0, 10, 10.5], [0, 0, 10, 10], [100, 100, 110, 110]]], F)
    t = np.zeros((1, 4, 2, 4), F)
    norm = np.array([0, 0, 0, 0, 1, 1, 1, 1], F)
    run = lambda p, mp: R.det_class_nms(prop, t, np.stack([np.zeros(4, F), np.array(p, F)], axis=1)[None], norm, 600, 400, 0.5, mp)
    ob, op, counts, known = run([1, 1, 1, 1], 0.25)                     # all tied at 1.0: 0 strikes 1 and 2, 3 survives
    assert known.all() and counts.tolist() == [2] and ob[0, :2].tolist() == [prop[0, 0].tolist(), prop[0, 3].tolist()]
    ob, op, counts, _ = run([0.5, 1, 0.5, 0.25], 0.25)                  # 1 leads and strikes 0 and 2; 3 is exactly on min_prob: out
    assert counts.tolist() == [1] and ob[0, 0].tolist() == prop[0, 1].tolist() and op[0, 0] == 1
    ob, op, counts, _ = run([0.5, 0.25, 0.5, 0.25], 0.25)               # 0 before 2 by index
    assert counts.tolist() == [1] and ob[0, 0].tolist() == prop[0, 0].tolist()
    ob, op, counts, _ = run([0.25, 0.25, 0.25, 0.25], 0.25)             # an empty list
    assert counts.tolist() == [0]
    ob, op, counts, _ = run([0.25, 0.5, 0.25, 0.25], -1.0)              # min_prob < 0: every box enters
    assert counts.tolist() == [2] and op[0, :2].tolist() == [0.5, 0.25]


def test_the_tied_tables_hold_ties_and_the_probability_one_block():
    for c in R.NMS_CASES:
        if c.kind != "ties":
            continue
        prop, t, probs, mp = R.nms_inputs(c)
        if c.N >= 255:
            assert (probs == 1).any() and (probs == F(mp)).any()
            p = probs[0, :, c.C - 1]
            assert len(np.unique(p[p > mp])) < (p > mp).sum() / 4
    assert any(c.B * (c.C - 1) > R.TB for c in R.NMS_CASES), "more lists than one trip of the pack's prefix"


def test_pack_out_of_range_counts_by_hand():
    c = R.PC(6, 5, "out_of_range")
    boxes, probs, counts, total = R.pack_inputs(c)
    assert counts.tolist() == [2, 9, -2, 1, 0, -7] and total == 10
    fb, fp, w = R.det_pack(boxes, probs, counts, total)
    # offsets 0, 2, 11, 9, 10, 10: the count above N moved the offset by 9 and copied 5 rows; the negative one moved it back by 2
    assert w.tolist() == [True] * 7 + [False, False, True]
    assert fp[:2].tolist() == probs[0, :2].tolist() and fp[2:7].tolist() == probs[1].tolist() and fp[9] == probs[3, 0]


# ====================================================================================================================== small entries
def test_small_entries_by_hand():
    cand = np.arange(40, dtype=F).reshape(10, 4)
    rows, kept = R.proposal_rows(cand, 10, np.array([3, -1, 99, 2], I64), 4, 7, 3)
    assert kept == 3 and rows.tolist() == [cand[3].tolist(), cand[0].tolist(), cand[9].tolist()]
    rows, kept = R.proposal_rows(cand, 10, np.array([3, 1], I64), 2, 7, 5)
    assert kept == 2 and rows[2:].tolist() == [[0.0] * 4] * 3
    assert R.proposal_rows(cand, 0, np.array([3], I64), 1, 1, 2)[0].tolist() == [[0.0] * 4] * 2
    lab = R.labels_limit(np.ones((2, 4), I64), (1, 3))
    assert lab.tolist() == [[1, 1, 1, -1]] * 2
    a, b, c, d = R.sum_inputs(4, "order")
    assert R.sum_scalars(a, b, c, d) == F(0) and F(F(a + d) + F(b + c)) != F(0)
    assert R.sum_scalars(a, b) == F(1) and R.sum_scalars(a, b, c) == F(1)


def test_window_helper():
    ok, ratio, _ = R.window([1.0, np.nan, 5.0], [1.0, np.nan, 5.5], [0.0, 0.0, 1.0])
    assert ok and ratio == 0.5
    assert not R.window([0.0], [np.nan], [1.0])[0] and not R.window([np.nan], [0.0], [np.inf])[0] and not R.window([2.0], [0.0], [1.0])[0]
