"""tests/nms_pinned_refs.py (what tests/test_nms_pinned_gpu.py holds the proposal NMS kernels to) checked on the CPU: the np.float32
reference against the C oracle's oracle_nms on every table (the oracle uses fmaxf / fminf, so the NaN rows apply too) and against the
reference's golden 9 770 -> 1 934 list; every planted list against the survivors its planner states by hand; the restated shortcut of
iou_over sound against the division over the whole pair table and an adversarial sweep; and the coverage the tables claim."""
import os

import numpy as np
import pytest

import nms_pinned_refs as R
from conftest import GOLDEN, ptr

F, I64 = R.F, R.I64


def oracle_kept(lib, pos_boxes, t, inclusive, perm_seed=None):
    """kept by position from oracle_nms, run on the identity order or through a permutation of the original indices."""
    n = len(pos_boxes)
    order = np.arange(n, dtype=I64) if perm_seed is None else np.random.default_rng(perm_seed).permutation(n).astype(I64)
    boxes = np.empty((n, 4), F)
    boxes[order] = pos_boxes
    keep, scratch = np.zeros(max(n, 1), I64), np.zeros(max(n, 1), np.uint8)
    k = lib.oracle_nms(ptr(boxes), ptr(order), n, float(t) if not np.isnan(t) else float("nan"), inclusive, ptr(keep), ptr(scratch))
    kept = np.zeros(n, bool)
    inv = np.empty(n, I64)
    inv[order] = np.arange(n)
    kept[inv[keep[:k]]] = True
    return kept


# ============================================================================================================================ constants
def test_the_scan_constants_and_what_is_derived_from_them():
    assert R.SC_NW == R.SCAN_WAVES - 1 - R.SC_P and R.FAR == R.SC_D + 1
    assert R.FAR2 == R.FAR + 3 * R.W64 and R.BIG_BLOCKS * R.W64 == 13312
    assert R.DISTANCES == (0, 1, 12, 13, 14, 25, 31, 32, 33, 100, 205, 206)
    assert R.workspace_bytes(13312) == 13312 * 208 * 8 + 13312 + 208 * 13 * 64 * 8 < 24 << 20
    assert R.LDS_N == 524288 and (R.LDS_N + 1 + R.W64 - 1) // R.W64 * 8 > 64 * 1024


# ===================================================================================================================== lists by hand
@pytest.mark.parametrize("lst", R.list_cases(), ids=repr)
def test_reference_oracle_and_hand_agree_on_every_list(c_oracle, lst):
    for inclusive in lst.modes:
        kept = lst.kept(inclusive)
        if not (lst.perm and lst.n > 4096):                               # (the same positions as its unpermuted twin, 2 s of oracle)
            assert np.array_equal(kept, oracle_kept(c_oracle, lst.pos, lst.t, inclusive)), (lst, inclusive)
        if lst.n <= 4096:
            assert np.array_equal(kept, oracle_kept(c_oracle, lst.pos, lst.t, inclusive, perm_seed=lst.n)), (lst, inclusive, "permuted")
        if lst.hand is not None:
            assert np.array_equal(kept, lst.hand), (lst, inclusive, np.flatnonzero(kept != lst.hand)[:8])
    boxes, order = R.deal(lst)
    assert np.array_equal(boxes[order], lst.pos) or np.isnan(lst.pos).any()
    assert lst.perm == bool(lst.n > 1 and (order != np.arange(lst.n)).all())


@pytest.mark.parametrize("lst", R.batch_lists(R.RPN_N), ids=repr)
def test_reference_oracle_and_hand_agree_on_the_proposal_batch_lists(c_oracle, lst):
    kept = lst.kept(0)
    assert np.array_equal(kept, oracle_kept(c_oracle, lst.pos, lst.t, 0)) and np.array_equal(kept, lst.hand), lst
    if hasattr(lst, "nan_at"):
        assert kept[lst.nan_at].all() and np.isnan(lst.pos[lst.nan_at]).any(axis=1).all()


def test_every_plant_is_kept_struck_kept():
    big = R.chain_lattice()
    assert len(big.pairs) == 29 and {"same", "band1", "bandD", "far1", "farNW", "far2nd"} == {p[0] for p in big.pairs} == {p[1] for p in big.pairs}
    assert ("far1", "far1") in big.pairs and ("bandD", "farNW") in big.pairs and ("same", "far2nd") in big.pairs
    seen = set()
    for lst in (big, R.chain_lattice(perm=True), R.struck_striker(), R.chain_lattice(R.RPN_N)):
        kept = lst.kept(0)
        for a, b, c in lst.plants:
            assert kept[a] and not kept[b] and (c is None or kept[c]), (lst, a, b, c)
            assert a // R.W64 == 0 or lst is R.struck_striker()
            seen.add((b // R.W64 - a // R.W64, None if c is None else c // R.W64 - b // R.W64))
        assert int((~kept).sum()) == len(lst.plants)
    assert {(d, 1) for d in R.DISTANCES} <= seen and (R.FAR + 2, R.FAR) in seen
    # each B has ONE striker and each C none: the pair values by hand
    a, b, c = big.plants[0]
    v = lambda i, j: R.pair_terms(big.pos[i], R.area(big.pos[i]), big.pos[j], R.area(big.pos[j]))[2]
    assert v(a, b) == F(1517) / F(1845) > R.T7 > v(a, c) == F(1353) / F(2009) and v(b, c) == v(a, b)
    sa = R.area(big.pos)
    for a, b, c in big.plants[:6]:
        hits = np.flatnonzero(R.pair_terms(big.pos[b], sa[b], big.pos, sa)[2] > R.T7)
        assert set(hits.tolist()) == {a, b} | ({c} if c is not None else set())


def test_the_structural_lists_are_what_they_claim():
    f = R.fan()
    assert f.kept(0)[:R.W64].all() and not f.kept(0)[R.FAN_D * R.W64:(R.FAN_D + 1) * R.W64].any() and R.W64 // R.SC_RC + 1 == 6
    assert R.fan(single=True).plants == [(R.SC_RC, R.FAN_D * R.W64 + R.SC_RC, None)]
    assert R.chain_in_block(0).kept(0).tolist() == [True, False] * 32
    assert R.chain_in_block(32).kept(0).tolist() == [True] * 32 + [True, False] * 32
    assert R.identical(837).kept(0).sum() == 1 == R.identical(837).kept(1).sum()
    n = R.nan_lattice()
    assert np.isnan(n.pos[n.nan_at]).any(axis=1).all() and n.kept(0)[n.nan_at].all() and n.kept(1)[n.nan_at].all()
    assert [(R.CP_THREADS + m - 1) // R.CP_THREADS for m in R.DISJOINT_N[-4:]] == [1, 1, 2, 3]
    for cb in R.BLOCK_COUNTS:
        for last in R.LASTS:
            lst = R.block_count_list(cb, last)
            assert (lst.n + R.W64 - 1) // R.W64 == cb and (lst.n - 1) % R.W64 + 1 == last
            assert cb == 1 or any(b // R.W64 == cb - 1 for _, b, _ in lst.plants), "a victim in the last block"
    for lst in R.mixed_lists()[-3:]:
        assert 0.05 < lst.kept(0).mean() < 0.2, lst


def test_reference_equals_the_golden_list(c_oracle):
    det = np.load(os.path.join(GOLDEN, "det_nms_large_input.npy"))
    expect = np.load(os.path.join(GOLDEN, "det_nms_large_output.npy"))
    order = np.argsort(-det[:, 4], kind="stable").astype(I64)
    pos = np.ascontiguousarray(det[order, :4], F)
    for inclusive in (0, 1):
        kept = R.greedy(pos, 0.7, inclusive)
        assert R.plain_expect(order, kept).tolist() == sorted(expect.tolist()) and kept.sum() == 1934


# ======================================================================================================================= the pair table
@pytest.mark.parametrize("inclusive", (0, 1))
def test_pair_table_against_the_c_oracle(c_oracle, inclusive):
    pairs = R.pair_table()
    want = R.pair_decisions(pairs, inclusive)
    for k, p in enumerate(pairs):
        kept = oracle_kept(c_oracle, np.stack([p.a, p.b]), p.t, inclusive)
        assert kept[0] and kept[1] == (not want[k]), (k, p, inclusive)
        if k % 16 == 0:
            assert np.array_equal(R.greedy(np.stack([p.a, p.b]), p.t, inclusive), kept)


def test_pair_table_by_hand():
    pairs, s0, s1 = R.pair_table(), R.pair_decisions(R.pair_table(), 0), R.pair_decisions(R.pair_table(), 1)
    find = lambda kind, t: [k for k, p in enumerate(pairs) if p.kind == kind and F(p.t).tobytes() == F(t).tobytes()]
    (k,) = find("identical", 1)
    assert not s0[k] and s1[k]                                           # IoU 1 at t = 1: > keeps both, >= strikes
    (k,) = find("identical", np.nextafter(F(1), F(0)))
    assert s0[k] and s1[k]
    (k,) = find("t-disjoint", F(0))
    assert not s0[k] and s1[k]                                           # 0 >= 0
    for kind in ("t-overlap", "t-disjoint", "t-identical"):
        (k,) = find(kind, R.QNAN)
        assert not s0[k] and not s1[k]
    for k, p in enumerate(pairs):
        if p.kind.startswith("tie"):
            exact = F(p.t) == F(int(p.kind[3:].split("/")[0])) / F(int(p.kind.split("/")[1]))
            assert bool(s1[k]) == bool(s0[k] or exact) and (not exact or not s0[k])
        if p.kind.startswith("nan") or p.kind == "overflow":
            assert not s0[k] and not s1[k], p                            # a NaN area: never struck, strikes nothing
        if p.kind in ("area0-self",):
            assert not s1[k]                                             # 0 / 0
    assert all(F(p.t).view(np.uint32) == 0x7fc00000 for p in pairs if np.isnan(p.t))
    assert all(int(np.asarray(x, F).view(np.uint32)[i]) == 0x7fc00000 for p in pairs for x in (p.a, p.b) for i in np.flatnonzero(np.isnan(x)))


def _terms(pairs):
    a, b = np.stack([p.a for p in pairs]), np.stack([p.b for p in pairs])
    with np.errstate(all="ignore"):
        return R.pair_terms(a, R.area(a), b, R.area(b))


def test_no_subnormal_intermediate_in_the_pair_table():
    for x in _terms(R.pair_table()):
        assert not ((x != 0) & (np.abs(x) < np.finfo(F).tiny)).any()


def test_shortcut_is_sound_on_the_pair_table_and_the_tables_reach_every_path():
    pairs = R.pair_table()
    inter, u, v = _terms(pairs)
    kinds = set()
    for t in {F(p.t).tobytes() for p in pairs}:
        idx = [k for k, p in enumerate(pairs) if F(p.t).tobytes() == t]
        tt = np.frombuffer(t, F)[0]
        decided, hit, sane = R.shortcut(inter[idx], u[idx], tt)
        for inclusive in (0, 1):
            assert np.array_equal(hit[decided], R.over(v[idx], tt, inclusive)[decided]), float(tt)
        kinds |= {("hit" if h else "miss") if d else "undecided" for d, h in zip(decided, hit)} | {("sane" if s else "insane") for s in sane}
    assert kinds == {"hit", "miss", "undecided", "sane", "insane"}
    # the searched pairs sit where they were aimed: within 4 neighbours of t on both sides; inside, outside and far outside the margin
    near = [k for k, p in enumerate(pairs) if p.kind == "near"]
    d = R.ulps(np.array([pairs[k].t for k in near], F), v[near])
    assert len(near) >= 2000 and np.abs(d).max() <= 4 and (d < 0).sum() > 300 and (d > 0).sum() > 300 and (d == 0).sum() > 30
    for kind, want in (("rel1e-06", False), ("rel3e-06", True), ("rel1e-05", True)):
        idx = [k for k, p in enumerate(pairs) if p.kind == kind]
        dec = np.array([R.shortcut(inter[k], u[k], pairs[k].t)[0] for k in idx])
        assert len(idx) >= 700 and dec.all() == want and dec.any() == want, kind
    assert len(near) == sum(p.kind.startswith("rel") for p in pairs) - 6
    # u on both sides of 1e30f
    us = [float(u[k]) for k, p in enumerate(pairs) if p.kind == "u-1e30"]
    assert min(us) < 1e30 < max(us) and max(us) < 1.01e30 and min(us) > 0.99e30


def test_shortcut_is_sound_on_an_adversarial_sweep():
    """40 million (inter, u, t): u log-uniform over [1, 1e30], inter within 40 neighbours of fl(t u) and at relative offsets to 3e-6."""
    rng = np.random.default_rng(404)
    steps = np.arange(-40, 41)
    for t in (F(1e-3), F(0.3), F(1) / F(3), F(0.5), F(0.7), F(0.999), F(1)):
        u = np.exp(rng.uniform(0, np.log(1e30), 41000)).astype(F)
        u[:4] = [1, 1e30, np.nextafter(F(1e30), F(0)), 2]
        q = t * u
        near = (q.view(np.int32)[:, None] + steps[None, :]).astype(np.int32).view(F)
        rel = (q[:, None].astype(np.float64) * (1 + rng.uniform(-3e-6, 3e-6, (len(u), 60)))).astype(F)
        inter = np.concatenate([near, rel], axis=1)
        uu = np.broadcast_to(u[:, None], inter.shape)
        with np.errstate(all="ignore"):
            v = inter / uu
        decided, hit, sane = R.shortcut(inter, uu, t)
        assert sane.all() and decided.any() and not decided.all()
        assert np.array_equal(hit[decided], (v > t)[decided]) and np.array_equal(hit[decided], (v >= t)[decided]), float(t)


def test_a_wave_of_the_mixed_tables_holds_decided_and_undecided_lanes():
    """64 consecutive rows against one column of a later block: the wave divides for some lanes and not for others."""
    seen = {}
    for lst in R.mixed_lists():
        pos, sa = lst.pos, R.area(lst.pos)
        found = False
        for rb in range(lst.n // R.W64 - 1):
            rows = slice(rb * R.W64, (rb + 1) * R.W64)
            for j in range((rb + 1) * R.W64, min((rb + 3) * R.W64, lst.n)):
                inter, u, _ = R.pair_terms(pos[rows], sa[rows], pos[j], sa[j])
                decided = R.shortcut(inter, u, lst.t)[0]
                if decided.any() and not decided.all():
                    found = True
                    break
            if found:
                break
        seen[lst.name] = found
    assert all(v for k, v in seen.items() if k.startswith("int700")) and sum(k.startswith("int700") for k in seen) == len(R.TIE_T), seen


# ================================================================================================================ the derived outputs
def test_top_and_proposal_expectations_by_hand():
    kept = np.zeros(200, bool)
    kept[[0, 3, 63, 64, 70, 130, 199]] = True                            # 3 in block 0, 2 in block 1, 1 in block 2, 1 in block 3
    assert R.top_expect(kept, 1)[0].tolist() == [0, 3, 63] and R.top_expect(kept, 3)[1] == 0 and R.top_expect(kept, 3)[0].tolist() == [0, 3, 63]
    assert R.top_expect(kept, 4)[1] == 1 and R.top_expect(kept, 5)[0].tolist() == [0, 3, 63, 64, 70] and R.top_expect(kept, 6)[1] == 2
    assert R.top_expect(kept, 8)[1] == 3 and len(R.top_expect(kept, 1 << 31)[0]) == 7 == len(R.top_expect(kept, 0)[0])
    boxes = np.arange(800, dtype=F).reshape(200, 4)
    order = np.arange(200, dtype=I64)[::-1].copy()
    rows, k = R.proposal_expect(boxes, order, kept, 3)
    assert k == 3 and rows.tolist() == boxes[[199, 196, 136]].tolist()
    rows, k = R.proposal_expect(boxes, order, kept, 9)
    assert k == 7 and not rows[7:].any() and rows[6].tolist() == boxes[0].tolist()
    assert R.plain_expect(order, kept).tolist() == sorted(199 - np.flatnonzero(kept))
    lst = R.chain_lattice(R.RPN_N)
    assert all(m > 0 for m in R.top_cases(lst)) and len(R.top_cases(lst)) >= 8
    assert len({l.kept(0).sum() for l in R.batch_lists(R.RPN_N)}) == 5 and all(l.n == R.RPN_N for l in R.batch_lists(R.RPN_N))
    b, o = R.deal(R.disjoint(65), perm=True, extra=7)
    assert len(b) == len(o) == 72 and sorted(o.tolist()) == list(range(72)) and (o != np.arange(72)).all()
    assert np.array_equal(b[o][:65], R.disjoint(65).pos)
