"""The packed PGD loop's arithmetic on the CPU: pgd_packed_refs' pack and replay against the plain chain of update_pinned_refs.pgd_step,
bit for bit (any NaN equals any NaN), K = 1..5, clip off and on, with zero, -0.0, NaN and +-inf gradients and starts of -0.0, 1e-30,
3e4 and 1e6.  The GPU module holds the kernels to the same functions."""
import numpy as np
import pytest

import pgd_packed_refs as P
import update_pinned_refs as R


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5])
def test_pack_and_replay_equal_the_plain_chain(steps, clip):
    n = 997
    x0, grads = P.inputs(n, steps, seed=steps)
    want = P.chain(x0, grads, P.GAMMA, P.EPS, clip)
    codes = None
    for t in range(steps):
        # what the next launch would rebuild from the bytes alone
        if t > 0:
            assert R.same_f32(P.replay(x0, codes, t, P.GAMMA, P.EPS, clip), want[t - 1]) is None, f"replay before step {t}"
        new, shadow, xa = P.packed_step(x0, grads[t], codes, min(t, P.MAX_CODES), P.GAMMA, P.EPS, clip)
        assert R.same_f32(xa, want[t]) is None, f"iterate after step {t}"
        assert R.same_bf16(shadow, R.bf16_bits(want[t])) is None, f"shadow after step {t}"
        if t < P.MAX_CODES:
            assert np.array_equal(new >> (2 * t), P.code_of(grads[t])), "step t's code, nothing above it"
            if t > 0:
                assert np.array_equal(new & ((1 << (2 * t)) - 1), codes & ((1 << (2 * t)) - 1)), "the earlier codes are kept"
            codes = new


def test_the_inputs_hold_the_special_values():
    x0, grads = P.inputs(997, 5, seed=0)
    xc = R.bf16_widen(x0)
    assert np.signbit(xc[xc == 0]).any() and (xc == R.bf16_widen(R.bf16_bits(np.array([1e-30], R.F)))[0]).any()
    assert (xc > 2.9e4).any() and (xc >= 9e5).any()
    for g in grads:
        assert np.isnan(g).any() and np.isposinf(g).any() and np.isneginf(g).any()
        assert (g == 0).any() and np.signbit(g[g == 0]).any()
    # every code occurs at an element whose start is -0.0: the case where `xa + gamma * 0.f` matters
    c = P.code_of(grads[0])[np.signbit(xc) & (xc == 0)]
    assert set(c.tolist()) == {0, 1, 2, 3}


def test_special_cases_by_hand():
    g, e = P.GAMMA, P.EPS
    x0 = R.bf16_bits(np.array([-0.0, -0.0, 1e6, 1.0, 1.0], R.F))
    grad = np.array([0.0, np.nan, 1.0, np.inf, -np.inf], R.F)
    codes, _, xa = P.packed_step(x0, grad, None, 0, g, e, False)
    assert codes.tolist() == [0, 3, 1, 1, 2]
    assert xa[0] == 0 and not np.signbit(xa[0]), "-0 + gamma * 0 = +0, as the plain kernel evaluates it"
    assert np.isnan(xa[1]) and xa[2] == R.bf16_widen(x0)[2] > 9e5, "+gamma is absorbed at 1e6"
    # a NaN decision stays: the next step's replay is NaN whatever the new gradient says
    _, _, xb = P.packed_step(x0, np.ones(5, R.F), codes, 1, g, e, True)
    assert np.isnan(xb[1]) and xb[3] == R.F(R.F(1.0) + g) + g
    # five steps up with clip: the fifth lands on the rounded upper bound
    c, xs = None, None
    for t in range(5):
        c, _, xs = P.packed_step(x0, np.ones(5, R.F), c, min(t, 4), g, e, True)
    assert xs[3] == R.F(R.F(1.0) + e)
