"""CPU checks of what tests/test_bn_pinned_gpu.py rests on: its float64 references against torch.nn.functional.batch_norm and autograd
in double, its exact-sum generator against its own preconditions, and the near-zero-activation share of its Gaussian inputs."""
import pytest
import torch
import torch.nn.functional as F

import test_bn_pinned_gpu as pin


@pytest.mark.parametrize("shape", [(2, 5, 3, 4), (3, 8, 1, 1), (4, 3, 7, 9)])
@pytest.mark.parametrize("res_on,relu", pin.FWD_COMBOS)
def test_references_match_torch_double(shape, res_on, relu):
    g = torch.Generator().manual_seed(sum(shape) + 2 * res_on + relu)
    c = shape[1]
    m = shape[0] * shape[2] * shape[3]
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 1.5 + 0.7).requires_grad_(True)
    r = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_(True) if res_on else None
    w = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    b = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_(True)
    rm0, rv0 = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    eps, mom = 1e-3, 0.3
    rm, rv = rm0.clone(), rv0.clone()
    y = F.batch_norm(x, rm, rv, w, b, True, mom, eps)
    if res_on:
        y = y + r
    if relu:
        y = torch.relu(y)
    y.backward(dy)
    # forward, running buffers
    y_ref, mean, var, invstd = pin.ref_bn_forward(x.detach(), w.detach(), b.detach(), eps, r.detach() if res_on else None, relu)
    torch.testing.assert_close(y_ref, y.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(pin.ref_running(rm0, mean, mom), rm, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(pin.ref_running(rv0, var * pin.ref_unbias(m), mom), rv, rtol=1e-12, atol=1e-12)
    two = pin.ref_running(pin.ref_running(rm0, mean, mom), mean, mom)
    torch.testing.assert_close(pin.ref_running(rm0, mean, mom, 2), two, rtol=0, atol=0)
    # backward
    out = pin.ref_bn_backward(dy, x.detach(), mean, invstd, invstd * w.detach(), (y.detach() > 0) if relu else None)
    torch.testing.assert_close(out["dx"], x.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(out["dw"], w.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(out["db"], b.grad, rtol=1e-10, atol=1e-11)
    if res_on:
        assert torch.equal(out["g"], r.grad)
    assert bool((out["s_dx"] >= out["dx"].abs() * (1 - 1e-12)).all())


def test_unbias_is_guarded_at_one_row():
    assert pin.ref_unbias(1) == 1.0 and pin.ref_unbias(2) == 2.0 and pin.ref_unbias(7) == 7.0 / 6.0


def _small(case):
    return case.shape[0] * case.shape[1] * case.shape[2] * case.shape[3] <= 500000


# the table's own cases, unchanged (the generators are seeded by the whole case); the two cap shapes once each
EXACT_CASES = [c for c in pin.FWD_CASES + pin.BWD_CASES if not c.cancel and c.entry not in ("apply", "affine") and
               (_small(c) or c.entry == "train")]


@pytest.mark.parametrize("case", EXACT_CASES, ids=pin.case_id)
def test_exact_generator_meets_its_preconditions(case):
    x, dy, res, mean = pin.exact_inputs(case)
    groups = 2 if case.entry.endswith("_g2") else 1
    ng = case.shape[0] // groups
    for i in range(groups):
        pin.assert_exact_preconditions(x[i * ng:(i + 1) * ng], dy[i * ng:(i + 1) * ng], mean)
    for t in (x, dy, res):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= 4 and bool((t.to(case.dt).double() == t).all())
    if case.shape[1] > 1:
        assert bool((mean[1:] != mean[:-1]).all()), "neighbouring channels share a mean"
    # the non-integer shift of the test-filled accumulators keeps the shifted sums exact in float64
    g = torch.Generator().manual_seed(1)
    sh = pin.snapshot_shift(mean, g, True)
    assert bool((sh != sh.round()).all())
    a, b = pin.shifted_sums(x[:ng], sh)
    m = ng * case.shape[2] * case.shape[3]
    assert bool((a * 64 == (a * 64).round()).all()) and bool((b * 4096 == (b * 4096).round()).all())
    assert bool((sh + a / m == mean).all())
    for ns in (1, 2, 16):
        assert pin.split_exact(b, ns, g).shape == (ns, case.shape[1])


@pytest.mark.parametrize("exact", [False, True], ids=["gauss", "exact"])
@pytest.mark.parametrize("case", [c for c in pin.BWD_CASES if _small(c)], ids=pin.case_id)
def test_inputs_keep_activations_off_zero(case, exact):
    """No activation of the reference lies within 2^-22 * (|x alpha| + |beta|) of zero (far wider than the ulp of beta that an NCHW
    kernel's own beta may differ by): under the 1e-5 share everywhere, and zero for every NCHW case, Gaussian and exact inputs alike."""
    n = pin.near_zero_count(case, exact)
    numel = case.shape[0] * case.shape[1] * case.shape[2] * case.shape[3]
    assert n <= 1e-5 * numel
    if case.layout == pin.NCHW:
        assert n == 0
