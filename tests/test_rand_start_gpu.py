"""afan_pgd_rand_start on the GPU against the numpy Philox4x32-10 of tests/test_rand_start_ref.py, through the kernel it replaces: the
reference u is uploaded, ops.axpy_noise_ is applied to a clone of x, and ops.pgd_rand_start's output must equal that bit for bit.
Not tested: element indices at or above 2^32 (the counter's second word, the 64-bit channels-last decomposition) — such a tensor and
its output need 16 GB each way."""
import numpy as np
import pytest
import torch

import test_rand_start_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 / 255
SEED = 0x1234_5678_9ABC_DEF1          # bits above 2^32 set: both key words are in play


def _state(gpu, seed):
    return torch.tensor([seed], dtype=torch.int64, device=gpu)


def _x(shape, gpu, channels_last=False, seed=0):
    x = torch.from_numpy(np.random.default_rng(seed).random(shape, dtype=np.float32)).to(gpu)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


def _expected(pkg, x, seed, eps):
    """x + (2u - 1) eps through afan_axpy_noise, u from the numpy reference in x's logical (NCHW) order."""
    u = torch.from_numpy(R.uniform(seed, tuple(x.shape))).to(x.device)
    return pkg.ops.axpy_noise_(x.clone(), u, eps)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape", [(1,), (3,), (4,), (5,), (2, 3, 5, 7), (1, 1, 1, 65539)], ids=str)
def test_equals_the_reference_draw_through_axpy_noise(pkg, gpu, shape):
    x, st = _x(shape, gpu), _state(gpu, SEED)
    got, used = pkg.ops.pgd_rand_start(x, EPS, state=st)
    want = _expected(pkg, x, SEED, EPS)
    d = (got - x).abs()
    print(f"{shape}: max |x_adv - x| = {float(d.max()):.9g} (eps {EPS:.9g}), differing elements {int((got != want).sum())}")
    assert got.shape == x.shape and got.stride() == x.stride() and got.data_ptr() != x.data_ptr()
    assert _same_bits(got, want)
    # |fl((2u - 1) eps)| <= eps holds exactly; the one add could carry an element half an ulp of x_adv past it, which none of
    # these fixed inputs does (the numpy reference gives the same maxima as printed above)
    assert bool((d <= EPS).all())
    assert int(used) == SEED and int(st) == R.lcg(SEED)
    if x.numel() > 8:
        assert float(d.max()) > 0.5 * EPS and len(torch.unique(got - x)) > x.numel() // 2      # a draw, not a constant


def test_channels_last_receives_its_nchw_twins_numbers(pkg, gpu):
    x = _x((2, 3, 5, 7), gpu)
    xl = x.contiguous(memory_format=torch.channels_last)
    a, _ = pkg.ops.pgd_rand_start(x, EPS, state=_state(gpu, SEED))
    b, _ = pkg.ops.pgd_rand_start(xl, EPS, state=_state(gpu, SEED))
    assert b.is_contiguous(memory_format=torch.channels_last) and not b.is_contiguous()
    assert _same_bits(a, b.contiguous()) and _same_bits(b.contiguous(), _expected(pkg, x, SEED, EPS))
    # ragged in memory order too: 3 x 3 x 3 x 3 = 81 elements, the last lane owns one
    y = _x((3, 3, 3, 3), gpu, channels_last=True, seed=1)
    c, _ = pkg.ops.pgd_rand_start(y, EPS, state=_state(gpu, 7))
    assert _same_bits(c.contiguous(), _expected(pkg, y.contiguous(), 7, EPS))


@pytest.mark.parametrize("channels_last", [False, True])
def test_shadow_is_the_rne_bf16_of_the_result(pkg, gpu, channels_last):
    x = _x((2, 3, 5, 7), gpu, channels_last)
    shadow = torch.empty_like(x, dtype=torch.bfloat16)
    got, _ = pkg.ops.pgd_rand_start(x, EPS, shadow=shadow, state=_state(gpu, SEED))
    assert _same_bits(got.contiguous(), _expected(pkg, x.contiguous(), SEED, EPS))
    assert torch.equal(shadow.view(torch.int16), got.to(torch.bfloat16).view(torch.int16))     # torch's cast rounds to nearest even
    tail = _x((5,), gpu)                                                # the scalar tail writes the shadow too
    sh = torch.empty(5, dtype=torch.bfloat16, device=gpu)
    g, _ = pkg.ops.pgd_rand_start(tail, EPS, shadow=sh, state=_state(gpu, SEED))
    assert torch.equal(sh.view(torch.int16), g.to(torch.bfloat16).view(torch.int16))


def test_eps_zero_returns_x(pkg, gpu):
    x = _x((2, 3, 5, 7), gpu)
    got, _ = pkg.ops.pgd_rand_start(x, 0.0, state=_state(gpu, SEED))
    assert _same_bits(got, x)


def test_state_and_used(pkg, gpu):
    x = _x((9,), gpu)
    st = _state(gpu, SEED)
    a, used = pkg.ops.pgd_rand_start(x, EPS, state=st, advance=False)
    assert int(used) == SEED and int(st) == SEED                        # unchanged without advance
    b, used = pkg.ops.pgd_rand_start(x, EPS, state=st, advance=True)
    assert int(used) == SEED and int(st) == R.lcg(SEED) and _same_bits(a, b)
    c, used = pkg.ops.pgd_rand_start(x, EPS, state=st)
    assert int(used) == R.lcg(SEED) and int(st) == R.lcg(R.lcg(SEED)) and not _same_bits(b, c)
    assert _same_bits(c, _expected(pkg, x, R.lcg(SEED), EPS))           # (a negative int64 word: the kernel reads it as uint64)
    # the default generator is the device's noise word, not dropout's
    ns, ds = pkg.ops.noise_state(gpu), pkg.ops.dropout_state(gpu)
    assert ns.data_ptr() != ds.data_ptr() and ns.dtype == torch.int64 and ns.numel() == 1
    n0, d0 = int(ns), int(ds)
    _, used = pkg.ops.pgd_rand_start(x, EPS)
    assert int(used) == n0 and int(ns) == R.lcg(n0) and int(ds) == d0   # the dropout stream did not move


def test_wrapper_checks(pkg, gpu):
    x = _x((2, 3, 5, 7), gpu)
    with pytest.raises(TypeError):
        pkg.ops.pgd_rand_start(x.to(torch.bfloat16), EPS)
    with pytest.raises(ValueError):
        pkg.ops.pgd_rand_start(x, EPS, shadow=torch.empty_like(x, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last))
    with pytest.raises(pkg.AfanLibraryError):
        pkg.ops.pgd_rand_start(x.cpu(), EPS)


def test_a_replayed_graph_draws_fresh_numbers(pkg, gpu):
    x = _x((2, 3, 5, 7), gpu)
    st = _state(gpu, SEED)
    eager, seeds = [], []
    for _ in range(3):
        o, used = pkg.ops.pgd_rand_start(x, EPS, state=st)
        eager.append(o.clone())
        seeds.append(int(used))
    assert seeds == [SEED, R.lcg(SEED), R.lcg(R.lcg(SEED))]
    st.fill_(SEED)
    torch.cuda.synchronize()
    g, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            out, used = pkg.ops.pgd_rand_start(x, EPS, state=st)
    assert int(st) == SEED                                              # capture launches nothing
    replays = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
        assert int(used) == seeds[k]
    for k in range(3):
        assert _same_bits(replays[k], eager[k]), k
    assert not any(_same_bits(replays[a], replays[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
