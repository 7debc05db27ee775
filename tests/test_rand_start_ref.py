"""The device random start's generator, without a GPU: a numpy Philox4x32-10 written from the Random123 definition (Salmon, Moraes,
Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11 — multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
0xBB67AE85, ten rounds), checked against the published known-answer vectors; the word -> u mapping of afan_pgd_rand_start; and the
entry point's argument errors with host pointers (nothing is launched).  tests/test_rand_start_gpu.py imports the reference from here."""
import ctypes

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
LCG_A, LCG_C = 6364136223846793005, 1442695040888963407


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two -> four uint64 arrays holding the 32-bit output words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    k = [int(v) & MASK for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & np.uint64(MASK)]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def word_to_u(word):
    """u = (word >> 8) * 2^-24: 24 bits, exact in fp32, in [0, 1)."""
    return ((np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def uniform(seed, shape):
    """afan_pgd_rand_start's u for a tensor of logical (NCHW, row-major) `shape`, as float32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    total = int(np.prod(shape))
    e = np.arange(total, dtype=np.uint64)
    q = e >> np.uint64(2)
    zero = np.zeros_like(q)
    words = np.stack(philox4x32_10((q & np.uint64(MASK), q >> np.uint64(32), zero, zero), (seed & MASK, seed >> 32)), axis=1)
    return word_to_u(words[np.arange(total), (e & np.uint64(3)).astype(np.int64)]).reshape(shape)


def lcg(seed):
    """The generator's step (afan_dropout's): s * 6364136223846793005 + 1442695040888963407 mod 2^64, as a signed int64 value."""
    v = (int(seed) % 2 ** 64 * LCG_A + LCG_C) % 2 ** 64
    return v - 2 ** 64 if v >= 2 ** 63 else v


def test_known_answer_vectors():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    pi = ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])
    for (ctr, key), want in ((([0, 0, 0, 0], [0, 0]), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                             (([MASK] * 4, [MASK] * 2), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                             (pi, [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        got = [int(v) for v in philox4x32_10(ctr, key)]
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])


def test_vectorised_equals_scalar():
    seed = 0x0123456789ABCDEF
    u = uniform(seed, (11,))
    for e in (0, 3, 4, 10):
        w = philox4x32_10((e >> 2, 0, 0, 0), (seed & MASK, seed >> 32))[e & 3]
        assert u[e] == word_to_u(w)


def test_u_mapping_at_the_ends():
    u0, u1 = word_to_u(0), word_to_u(0xFFFFFFFF)
    assert u0.dtype == np.float32 and u0 == 0.0
    assert u1 == np.float32(1.0 - 2.0 ** -24) and u1 < 1.0
    assert word_to_u(0xFF) == 0.0 and word_to_u(0x100) == np.float32(2.0 ** -24)       # the low 8 bits are dropped
    # the start's end points stay inside the ball: fl(fl(2u) - 1) lies in [-1, 1 - 2^-23], both roundings exact
    for u, want in ((u0, -1.0), (u1, 1.0 - 2.0 ** -23)):
        assert np.float32(np.float32(2.0) * u) - np.float32(1.0) == np.float32(want)


def test_generator_step():
    assert lcg(0) == LCG_C and lcg(1) == LCG_A + LCG_C                     # (below 2^63: no wrap yet)
    assert -2 ** 63 <= lcg(2 ** 62 + 12345) < 2 ** 63


def test_argument_errors_without_gpu(pkg):
    lib = pkg._lib.load()
    f = lib.afan_pgd_rand_start
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) // 16 * 16)                     # 16-byte aligned inside the buffer
    odd = ctypes.c_void_p(p.value + 4)                              # float-aligned, not 16-byte aligned
    ok = [p, p, None, 1, 1, 1, 4, 0, 0.1, p, p, 1, None]
    assert f(None, None, None, 0, 1, 1, 1, 0, 0.1, None, None, 1, None) == 0          # n == 0: no launch
    assert f(None, None, None, 4, 3, 0, 5, 1, 0.1, None, None, 1, None) == 0          # an empty tensor
    for k in (3, 4, 5, 6):
        a = list(ok)
        a[k] = -1
        assert f(*a) == -3, k                                                          # AFAN_ESHAPE: a negative size
    for layout in (2, -1):
        a = list(ok)
        a[7] = layout
        assert f(*a) == -3, layout                                                     # AFAN_ESHAPE: an unknown layout
    for k in (0, 1, 9):
        a = list(ok)
        a[k] = None
        assert f(*a) == -4, k                                                          # AFAN_ENULL: x, x_adv, state
    for k in (0, 1, 2):
        a = list(ok)
        a[k] = odd
        assert f(*a) == -2, k                                                          # AFAN_EALIGN: x, x_adv, shadow
    assert "afan_pgd_rand_start" in pkg._lib.SIGNATURES and callable(pkg.ops.pgd_rand_start) and callable(pkg.ops.noise_state)
