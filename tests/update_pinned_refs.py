"""References of the kernels that write the model's state on every step: the PGD sign step, noise, clamp, cast and start of
csrc/afan_pgd.hip, the SGD update and the guarded copy of csrc/afan_sgd.hip, and the KRSC -> CRSK weight transpose at the end of
csrc/afan_conv.hip.  tests/test_update_pinned_gpu.py holds every kernel form to them BIT FOR BIT; tests/test_update_pinned_ref.py
checks them on the CPU against the C oracle and torch.

Every arithmetic step of these kernels is one correctly rounded fp32 operation (-ffp-contract=off) or a copy, so the references
restate each operation with np.float32 arithmetic, one numpy operation per rounding (never float64 rounded afterwards: that rounds
twice).  bf16 values are uint16 bit patterns throughout.  The norms reuse tail_pinned_refs.perturb_norms.

The host-side dispatch is restated below (the alignment rules that choose the vector kernels, grid_for and its cap, NORM_CHUNK, the
tile count of the transpose) with the sources' constants named, and the *_tags functions map a table row of the GPU module to the
instantiations and inner paths it reaches, so that the GPU tables and the CPU coverage test share one statement of it.  Alignment
is given as byte offsets from a 256-byte-aligned base.
"""
import numpy as np

from tail_pinned_refs import NORM_CHUNK, perturb_norms  # noqa: F401  (the norms reference and its chunk are shared, not restated)

F = np.float32

# ---- constants of csrc/afan_common.h, afan_pgd.hip, afan_sgd.hip, afan_conv.hip ---------------------------------------------------
BLOCK = 256
WAVE = 64
GRID_CAP = 256 * 8                  # grid_for's default max_blocks
MAX_BATCH = 65535                   # gridDim.y of the norms kernels
TILE = 64                           # transpose_weights_kernel: 64 (k) x 64 (c) per workgroup
AFAN_OK, AFAN_EDTYPE, AFAN_EALIGN, AFAN_ESHAPE, AFAN_ENULL = 0, -1, -2, -3, -4

# ---- the smallest sizes whose grid-stride loops make a second trip ------------------------------------------------------------------
T4 = 4 * GRID_CAP * BLOCK + 4 * BLOCK * 3 + 3       # float4 paths: 768 threads make two trips, the others one; 3 ragged elements
T8 = 8 * GRID_CAP * BLOCK + 8 * 100 + 5             # 8-wide paths: 100 threads make two trips; 5 ragged elements
T1 = GRID_CAP * BLOCK + 777                         # scalar paths
SMALL_N = (1, 3, 4, 5, 7, 8, 9, 63, 64, 257)


# ================================================================================================================ dispatch, restated
def grid_for(work_items, block=BLOCK, max_blocks=GRID_CAP):
    return int(max(1, min(max_blocks, -(-work_items // block))))


def loop_trips(n, vec, width):
    """Trips of the busiest thread through the main grid-stride loop: the vector body handles n // width items, grid_for is given
    ceil(n / width); the scalar loop handles n."""
    work = n // width if vec else n
    grid = grid_for(-(-n // width) if vec else n)
    return -(-work // (grid * BLOCK))


def step_scalar_terms(g_bytes, clip, shadow, o):
    """launch_step: the operands (of x_adv, grad, x_clean, shadow at byte offsets o) whose alignment refuses the float4 kernel."""
    xa, g, xc, sh = o
    out = []
    if xa % 16:
        out.append("x_adv")
    if g % (4 * g_bytes):
        out.append("grad")
    if clip and xc % 16:
        out.append("x_clean")
    if shadow and sh % 8:
        out.append("shadow")
    return out


def step_norms_scalar_terms(g_bytes, shadow, per_sample, o):
    """launch_step_norms<STEP = true>: x_clean is read with or without the projection."""
    xa, g, xc, sh = o
    out = []
    if per_sample % 4:
        out.append("per%4")
    if xa % 16:
        out.append("x_adv")
    if xc % 16:
        out.append("x_clean")
    if g % (4 * g_bytes):
        out.append("grad")
    if shadow and sh % 8:
        out.append("shadow")
    return out


def norms_vec(per_sample, xa_off, xc_off):
    """launch_step_norms<STEP = false> (afan_perturb_norms)."""
    return per_sample % 4 == 0 and xa_off % 16 == 0 and xc_off % 16 == 0


def norm_slices(per_sample):
    return -(-per_sample // NORM_CHUNK)


def norms_workspace_floats(batch, per_sample):
    return 0 if batch <= 0 or per_sample <= 0 else 2 * batch * norm_slices(per_sample)


def noise_vec(shadow, o):
    xa, u, sh = o
    return xa % 16 == 0 and u % 16 == 0 and (not shadow or sh % 8 == 0)


def sgd_vec(shadow, o):
    p, g, m, sh = o
    return p % 16 == 0 and g % 16 == 0 and m % 16 == 0 and (not shadow or sh % 8 == 0)


def cast_vec(o):
    src, dst = o
    return src % 16 == 0 and dst % 16 == 0


def init_scalar_terms(x32, shadow, o):
    x, x32o, xa, sh = o
    out = []
    if x % 16:
        out.append("x")
    if xa % 16:
        out.append("x_adv")
    if x32 and x32o % 16:
        out.append("x32")
    if shadow and sh % 16:
        out.append("shadow")
    return out


def transpose_tiles(k, rs, c):
    return -(-k // TILE) * rs * -(-c // TILE)


def make_descs(rows):
    """rows of (src_off, dst_off, K, RS, C, dst_RS, rs0) -> (int64 [n, 8] descriptors with the running first_tile, total_tiles)."""
    out, tiles = [], 0
    for so, do, k, rs, c, drs, rs0 in rows:
        out.append([so, do, k, rs, c, tiles, drs, rs0])
        tiles += transpose_tiles(k, rs, c)
    return np.array(out, np.int64).reshape(-1, 8), tiles


# ----------------------------------------------------------------------------------------------------------------------- variant tags
def _trip(n, vec, width):
    return {f"trip2|{'vec' if vec else 'scalar'}"} if loop_trips(n, vec, width) > 1 else set()


def step_tags(g_name, g_bytes, clip, shadow, n, o, x_clean_null=False, eps0=False):
    why = step_scalar_terms(g_bytes, clip, shadow, o)
    vec = not why
    out = {f"pgd_step<{g_name},{'clip' if clip else 'noclip'},{'shadow' if shadow else 'noshadow'},{'vec' if vec else 'scalar'}>"}
    out |= {f"pgd_step|{t}" for t in _trip(n, vec, 4)}
    if vec and n % 4:
        out.add("pgd_step|ragged_tail")
    if len(why) == 1:
        out.add(f"pgd_step|scalar_by|{why[0]}")
    if x_clean_null:
        out.add("pgd_step|x_clean_null")
    if eps0:
        out.add("pgd_step|eps0")
    return out


def step_norms_tags(g_name, g_bytes, clip, shadow, batch, per, o, nan_sample=False):
    if batch > MAX_BATCH:
        return {"step_norms|batch_refused"}
    why = step_norms_scalar_terms(g_bytes, shadow, per, o)
    vec = not why
    v = "vec" if vec else "scalar"
    out = {f"step_norms<{g_name},{'clip' if clip else 'noclip'},{'shadow' if shadow else 'noshadow'},{v}>"}
    slices = norm_slices(per)
    if slices > 1:
        out.add(f"step_norms|multi_slice|{v}")
        if per % NORM_CHUNK:
            out.add(f"step_norms|ragged_slice|{v}")
    if slices > WAVE:
        out.add(f"step_norms|finalize_trip2|{v}")
    if per < BLOCK * (4 if vec else 1):
        out.add(f"step_norms|idle_threads|{v}")
    if batch == MAX_BATCH:
        out.add(f"step_norms|batch_limit|{v}")
    if len(why) == 1:
        out.add(f"step_norms|scalar_by|{why[0]}")
    if nan_sample:
        out.add(f"step_norms|nan_sample|{v}")
    return out


def noise_tags(shadow, n, o):
    vec = noise_vec(shadow, o)
    out = {f"noise<{'vec' if vec else 'scalar'}>|{'shadow' if shadow else 'noshadow'}"}
    out |= {f"noise|{t}" for t in _trip(n, vec, 4)}
    if vec and n % 4:
        out.add("noise|ragged_tail")
    return out


def clamp_tags(n):
    return {"clamp"} | {f"clamp|{t}" for t in _trip(n, False, 1)}


def cast_tags(n, o):
    vec = cast_vec(o)
    out = {f"cast<{'vec' if vec else 'scalar'}>"} | {f"cast|{t}" for t in _trip(n, vec, 8)}
    if vec and n % 8:
        out.add("cast|ragged_tail")
    return out


def init_tags(src_name, x32, shadow, n, o):
    if src_name == "bf16" and not x32:
        return {"init|x32_null|bf16_refused"}
    why = init_scalar_terms(x32, shadow, o)
    vec = not why
    out = {f"init<{src_name},{'vec' if vec else 'scalar'}>|{'shadow' if shadow else 'noshadow'}"}
    out |= {f"init|{t}" for t in _trip(n, vec, 8)}
    if vec and n % 8:
        out.add("init|ragged_tail")
    if not x32:
        out.add(f"init|x32_null|{'vec' if vec else 'scalar'}")
    if why == ["shadow"]:
        out.add("init|scalar_by|shadow")
    return out


def sgd_tags(first, shadow, n, o, kind=""):
    vec = sgd_vec(shadow, o)
    out = {f"sgd<{'first' if first else 'later'},{'shadow' if shadow else 'noshadow'}>|{'vec' if vec else 'scalar'}"}
    out |= {f"sgd|{t}" for t in _trip(n, vec, 4)}
    if vec and n % 4:
        out.add("sgd|ragged_tail")
    if kind:
        out.add(f"sgd|{kind}")
        if kind == "guard_set" and loop_trips(n, vec, 4) > 1:
            out.add("sgd|guard_set|trip2")
    return out


def copy_tags(nbytes):
    return {"copy"} | {f"copy|{t}" for t in _trip(nbytes // 16, False, 1)}


def transpose_tags(rows):
    """rows as make_descs takes them."""
    out = set()
    for so, do, k, rs, c, drs, rs0 in rows:
        if k % TILE:
            out.add("transpose|partial_k_tile")
        if c % TILE:
            out.add("transpose|partial_c_tile")
        if k > TILE:
            out.add("transpose|multi_k_tile")
        if c > TILE:
            out.add("transpose|multi_c_tile")
        if k % TILE == 0 and c % TILE == 0:
            out.add("transpose|full_tiles")
        if rs > 1:
            out.add("transpose|rs>1")
        if drs != rs:
            out.add("transpose|shared_operand|rs0=%d" % rs0)
    if len(rows) > 1:
        out.add("transpose|multi_desc")
    dsts = [r[1] for r in rows]
    if len(rows) == 1 and rows[0][5] > rows[0][3]:
        out.add("transpose|slot_left_alone")
    if dsts != sorted(dsts) or [r[0] for r in rows] != sorted(r[0] for r in rows):
        out.add("transpose|offsets_out_of_order")
    return out


# ======================================================================================================================== bit patterns
def bf16_is_nan(b):
    return (np.asarray(b, np.uint16) & 0x7fff) > 0x7f80


def bf16_bits(x):
    """fp32 array -> the uint16 patterns of its round-to-nearest-even bf16 (the largest finite fp32 rounds to infinity; a NaN stays a
    NaN, its payload is not pinned)."""
    x = np.ascontiguousarray(x, F)
    bits = x.view(np.uint32).astype(np.uint64)
    r = ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), ((bits >> 16) | 0x40).astype(np.uint16), r)


def bf16_widen(b):
    """uint16 bf16 patterns -> their fp32 values (exact)."""
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(F)


def same_f32(got, want):
    """Index of the first element whose fp32 bits differ (any NaN equals any NaN), or None."""
    got, want = np.ascontiguousarray(got, F).ravel(), np.ascontiguousarray(want, F).ravel()
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & (got.view(np.uint32) != want.view(np.uint32)))
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


def same_bf16(got, want):
    got, want = np.ascontiguousarray(got, np.uint16).ravel(), np.ascontiguousarray(want, np.uint16).ravel()
    gn, wn = bf16_is_nan(got), bf16_is_nan(want)
    bad = (gn != wn) | (~gn & (got != want))
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


# ========================================================================================================================= references
def _f(a):
    a = np.asarray(a)
    assert a.dtype == F, a.dtype
    return a


def sign(g):
    """torch.sign: sign(+-0) = 0, sign(NaN) = NaN."""
    g = _f(g)
    with np.errstate(invalid="ignore"):
        s = (g > 0).astype(F) - (g < 0).astype(F)
    return _f(np.where(np.isnan(g), g, s))


def clamp(t, lo, hi):
    """The attack's tensor_clamp: `if t < lo: t = lo`, then `if t > hi: t = hi` (the order decides when lo > hi; a NaN, in t or in
    a bound, compares false and leaves t as it is)."""
    with np.errstate(invalid="ignore"):
        t = np.where(_f(t) < _f(lo), lo, t)
        t = np.where(t > _f(hi), hi, t)
    return _f(t)


def pgd_step(x_adv, grad, x_clean, gamma, eps, clip):
    """x_adv + gamma * sign(grad) (one rounding: the product is exact), projected onto [x_clean - eps, x_clean + eps] (both bounds
    rounded first) when clip.  grad as fp32 values (a bf16 gradient widened)."""
    gamma, eps = F(gamma), F(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        d = _f(gamma * sign(grad))
        t = _f(_f(x_adv) + d)
        if clip:
            lo = _f(_f(x_clean) - eps)
            hi = _f(_f(x_clean) + eps)
            t = clamp(t, lo, hi)
    return t


def axpy_noise(x_adv, u, eps):
    t = _f(F(2) * _f(u))
    t = _f(t - F(1))
    t = _f(t * F(eps))
    return _f(_f(x_adv) + t)


def sgd_step(p, g, m, lr, mom, wd, gscale, first):
    """torch.optim.SGD (dampening 0, no nesterov) -> (p, m)."""
    lr, mom, wd, gscale = F(lr), F(mom), F(wd), F(gscale)
    gg = _f(_f(g) * gscale)
    gg = _f(gg + _f(wd * _f(p)))
    m = gg if first else _f(_f(_f(m) * mom) + gg)
    p = _f(p - _f(lr * m))
    return p, m


def transpose_weights(src, dst, descs):
    """Each descriptor {src_off, dst_off, K, RS, C, first_tile, dst_RS, rs0}: src[src_off:] as [K][RS][C] lands in dst[dst_off:] as
    [C][dst_RS][K], taps in slots rs0 .. rs0 + RS - 1.  uint16 patterns; dst (pre-filled by the caller) is written in place."""
    assert src.dtype == np.uint16 and dst.dtype == np.uint16
    for so, do, k, rs, c, _, drs, rs0 in np.asarray(descs, np.int64).reshape(-1, 8).tolist():
        s = src[so:so + k * rs * c].reshape(k, rs, c)
        d = dst[do:do + c * drs * k].reshape(c, drs, k)
        d[:, rs0:rs0 + rs, :] = s.transpose(2, 1, 0)
    return dst
