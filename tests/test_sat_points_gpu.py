"""afan_sat_points_nhwc / ops.sat_points on the GPU.  The yardstick is the library's own separate launches, which other tests pin to
float64: every output of the one launch is held BIT FOR BIT to them —
  * fp32: ops.lerp_points' interior points, `clean` / `adv` themselves at weights 0 / 1, ops.mix_feature(point, clean) for mixed points
    (the evaluation's reversed order: the point is normalised onto the clean map's statistics);
  * bf16: `.to(torch.bfloat16)` (round to nearest even) of the fp32 output.
Shapes, each a few thousand elements, are the smallest at which a branch of the kernel can go wrong: c in {2, 8, 63, 64, 65} (lane
tails), {512, 513} (KEEP 8 -> 20), {1280, 1281} (the re-read loop beyond 64 * 20 channels); 1, 3 and 37 pixels; an hw == 1 NCHW tensor;
4 * 8192 + 5 pixels of 8 channels (past the grid cap: the wave-stride loop).  Inputs are Gaussian around a positive per-pixel offset,
post-ReLU-like, so that mean and spread are of one order."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TABLE = [(j, m) for j in range(5) for m in (False, True)]


def _maps(gpu, n, c, h, w, seed, channels_last=True):
    g = torch.Generator().manual_seed(seed)
    off = torch.rand(n, 1, h, w, generator=g) + 0.5
    clean = torch.relu(off + 0.5 * torch.randn(n, c, h, w, generator=g))
    adv = clean + (2.0 / 255) * torch.sign(torch.randn(n, c, h, w, generator=g)) * torch.rand(n, c, h, w, generator=g)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    return clean.to(gpu).contiguous(memory_format=fmt), adv.to(gpu).contiguous(memory_format=fmt)


def _expected(pkg, clean, adv, settings):
    """The separate launches: lerp_points, then mix_feature(point, clean)."""
    pts = [clean] + pkg.ops.lerp_points(clean, adv, 5) + [adv]
    return [pkg.ops.mix_feature(pts[j], clean) if m else pts[j] for j, m in settings]


def _check(pkg, clean, adv, settings):
    weights, mix = [j * (1.0 / 4) for j, _ in settings], [m for _, m in settings]
    want = _expected(pkg, clean, adv, settings)
    before = pkg.ops.CALLS["sat_points"]
    got = pkg.ops.sat_points(clean, adv, weights, mix)
    assert pkg.ops.CALLS["sat_points"] == before + 1
    assert len(got) == len(settings)
    for (j, m), g, w in zip(settings, got, want):
        assert g.dtype == torch.float32 and g.shape == clean.shape and g.stride() == clean.stride()
        assert torch.equal(g, w), f"point {j} mix {m}: max |new - separate| = {float((g - w).abs().max()):.3e}"
    half = pkg.ops.sat_points(clean, adv, weights, mix, out_dtype=torch.bfloat16)
    assert pkg.ops.CALLS["sat_points"] == before + 2
    for g, h in zip(got, half):
        assert h.dtype == torch.bfloat16 and h.stride() == clean.stride() and torch.equal(h, g.to(torch.bfloat16))
    return got


@pytest.mark.parametrize("c", [2, 8, 63, 64, 65, 512, 513, 1280, 1281])
@pytest.mark.parametrize("pixels", [1, 3, 37])
def test_all_ten_outputs_equal_the_separate_launches(pkg, gpu, c, pixels):
    h, w = {1: (1, 1), 3: (1, 3), 37: (37, 1)}[pixels]
    clean, adv = _maps(gpu, 1, c, h, w, seed=c * 100 + pixels)
    _check(pkg, clean, adv, TABLE)


def test_batch_of_two_and_a_single_output(pkg, gpu):
    clean, adv = _maps(gpu, 2, 65, 3, 5, seed=7)
    got = _check(pkg, clean, adv, TABLE)
    block = pkg.ops.sat_points_block(clean, adv, [j * 0.25 for j, _ in TABLE], [m for _, m in TABLE])
    assert block.shape == (20, 65, 3, 5) and block.is_contiguous(memory_format=torch.channels_last)
    for k, g in enumerate(got):
        assert torch.equal(block[2 * k:2 * k + 2], g)
    for s in [(0, False), (2, False), (3, True), (4, True)]:
        _check(pkg, clean, adv, [s])
    # the same weight twice with different mask bits
    _check(pkg, clean, adv, [(1, True), (1, False), (4, False), (0, True)])


def test_hw_one_nchw(pkg, gpu):
    clean, adv = _maps(gpu, 5, 513, 1, 1, seed=9, channels_last=False)
    assert clean.is_contiguous()
    _check(pkg, clean, adv, TABLE)


def test_past_the_grid_cap(pkg, gpu):
    pixels = 4 * 8192 + 5
    clean, adv = _maps(gpu, 1, 8, pixels, 1, seed=13)
    _check(pkg, clean, adv, TABLE)


def test_the_mix_order_is_the_reversed_one(pkg, gpu):
    clean, adv = _maps(gpu, 1, 64, 3, 3, seed=21)
    (mixed, point) = pkg.ops.sat_points(clean, adv, [1.0, 1.0], [True, False])
    assert torch.equal(point, adv)
    assert torch.equal(mixed, pkg.ops.mix_feature(adv, clean)) and not torch.equal(mixed, pkg.ops.mix_feature(clean, adv))
    # per pixel the mixed point carries the CLEAN map's channel statistics
    assert float((mixed.mean(dim=1) - clean.mean(dim=1)).abs().max()) < 1e-5
    assert float((mixed.var(dim=1) - clean.var(dim=1)).abs().max()) < 1e-4
    assert float((mixed - point).abs().max()) > 1e-4


def test_nchw_composes_the_existing_launches(pkg, gpu):
    clean, adv = _maps(gpu, 2, 16, 4, 5, seed=23, channels_last=False)
    before = pkg.ops.CALLS["sat_points"]
    got = pkg.ops.sat_points(clean, adv, [j * 0.25 for j, _ in TABLE], [m for _, m in TABLE], out_dtype=torch.bfloat16)
    assert pkg.ops.CALLS["sat_points"] == before                  # no new kernel in this layout
    for g, w in zip(got, _expected(pkg, clean, adv, TABLE)):
        assert g.stride() == clean.stride() and torch.equal(g, w.to(torch.bfloat16))
    cl, al = clean.contiguous(memory_format=torch.channels_last), adv.contiguous(memory_format=torch.channels_last)
    off = pkg.ops.sat_points(cl, al, [0.5, 0.75], [True, False], fused=False)
    assert pkg.ops.CALLS["sat_points"] == before
    on = pkg.ops.sat_points(cl, al, [0.5, 0.75], [True, False])
    assert all(torch.equal(a, b) for a, b in zip(on, off))
    with pytest.raises(ValueError):
        pkg.ops.sat_points_block(clean, adv, [0.5], [False])
    with pytest.raises(ValueError):
        pkg.ops.sat_points(cl, al, [1.5], [False])
    with pytest.raises(TypeError):
        pkg.ops.sat_points(cl.to(torch.bfloat16), al.to(torch.bfloat16), [0.5], [False])
