"""A-FAN operators, MI355X-native: drop-in for the reference's `attack_algo` modules.

Same names, argument meaning and return contract as
  Classification/attack_algo.py:9-58   tensor_clamp, linfball_proj, PGD
  Segmentation/attack_algo.py:108-130  get_sample_points, mix_feature   (== Detection/attack_algo.py:236-265)
but every arithmetic step is a hand-written HIP kernel from libafan_hip.so (sign-step + projection +
per-sample norms fused in one pass; channel-moment re-normalisation in one pass).  `model` may be any
nn.Module on the GPU that follows the slice protocol `model(t, end_point=, start_point=)`.  The loop
itself (input gradient, sign step) is pgd.py's; PGD keeps its one-launch start and the bf16 shadow.
"""
import os

import torch

from . import ops, pgd
from .resnet_s import _dense, _like_layout, fused_criterion, tail_end_kwargs

__all__ = ["PGD", "tensor_clamp", "linfball_proj", "l2ball_proj", "mix_feature", "get_sample_points", "last_norms"]

_last = {"l2": None, "linf": None}
# 1: the L-inf loop on a bf16 map keeps one byte of sign codes per element between its steps and writes the fp32 iterate once, after
# the last (ops.pgd_packed_step_ / pgd_packed_last: the same bits); 0: the fp32 iterate of ops.pgd_init / pgd_step_ throughout (A/B)
_PGD_PACKED = os.environ.get("AFAN_PGD_PACKED", "1") != "0"


def pgd_packed_ok(x, model, steps, norm="linf", randinit=False):
    """Whether PGD(x, ...) takes the packed route: a bf16 map on the GPU under a bf16 model, the L-inf attack from x itself, one to
    ops.PGD_PACKED_MAX_STEPS steps, and the switch on.  The trainers ask before they decide which tensor to hand over."""
    return bool(_PGD_PACKED and isinstance(x, torch.Tensor) and x.device.type == "cuda" and x.dtype == torch.bfloat16
                and getattr(model, "compute_dtype", torch.float32) == torch.bfloat16 and norm == "linf" and not randinit
                and 1 <= steps <= ops.PGD_PACKED_MAX_STEPS)


def last_norms():
    """Per-sample (L2, Linf) of the perturbation produced by the most recent PGD(..., with_norms=True) call:
    device tensors, no host sync (main_perturb.py:188-192 computes them on the host from a D2H copy)."""
    return _last["l2"], _last["linf"]


def tensor_clamp(t, min, max, in_place=True):
    """attack_algo.py:9-19: element-wise clamp between two tensors, lower bound first."""
    res = t if in_place else t.clone()
    ops.tensor_clamp_(res.data, min.contiguous(), max.contiguous())
    return res


def linfball_proj(center, radius, t, in_place=True):
    """attack_algo.py:35-36: project t onto the L-inf ball of `radius` around `center` (one HIP launch)."""
    res = t if in_place else t.clone()
    zero = torch.zeros_like(res.data)
    ops.pgd_step_(res.data, zero, 0.0, x_clean=center.contiguous(), eps=float(radius), clip=True)
    return res


def l2ball_proj(center, radius, t, in_place=True):
    """attack_algo.py:21-33: project each sample t[b] onto the L2 ball of `radius` around center[b] (the projection-only form of
    ops.pgd_step_l2_: two launches).  Two deliberate differences from the reference as written: a point inside the ball keeps its
    bits, where the reference rounds every point through `/ dist * dist`; and a zero perturbation stays zero, where the reference
    divides 0 / 0 and returns NaN."""
    res = t if in_place else t.clone()
    data = res.data
    if _dense(data) is not data or data.dtype != torch.float32:
        raise ValueError("l2ball_proj: t must be a dense fp32 tensor (contiguous NCHW or channels_last)")
    ops.pgd_step_l2_(data, None, 0.0, x_clean=_like_layout(center.detach().float(), data), eps=float(radius), clip=True)
    return res


def PGD(x, loss_fn, y=None, model=None, steps=3, gamma=None, start_idx=1, layer_number=16, eps=(2 / 255),
        randinit=False, clip=False, with_norms=False, grad0=None, norm="linf", tail_end=False):
    """K-step sign-gradient ascent on the feature map `x` (attack_algo.py:38-58).  norm="l2" (an addition): the steps are
    normalised-gradient steps and the projection is onto the L2 ball (pgd.step(norm="l2")); the random start is pgd.start's.

    Returns a NEW fp32 leaf tensor with requires_grad=True; `x` is not modified.  `with_norms=True`
    (an addition) fuses the per-sample L2/Linf perturbation norms into the last step; read them with
    `last_norms()`.  `grad0` (an addition; not with randinit): a positive multiple of d(loss)/d(x) at x itself, already
    computed by the caller — the first ascent step uses it instead of running the tail on x (sign() ignores the scale).
    `tail_end=True` (an addition): the caller allows the one-launch end of each tail pass (resnet_s._HeadCEFn) where the model and
    the criterion take it; the default keeps the separate launches, and with them the bits of every schedule that does not ask.
    A bf16 `x` under a bf16 model, norm="linf", no randinit and 1 <= steps <= 5 take the packed route (pgd_packed_ok, _pgd_packed):
    the same values from fewer bytes; the result then also carries `_afan_clean32`, the fp32 copy of `x`.
    """
    if x.device.type != "cuda":
        raise ops.AfanLibraryError("PGD: x must live on the MI355X (no CPU path in this build)")
    pgd._check_norm(norm)
    # keep whatever dense layout the feature map has (the bf16 backbone hands over channels-last tensors: a
    # .contiguous() here would transpose 64 MB to NCHW and the tail would transpose it back every PGD step)
    lp = getattr(model, "compute_dtype", torch.float32) == torch.bfloat16
    if grad0 is not None and (randinit or steps < 1):
        raise ValueError("grad0 is the gradient at x: not with randinit, and only when there is a first step")
    if pgd_packed_ok(x, model, steps, norm, randinit):
        return _pgd_packed(_dense(x.detach()), loss_fn, y, model, steps, gamma, start_idx, layer_number, eps, clip, with_norms, grad0,
                           tail_end)
    # x (bf16 from the product's backbone, or fp32) -> fp32 x, its clone x_adv and, where the first tail pass needs it, the
    # bf16 shadow: one launch (with grad0 the first step's kernel writes the shadow; with randinit the noise kernel does)
    x, x_adv, shadow = ops.pgd_init(_dense(x.detach()), want_shadow=lp and grad0 is None and not randinit)
    if lp and shadow is None:
        shadow = torch.empty_like(x, dtype=torch.bfloat16)
    if randinit and norm == "l2":
        # pgd.start's L2 start (a point of the eps-sphere along a host-drawn Gaussian direction), written with the shadow
        u = _like_layout(torch.randn(x_adv.shape).to(x.device, non_blocking=True), x_adv)
        ops.pgd_step_l2_(x_adv, u, eps, clip=False, shadow=shadow)
    elif randinit:
        # the reference draws the noise on the CPU default generator (attack_algo.py:44); same stream here
        ops.axpy_noise_(x_adv, torch.rand(x_adv.shape).to(x.device, non_blocking=True), eps, shadow)
    l2 = linf = None
    loss_fn = fused_criterion(loss_fn, model)
    # the library's own criterion on a model that takes the target: head, loss gradient and the last BatchNorm's sums in one launch,
    # no loss value (only the gradient is used here)
    ce_kw = tail_end_kwargs(model, loss_fn, y, ops.one(x.device), want_value=False) if tail_end else {}
    for t in range(steps):
        if t == 0 and grad0 is not None:
            grad = grad0
        else:
            # the tail consumes the bf16 shadow written by the previous step's kernel (no separate cast)
            xin = (shadow if lp else x_adv).detach().requires_grad_(True)
            grad = pgd.input_gradient(lambda t: loss_fn(model(t, end_point=layer_number, start_point=start_idx, **ce_kw), y), xin)
        if with_norms and t == steps - 1:
            l2, linf = pgd.step(x_adv, grad, gamma, x, eps, clip, shadow, norms=True, norm=norm)
        else:
            pgd.step(x_adv, grad, gamma, x, eps, clip, shadow, norm=norm)
    if with_norms:
        if l2 is None:
            l2, linf = ops.perturb_norms(x_adv, x)
        _last["l2"], _last["linf"] = l2, linf
    x_adv.requires_grad_(True)
    if lp:
        x_adv._afan_shadow = shadow  # bf16 copy of the final x_adv for the adv tail forward
    return x_adv


def _pgd_packed(x, loss_fn, y, model, steps, gamma, start_idx, layer_number, eps, clip, with_norms, grad0, tail_end):
    """PGD's L-inf loop on the bf16 map x with no fp32 tensor before the last step: each step leaves its sign decision in one byte of
    2-bit codes per element and the bf16 shadow the next tail pass reads; the last launch writes the fp32 iterate, the fp32 copy of
    x (`_afan_clean32`: what the old route's start wrote) and the norms.  No start launch: the first tail pass reads x itself."""
    if eps is None:
        if clip:
            raise ValueError("clip=True needs an eps")
        eps = 0.0
    codes = torch.empty_like(x, dtype=torch.uint8) if steps > 1 else None
    shadow = torch.empty_like(x)
    loss_fn = fused_criterion(loss_fn, model)
    ce_kw = tail_end_kwargs(model, loss_fn, y, ops.one(x.device), want_value=False) if tail_end else {}
    for t in range(steps):
        if t == 0 and grad0 is not None:
            grad = grad0
        else:
            xin = (x if t == 0 else shadow).detach().requires_grad_(True)
            grad = pgd.input_gradient(lambda t: loss_fn(model(t, end_point=layer_number, start_point=start_idx, **ce_kw), y), xin)
        grad = _like_layout(grad.detach(), x)
        if t < steps - 1:
            ops.pgd_packed_step_(x, grad, codes, t, gamma, eps, clip, shadow)
        else:
            x_adv, x32, l2, linf = ops.pgd_packed_last(x, grad, codes, t, gamma, eps, clip, shadow, want_x32=True, norms=with_norms)
    if with_norms:
        _last["l2"], _last["linf"] = l2, linf
    x_adv.requires_grad_(True)
    x_adv._afan_shadow = shadow
    x_adv._afan_clean32 = x32
    return x_adv


def mix_feature(clean_feature, adv_feature):
    """Segmentation/attack_algo.py:121-130: re-normalise clean features to the adversarial channel statistics."""
    return ops.mix_feature(_dense(clean_feature), _dense(adv_feature), 1e-5)      # (either dense layout; adv follows clean's)


def sample_points_mixed(pointx, pointy, number, mix):
    """get_sample_points followed by `points[j] = mix_feature(pointx, points[j])` for every j >= 1 with mix[j-1] set
    (Segmentation/main_aug_final.py:186-192), fused: clean and adv are read once."""
    px, py = _dense(pointx), _dense(pointy)
    if py.stride() != px.stride():
        py = _like_layout(py, px)
    return [pointx] + ops.lerp_mix(px, py, number, [bool(f) for f in mix])


def get_sample_points(pointx, pointy, number):
    """Segmentation/attack_algo.py:108-118: [x, lerp(x,y,1/(n-1)), ..., y]; interior points in one launch."""
    px, py = _dense(pointx), _dense(pointy)
    if py.stride() != px.stride():
        py = _like_layout(py, px)
    inner = ops.lerp_points(px, py, number)
    return [pointx] + inner + [pointy]
