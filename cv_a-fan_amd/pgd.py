"""The sign-PGD core every attack path is built from (attack_algo, seg_attack_algo, det_ops, det_attack_algo, infer.Attacker):

    start(x, eps, randinit, u, noise)     fp32 x in its own dense layout, its clone x_adv (+ the host- or device-drawn random start)
    input_gradient(loss_of, leaves)       d loss / d leaves with parameter gradients switched off
    step(x_adv, grad, gamma, x, eps, clip)   x_adv += gamma * sign(grad) [projected onto the eps-ball around x]: one launch
    ascend(x_adv, loss_of, ...)           input_gradient at x_adv, then step
    clamp01_(x_adv)                       the image attacks' final clamp
    step(..., clamp=(lo, hi))             the last step and that clamp in one launch (det_attack_algo.adv_input behind its switch)

A caller that already has the first step's gradient (`grad0`) skips ascend at t == 0 and calls step with it.

norm="linf" (the default of start, step and ascend) is the above.  norm="l2": the step is x_adv += gamma * grad / ||grad||_2 per
sample and the projection a rescaling onto the L2 ball of radius eps (ops.pgd_step_l2_: three launches, deterministic sums); the
random start is a point of the eps-sphere."""
import torch

from . import ops
from .resnet_s import _dense, _like_layout, dgrad_only

NORMS = ("linf", "l2")


def _check_norm(norm):
    if norm not in NORMS:
        raise ValueError(f"norm must be 'linf' or 'l2', not {norm!r}")


def start(x, eps, randinit, u=None, noise="host", norm="linf"):
    """(x as detached fp32, x_adv = its clone), both dense in x's own layout (channels-last feature maps stay channels-last: no
    transposes per step).  randinit: x_adv += (2u - 1) * eps with u = torch.rand(x.shape) from the CPU default generator, as the
    reference draws it, unless the caller hands its own draw in (host or device).  noise="device" with randinit: x_adv and its
    start come out of ONE launch that draws u itself from ops.noise_state (ops.pgd_rand_start; capturable, a replay draws afresh);
    the seed it used ([1] int64 on the device) rides on the result as `x_adv._afan_noise_seed`.
    norm="l2" with randinit: u = torch.randn(x.shape) from the CPU default generator (unless handed in), then ONE normalised step
    along it of length eps without projection (ops.pgd_step_l2_(x_adv, u, gamma=eps, clip=False)): a start ON the eps-sphere in a
    uniformly drawn direction.  The sphere stands in for the ball: the radius of a uniform draw in a P-dimensional ball exceeds
    0.99 eps with probability 1 - 0.99^P, which is 1 - 4e-14 at P = 3072.  noise="device" is not built for "l2" (ValueError)."""
    _check_norm(norm)
    if noise not in ("host", "device"):
        raise ValueError(f"noise must be 'host' or 'device', not {noise!r}")
    if x.device.type != "cuda":
        raise ops.AfanLibraryError("x must live on the MI355X (no CPU path in this build)")
    if norm == "l2" and noise == "device":
        raise ValueError("noise='device' is not built for norm='l2': the L2 start is drawn on the host")
    x = _dense(x.detach().float())
    if randinit and norm == "l2":
        x_adv = x.clone()
        u = torch.randn(x_adv.shape) if u is None else u
        ops.pgd_step_l2_(x_adv, _like_layout(u.to(x.device, non_blocking=True), x_adv), eps, clip=False)
        return x, x_adv
    if randinit and noise == "device":
        if u is not None:
            raise ValueError("noise='device' draws its own u")
        x_adv, used = ops.pgd_rand_start(x, eps)
        x_adv._afan_noise_seed = used
        return x, x_adv
    x_adv = x.clone()
    if randinit:
        u = torch.rand(x_adv.shape) if u is None else u
        ops.axpy_noise_(x_adv, u.to(x.device, non_blocking=True), eps)
    return x, x_adv


def input_gradient(loss_of, leaves):
    """d loss_of(leaves) / d leaves — one tensor for one leaf, a tuple for a list — and nothing else: the library's layers skip (and
    must not add into) parameter gradients inside (the reference's only_inputs=True).  A 0-dim fp32 loss on the GPU gets the cached
    1.0 as its root gradient instead of autograd's ones_like fill."""
    many = isinstance(leaves, (list, tuple))
    with torch.enable_grad(), dgrad_only():
        loss = loss_of(leaves)
        root = ops.one(loss.device) if (loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32) else None
        grads = torch.autograd.grad(loss, leaves if many else [leaves], grad_outputs=root, only_inputs=True)
    return grads if many else grads[0]


def step(x_adv, grad, gamma, x, eps, clip, shadow=None, norms=False, norm="linf", clamp=None):
    """In place, one launch: x_adv += gamma * sign(grad), then the projection onto [x - eps, x + eps] when clip; `shadow` receives the
    bf16 copy of the result.  norms=True: the launch also returns the per-sample (l2, linf) of x_adv - x.
    norm="l2": x_adv += gamma * grad / ||grad||_2 per sample, then the projection onto the L2 ball of radius eps around x when clip
    (ops.pgd_step_l2_); norms=True composes ops.perturb_norms after it.
    clamp=(lo, hi), L-inf only and without norms: the same launch also clamps the result to the scalar bounds — an image attack's last
    step and its final clamp (ops.pgd_step_clamp_: the bits of step, then clamp01_); grad may then be None (no step: steps = 0)."""
    _check_norm(norm)
    if clamp is not None and (norm != "linf" or norms):
        raise ValueError("clamp=(lo, hi) is built for the L-inf step without norms (norm='linf', norms=False)")
    if eps is None:
        if clip:
            raise ValueError("clip=True needs an eps")
        eps = 0.0
    if clamp is not None:
        lo, hi = clamp
        ops.pgd_step_clamp_(x_adv, None if grad is None else _like_layout(grad.detach(), x_adv), gamma, x, eps, clip, shadow, lo, hi)
        return None
    grad = _like_layout(grad.detach(), x_adv)
    if norm == "l2":
        ops.pgd_step_l2_(x_adv, grad, gamma, x, eps, clip, shadow)
        return ops.perturb_norms(x_adv, x) if norms else None
    if norms:
        return ops.pgd_step_norms_(x_adv, grad, gamma, x, eps, clip, shadow)
    ops.pgd_step_(x_adv, grad, gamma, x, eps, clip, shadow)


def ascend(x_adv, loss_of, gamma, x, eps, clip, shadow=None, norm="linf", clamp=None):
    """One ascent step at x_adv; the model reads the bf16 shadow of x_adv where there is one (no separate cast).  clamp: step's."""
    _check_norm(norm)
    xin = (x_adv if shadow is None else shadow).detach().requires_grad_(True)
    step(x_adv, input_gradient(loss_of, xin), gamma, x, eps, clip, shadow, norm=norm, clamp=clamp)


def clamp01_(x_adv):
    return ops.tensor_clamp_(x_adv, torch.zeros_like(x_adv), torch.ones_like(x_adv))
