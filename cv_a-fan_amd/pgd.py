"""The sign-PGD core every attack path is built from (attack_algo, seg_attack_algo, det_ops, det_attack_algo, infer.Attacker):

    start(x, eps, randinit, u, noise)     fp32 x in its own dense layout, its clone x_adv (+ the host- or device-drawn random start)
    input_gradient(loss_of, leaves)       d loss / d leaves with parameter gradients switched off
    step(x_adv, grad, gamma, x, eps, clip)   x_adv += gamma * sign(grad) [projected onto the eps-ball around x]: one launch
    ascend(x_adv, loss_of, ...)           input_gradient at x_adv, then step
    clamp01_(x_adv)                       the image attacks' final clamp

A caller that already has the first step's gradient (`grad0`) skips ascend at t == 0 and calls step with it."""
import torch

from . import ops
from .resnet_s import _dense, _like_layout, dgrad_only


def start(x, eps, randinit, u=None, noise="host"):
    """(x as detached fp32, x_adv = its clone), both dense in x's own layout (channels-last feature maps stay channels-last: no
    transposes per step).  randinit: x_adv += (2u - 1) * eps with u = torch.rand(x.shape) from the CPU default generator, as the
    reference draws it, unless the caller hands its own draw in (host or device).  noise="device" with randinit: x_adv and its
    start come out of ONE launch that draws u itself from ops.noise_state (ops.pgd_rand_start; capturable, a replay draws afresh);
    the seed it used ([1] int64 on the device) rides on the result as `x_adv._afan_noise_seed`."""
    if noise not in ("host", "device"):
        raise ValueError(f"noise must be 'host' or 'device', not {noise!r}")
    if x.device.type != "cuda":
        raise ops.AfanLibraryError("x must live on the MI355X (no CPU path in this build)")
    x = _dense(x.detach().float())
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


def step(x_adv, grad, gamma, x, eps, clip, shadow=None, norms=False):
    """In place, one launch: x_adv += gamma * sign(grad), then the projection onto [x - eps, x + eps] when clip; `shadow` receives the
    bf16 copy of the result.  norms=True: the launch also returns the per-sample (l2, linf) of x_adv - x."""
    if eps is None:
        if clip:
            raise ValueError("clip=True needs an eps")
        eps = 0.0
    grad = _like_layout(grad.detach(), x_adv)
    if norms:
        return ops.pgd_step_norms_(x_adv, grad, gamma, x, eps, clip, shadow)
    ops.pgd_step_(x_adv, grad, gamma, x, eps, clip, shadow)


def ascend(x_adv, loss_of, gamma, x, eps, clip, shadow=None):
    """One ascent step at x_adv; the model reads the bf16 shadow of x_adv where there is one (no separate cast)."""
    xin = (x_adv if shadow is None else shadow).detach().requires_grad_(True)
    step(x_adv, input_gradient(loss_of, xin), gamma, x, eps, clip, shadow)


def clamp01_(x_adv):
    return ops.tensor_clamp_(x_adv, torch.zeros_like(x_adv), torch.ones_like(x_adv))
