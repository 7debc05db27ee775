"""The Segmentation A-FAN iteration (Segmentation/main_aug_final.py:149-232) on one MI355X: owner of the parameter arena,
the two-group SGD and the PolyLR schedule around `seg_attack_algo.seg_train_step`.

    head pass (SE, out_idx) + clean decoder-head pass (SD) -> K-step SE feature PGD + K-step SD decoder PGD
    -> 3 SAT sample points + mix_feature -> clean / SE1 / SE2 / SD forwards -> 0.7/0.1/0.1/0.1 loss -> backward -> SGD

Reference details kept: BatchNorm momentum 0.01 in the backbone (main_aug_final.py:77), SGD(momentum 0.9) with the
backbone at 0.1 x lr (:79-82), PolyLR(power 0.9) stepped once per iteration (:261), CrossEntropyLoss(ignore_index=255).
After `graph_warmup` eager iterations the whole iteration body is captured into a hipGraph and replayed
(train_step.StepTrainer's schedule)."""
import torch
import torch.nn as nn

from . import ops, resnet_s
from .arena import ArenaSGD, ParamArena
from .deeplab import PolyLR, set_bn_momentum
from .seg_attack_algo import _f32_logits, seg_train_phases, seg_train_step
from .train_step import StepTrainer


class SegTrainer(StepTrainer):
    """step(images, labels): one iteration, device tensors only.  The scheduler is NOT stepped there — call
    `trainer.scheduler.step()` once per iteration like main_aug_final.py:261 — and `flush_guard()` belongs at every logging
    interval (grid_guard.py)."""
    _what = "the segmentation A-FAN step"
    _small = ("loss", "losses")

    def __init__(self, model, criterion=None, *, steps=1, eps=2.0, gamma_se=0.5, gamma_sd=0.5, pertub_idx_se=3,
                 pertub_idx_sd="aspp", mix_layer="11", mix_sd=False, noise_sd=0.0, randinit=False, clip=False, lr=0.01,
                 momentum=0.9, weight_decay=1e-4, total_itrs=30000, lr_policy="poly", step_size=10000,
                 backbone_bn_momentum=0.01, use_graph=True, graph_warmup=2, dual_bn=False, fold_clean=None, group=None,
                 allreduce_chunks=4, fold_pgd0=None, segmented=None, wgrad_stream=None, batch_tails=None):
        self.model = model
        if dual_bn:      # BASELINE configs[3] "+ dual-BN": an option the reference does not have (resnet_s.enable_dual_bn); default off
            resnet_s.enable_dual_bn(model)
        self.criterion = criterion if criterion is not None else nn.CrossEntropyLoss(ignore_index=255, reduction="mean")
        self.kw = dict(steps=steps, eps=eps, gamma_se=gamma_se, gamma_sd=gamma_sd, pertub_idx_se=pertub_idx_se,
                       pertub_idx_sd=pertub_idx_sd, mix_layer=mix_layer, mix_sd=mix_sd, noise_sd=noise_sd, randinit=randinit,
                       clip=clip, dual_bn=bool(dual_bn), fold_clean=fold_clean, fold_pgd0=fold_pgd0, batch_tails=batch_tails)
        if backbone_bn_momentum is not None:
            set_bn_momentum(model.backbone, backbone_bn_momentum)
        self.arena = ParamArena(model, skip=())
        self.optimizer = ArenaSGD(self.arena, lr, momentum, weight_decay,
                                  groups=[("backbone.", 0.1 * lr), ("classifier.", lr)])
        if lr_policy == "poly":
            self.scheduler = PolyLR(self.optimizer, total_itrs, power=0.9)
        else:
            self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=step_size, gamma=0.1)
        # data parallel (BASELINE configs[3] is 4 GPUs x 2 images): minibatch sharding, BatchNorm per replica like the
        # reference's nn.DataParallel, ONE exchange per iteration — the fp32 gradient arena, summed over the ranks in
        # chunks on a side stream after the backward, 1/world folded into the SGD kernel.  The iteration's graph ends
        # before the optimizer step; the all-reduce and the one SGD launch follow it.
        self._init_exchange(model, group, allreduce_chunks)
        self.segmented = bool(segmented)      # True: run the two-phase (cut) schedule on one GPU too (tests)
        if self._phased():
            self.kw["defer_step"] = True
        self._init_schedule(bool(use_graph) and not randinit and noise_sd == 0, graph_warmup)
        # weight gradients on a side stream / parallel graph branch (resnet_s._WgradStream): None = by workload size — it
        # pays from about 8 images of 513 x 513 per GPU (55.2 -> 52.6 ms), not at the 2-image share (25.3 -> 25.5 ms)
        self.wgrad_stream = wgrad_stream

    WGRAD_STREAM_MIN_PIXELS = 1 << 21

    def _wgrad_side(self, images):
        if self.wgrad_stream is not None:
            return bool(self.wgrad_stream)
        return images.is_cuda and images.shape[0] * images.shape[2] * images.shape[3] >= self.WGRAD_STREAM_MIN_PIXELS

    def _body(self, images, labels):
        return seg_train_step(self.model, self.optimizer, self.criterion, images, labels, **self.kw)

    def _phases(self, images, labels, out):
        """The iteration as a generator that yields where a part of the gradients is final (what a subclass replaces with _body)."""
        return seg_train_phases(self.model, self.optimizer, self.criterion, images, labels, out, **self.kw)

    # ---- data parallel: the tail's gradients (everything behind the SE point: layer4, ASPP, decoder — 53 % of DeepLabv3+
    # ResNet-101's 58.7 M parameters, the LAST contiguous range of the arena) are final when seg_train_phases yields "tail";
    # their all-reduce starts there, on the side stream, and runs under the head's backward.  The rest follows at finish().
    def _tail_range(self):
        se = self.kw["pertub_idx_se"]
        if type(se) != int:
            return None
        pre = tuple(f"backbone.layer{k}." for k in range(se + 1, 5)) + ("classifier.",)
        idx = [i for i, n in enumerate(self.arena.names) if n.startswith(pre)]
        if not idx or idx != list(range(idx[0], idx[-1] + 1)):
            return None
        return idx[0], idx[-1] + 1

    def _phased(self):
        return self.segmented or self.reducer is not None

    def _use_phases(self, images):
        return self._phased()

    def _range_of(self, label):
        return self._tail_range() if label == "tail" else None

    def _around(self, images):
        return resnet_s.wgrad_stream(self._wgrad_side(images))

    def _update(self):
        if self._phased():                 # (else _body has stepped)
            super()._update()

    def _capture(self, images, labels):
        super()._capture(images, labels)
        if self._pieces is None:
            self._pieces = [(self._graph, None)]      # one graph: one piece with nothing to announce


def seg_base_phases(model, optimizer, criterion, images, labels, out, *, defer_step=False):
    """The baseline iteration, Segmentation/main_ori.py:158-163, as a generator in seg_train_phases' form: one train-mode forward,
    the cross-entropy on the upsampled logits (on the LOW-resolution logits where the one-pass kernel takes them), backward, step.
    Nothing is final before the end of the backward, so it never yields."""
    from .deeplab import seg_criterion
    criterion = seg_criterion(criterion)
    if images.is_cuda:
        ops.acc_reset(images.device)            # BatchNorm accumulator arena: one memset per iteration
    optimizer.zero_grad()
    low = bool(getattr(criterion, "low_res", False))
    o = model({"x": images, "adv": None, "out_idx": 0, "flag": "clean", "low_res": low})
    if getattr(criterion, "fused", False) and _f32_logits(o):
        loss = criterion(o, labels, grad_scale=1.0)
        torch.autograd.backward([loss], [ops.one(images.device)])
    else:
        loss = criterion(o, labels)
        loss.backward()
    if not defer_step:
        optimizer.step()
    out.update({"loss": loss.detach()})
    return
    yield


class SegBaseTrainer(SegTrainer):
    """The segmentation baseline (Segmentation/main_ori.py): SegTrainer's arena, two-group SGD, schedule, BatchNorm momentum, graph
    capture, grid guard and data-parallel exchange around the plain iteration — no PGD, no mixing.  step() returns {"loss": ...}."""

    def __init__(self, model, criterion=None, *, lr=0.01, momentum=0.9, weight_decay=1e-4, total_itrs=30000, lr_policy="poly",
                 step_size=10000, backbone_bn_momentum=0.01, use_graph=True, graph_warmup=2, group=None, allreduce_chunks=4,
                 segmented=None, wgrad_stream=None):
        super().__init__(model, criterion, lr=lr, momentum=momentum, weight_decay=weight_decay, total_itrs=total_itrs,
                         lr_policy=lr_policy, step_size=step_size, backbone_bn_momentum=backbone_bn_momentum, use_graph=use_graph,
                         graph_warmup=graph_warmup, group=group, allreduce_chunks=allreduce_chunks, segmented=segmented,
                         wgrad_stream=wgrad_stream)
        self.kw = {"defer_step": True} if self.kw.get("defer_step") else {}

    def _phases(self, images, labels, out):
        return seg_base_phases(self.model, self.optimizer, self.criterion, images, labels, out, **self.kw)

    def _body(self, images, labels):
        out = {}
        for _ in self._phases(images, labels, out):
            pass
        return out

    def _tail_range(self):
        return None


def seg_adv_phases(model, optimizer, criterion, images, labels, out, *, steps_pgd=1, eps_pgd=2.0, gamma_pgd=0.5, randinit=False,
                   clip=False, noise="device", defer_step=False):
    """The PGD-training iteration, Segmentation/main_advtrain.py:185-202, in seg_base_phases' form: image-space sign-PGD on the batch
    with the model as the loop leaves it, in TRAINING mode (:185-194 — every attack pass normalises with batch statistics, updates the
    running statistics and draws ASPP's dropout; no parameter gradient is computed, pgd.input_gradient runs under dgrad_only), then
    seg_base_phases' body on the adversarial images (:196-202).  noise: where --randinit_pgd's start is drawn — "device" in the
    start's own launch (ops.pgd_rand_start: the whole iteration can be captured), "host" on torch's CPU generator as the reference
    does.  out: loss, adv_images, noise_seed (the device draw's seed word, None without one).  Never yields."""
    from .deeplab import seg_criterion
    from .seg_attack_algo import adv_input
    criterion = seg_criterion(criterion)
    if images.is_cuda:
        ops.acc_reset(images.device)            # BatchNorm accumulator arena: one memset per iteration
    adv_images = adv_input(x=images, criterion=criterion, y=labels, model=model, steps=steps_pgd, eps=(eps_pgd / 255),
                           gamma=(gamma_pgd / 255), randinit=randinit, clip=clip, noise=noise)
    seed = getattr(adv_images, "_afan_noise_seed", None)
    adv_images = adv_images.detach()
    optimizer.zero_grad()
    low = bool(getattr(criterion, "low_res", False))
    o = model({"x": adv_images, "adv": None, "out_idx": 0, "flag": "clean", "low_res": low})
    if getattr(criterion, "fused", False) and _f32_logits(o):
        loss = criterion(o, labels, grad_scale=1.0)
        torch.autograd.backward([loss], [ops.one(images.device)])
    else:
        loss = criterion(o, labels)
        loss.backward()
    if not defer_step:
        optimizer.step()
    out.update({"loss": loss.detach(), "adv_images": adv_images, "noise_seed": seed})
    return
    yield


class SegAdvTrainer(SegBaseTrainer):
    """Segmentation PGD training (Segmentation/main_advtrain.py): SegBaseTrainer's arena, two-group SGD, schedule, BatchNorm momentum,
    grid guard and data-parallel exchange around seg_adv_phases.  step() returns {"loss", "adv_images", "noise_seed"}.  With a random
    start drawn on the host the iteration stays eager (the draw and its upload happen every step); drawn on the device it is captured
    whole — attack passes, random start, training pass, SGD launch — and every replay draws a fresh start."""
    _what = "the segmentation PGD-training step"
    _small = ("loss",)

    def __init__(self, model, criterion=None, *, steps_pgd=1, eps_pgd=2.0, gamma_pgd=0.5, randinit=False, clip=False, noise="device",
                 lr=0.01, momentum=0.9, weight_decay=1e-4, total_itrs=30000, lr_policy="poly", step_size=10000,
                 backbone_bn_momentum=0.01, use_graph=True, graph_warmup=2, group=None, allreduce_chunks=4, segmented=None,
                 wgrad_stream=None):
        if noise not in ("device", "host"):
            raise ValueError(f"noise must be 'device' or 'host', not {noise!r}")
        super().__init__(model, criterion, lr=lr, momentum=momentum, weight_decay=weight_decay, total_itrs=total_itrs,
                         lr_policy=lr_policy, step_size=step_size, backbone_bn_momentum=backbone_bn_momentum,
                         use_graph=bool(use_graph) and (not randinit or noise == "device"), graph_warmup=graph_warmup, group=group,
                         allreduce_chunks=allreduce_chunks, segmented=segmented, wgrad_stream=wgrad_stream)
        self.kw.update(steps_pgd=steps_pgd, eps_pgd=eps_pgd, gamma_pgd=gamma_pgd, randinit=bool(randinit), clip=bool(clip), noise=noise)
        if randinit and noise == "device" and self.arena.param.is_cuda:
            ops.noise_state(self.arena.param.device)        # seeded here, from the host generator: never inside a capture

    def _phases(self, images, labels, out):
        return seg_adv_phases(self.model, self.optimizer, self.criterion, images, labels, out, **self.kw)
