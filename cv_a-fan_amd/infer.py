"""Eval-mode forward of the Classification ResNets (resnet_s.ARCHS) for checkpoint evaluation: main_perturb.validate,
main_learnable (through it) and main_inference.

bf16 channels-last models run a fused forward: every convolution is ONE launch with its eval-mode BatchNorm (running
statistics, a frozen affine) (+ the block's residual) (+ ReLU) in the epilogue (afan_conv_fwd_affine_nhwc_bf16 with any_family = 1; the tiled,
small-channel, 64 -> 64 and 3-channel-stem kernels all have that form) — bit for bit the eager path's convolution followed by
its afan_bn_apply.  A projection shortcut's BatchNorm goes through its own convolution's epilogue; the option-A pad shortcut,
the ResNet-50 max-pool and the classifier head are the eager path's calls.  The ResNet-50 7x7 stem is its im2col followed by
a fused 1x1 convolution (the eager path's own decomposition); under AFAN_STEM7_DIRECT=1 it is the direct stem kernel followed
by one afan_affine_apply.

The forward reads only buffers the Evaluator owns (bf16 weight copies, [4][C] coefficient blocks, the head's parameters),
rewritten in place by refresh() at the start of every evaluation pass, so one hipGraph per batch shape (_ShapeGraphs: forward +
criterion + accuracy) serves every epoch.  fp32, NCHW, or a criterion other than a default
nn.CrossEntropyLoss: the model's own eager forward.

Attacker (below) is its counterpart for robust accuracy: image-space PGD on the eval-mode model, forward and backward one launch per
convolution, the whole attack one hipGraph per batch shape."""
import torch
import torch.nn as nn

from . import frozen, ops, pgd, resnet_s
from .deeplab import StemConv, _Stem7Fn


def accuracy(output, target):
    """main_perturb.accuracy: top-1 precision in percent, on the device."""
    return (output.argmax(dim=1) == target).float().sum() * (100.0 / target.shape[0])


class _Unfused(Exception):
    """A layer of this batch shape is not on the library's bf16 MFMA kernels in the eager path: evaluate eagerly."""


class _ShapeGraphs:
    """The per-batch-shape schedule of Evaluator and Attacker: eager on a key's first sight, captured into a hipGraph on its second (a
    shape that recurs every epoch gets its graph; its first pass was the warm-up), replayed from then on.  fused_fn(*statics) -> tuple
    of outputs is what gets captured (a static input may be None); where it raises _Unfused the shape is remembered and eager_fn
    runs, now and ever after.  A replay hands out clones of the outputs — except the first `borrow` of them, which stay the graph's
    own static tensors (overwritten by the next replay)."""

    def __init__(self, fused_fn, eager_fn, borrow=0):
        self.fused_fn, self.eager_fn, self.borrow = fused_fn, eager_fn, borrow
        self._graphs, self._seen, self._eager_shapes = {}, {}, set()
        self._pool = None               # one memory pool for the instance's graphs

    def __call__(self, key, shape, *inputs):
        g = self._graphs.get(key)
        if g is not None:
            graph, statics, outs = g
            for s, t in zip(statics, inputs):
                if s is not None:
                    s.copy_(t)
            graph.replay()
            return outs[:self.borrow] + tuple(o.clone() for o in outs[self.borrow:])
        if shape in self._eager_shapes:
            return self.eager_fn(*inputs)
        try:
            r = self.fused_fn(*inputs)
        except _Unfused:
            self._eager_shapes.add(shape)
            return self.eager_fn(*inputs)
        self._seen[key] = self._seen.get(key, 0) + 1
        if self._seen[key] >= 2:
            self._capture(key, inputs)
        return r

    def _capture(self, key, inputs):
        dev = inputs[0].device
        statics = tuple(None if t is None else t.clone() for t in inputs)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with ops.capturing(graph, stream, self._pool):
            outs = tuple(self.fused_fn(*statics))
        torch.cuda.current_stream(dev).wait_stream(stream)
        if self._pool is None:
            self._pool = graph.pool()
        self._graphs[key] = (graph, statics, outs)


def _default_ce(criterion):
    return (type(criterion) is nn.CrossEntropyLoss and criterion.weight is None and criterion.ignore_index == -100
            and criterion.reduction == "mean" and getattr(criterion, "label_smoothing", 0.0) == 0.0)


def _main_bn(bn):
    """(weight, bias, running_mean, running_var) of `bn`'s main set (dual BatchNorm: the set in the module unless the
    auxiliary one is swapped in)."""
    src = bn.adv if getattr(bn, "adv", None) is not None and bn._branch != "main" else bn
    return src.weight, src.bias, src.running_mean, src.running_var


class _Conv:
    """One convolution + its BatchNorm: a private bf16 weight copy and a coefficient block."""

    def __init__(self, conv, bn, relu):
        self.conv, self.bn, self.relu = conv, bn, relu
        self.stride = int(conv.stride[0])
        self.stem7 = isinstance(conv, StemConv)
        self.w = None
        self.coefs = None

    def refresh(self):
        w = self.conv.lp_weight().detach()
        if self.stem7 and not _Stem7Fn.DIRECT:
            # the eager stem's 1x1 weight over the 152 im2col columns (deeplab._Stem7Fn.forward), built in place
            k = ops._lib.load().afan_conv_stem7_im2col_k()
            if self.w is None:
                self.w = torch.zeros((64, k, 1, 1), dtype=torch.bfloat16, device=w.device)   # (1x1: also channels-last)
            self.w.view(64, k)[:, :147].copy_(w.permute(0, 2, 3, 1).reshape(64, 147))
        else:
            if self.w is None or self.w.shape != w.shape:
                self.w = torch.empty_like(w, memory_format=torch.channels_last)
            self.w.copy_(w)
        wt, b, rm, rv = _main_bn(self.bn)
        c = frozen.affine_coefs(wt, b, rm, rv, self.bn.eps)
        if self.coefs is None:
            self.coefs = torch.empty_like(c)
        self.coefs.copy_(c)

    def __call__(self, x, residual=None):
        if self.stem7:
            w = self.conv.lp_weight()          # (the eager StemConv's test: otherwise the general kernel)
            if not (ops.conv_stem7_ok(x, w, self.conv.stride, self.conv.padding) and w.is_contiguous(memory_format=torch.channels_last)):
                raise _Unfused
            if _Stem7Fn.DIRECT:
                return ops.affine_apply(ops.conv_stem7_fwd(x, self.w), self.coefs, residual, self.relu)
            x, stride = ops.conv_stem7_im2col(x), 1          # (the columns are already at the output's stride-2 positions)
        elif not resnet_s._own_conv_ok(x, self.w, self.conv.stride, self.conv.padding, self.conv.dilation):
            raise _Unfused
        else:
            stride = self.stride
        y = ops.conv_fwd_affine(x, self.w, stride, self.coefs, residual, self.relu, any_kernel=True)
        if y is None:     # (no kernel with the epilogue takes the shape: the two launches it stands for)
            y = ops.affine_apply(ops.conv_fwd(x, self.w, stride), self.coefs, residual, self.relu)
        return y


class Evaluator:
    """evaluate(inp, target) -> (loss, prec1) as device scalars, the model in eval mode, no gradients.  See the module
    docstring; call refresh() once per evaluation pass (after the weights or running statistics changed)."""

    def __init__(self, model, criterion):
        self.model, self.criterion = model, criterion
        self.fused = (isinstance(model, resnet_s.ResNet) and type(model).forward is resnet_s.ResNet.forward
                      and model.compute_dtype == torch.bfloat16 and model.channels_last and _default_ce(criterion)
                      and next(model.parameters()).is_cuda)
        self._shapes = _ShapeGraphs(self._fused_step, self._eager, borrow=1)
        self.last_logits = None          # logits of the last evaluate() (a graph's static output after a replay)
        if self.fused:
            self._plan()

    # ------------------------------------------------------------------------------------------------ plan
    def _plan(self):
        L = list(self.model.sequential_model)
        norm = L[0]
        assert isinstance(norm, resnet_s.NormalizeByChannelMeanStd)
        self.norm = norm
        self.stem = _Conv(L[1], L[2], isinstance(L[3], nn.ReLU))
        i = 4 if isinstance(L[3], nn.ReLU) else 3
        self.pre = []                                   # modules between the stem and the first block (ResNet-50's max-pool)
        while not isinstance(L[i], (resnet_s.BasicBlock, resnet_s.Bottleneck)):
            self.pre.append(L[i])
            i += 1
        self.blocks = []
        while isinstance(L[i], (resnet_s.BasicBlock, resnet_s.Bottleneck)):
            blk = L[i]
            chain = [_Conv(c, b, True) for c, b in blk._chain()]      # every BatchNorm of the chain is followed by a ReLU
            sc = _Conv(blk.shortcut[0], blk.shortcut[1], False) if blk._sc_kind == "conv" else None
            self.blocks.append((blk, chain, sc))
            i += 1
        if not (isinstance(L[i], resnet_s._HeadPool) and isinstance(L[i + 1], nn.Flatten) and isinstance(L[i + 2], nn.Linear)):
            raise ValueError("Evaluator: expected the pool / flatten / linear head")
        self.lin = L[i + 2]
        self.convs = [self.stem] + [c for _, ch, sc in self.blocks for c in ch + ([sc] if sc else [])]
        self.mean = self.std = self.lin_w = self.lin_b = None

    def refresh(self):
        """Rewrite the private buffers (weights, coefficients, normalisation constants, head) in place from the model."""
        if not self.fused:
            return
        with torch.no_grad():
            for c in self.convs:
                c.refresh()
            for name, src in (("mean", self.norm.mean), ("std", self.norm.std), ("lin_w", self.lin.weight), ("lin_b", self.lin.bias)):
                if src is None:
                    continue
                dst = getattr(self, name)
                if dst is None:
                    setattr(self, name, src.detach().clone())
                else:
                    dst.copy_(src.detach())

    # --------------------------------------------------------------------------------------------- forward
    def _forward(self, x):
        """The eval forward of ResNet.forward, one fused launch per convolution."""
        x = ops.normalize_nchw(x.contiguous().float(), self.mean, self.std, torch.bfloat16, True)
        x = self.stem(x)
        for m in self.pre:
            x = m(x)
        for blk, chain, sc in self.blocks:
            h = x
            for c in chain[:-1]:
                h = c(h)
            if sc is not None:
                res = sc(x)
            elif blk._sc_kind == "pad":
                res = blk.shortcut(x).contiguous(memory_format=torch.channels_last)
            else:
                res = x
            x = chain[-1](h, res)
        lin = self.lin
        xh = resnet_s._head_in(x)
        if resnet_s._head_ok(xh, lin):
            return ops.head_forward(xh, self.lin_w, self.lin_b)[0]
        x = x.float().mean(dim=(2, 3), keepdim=True).flatten(1)          # _HeadPool, Flatten, then resnet_s._linear's kernel
        return resnet_s._LinearFn.apply(x, self.lin_w, self.lin_b, False)

    def _eager(self, inp, target):
        m = self.model
        out = m(inp, end_point=m.layer_number, start_point=0)
        loss = self.criterion(out, target)
        return out, loss.float(), accuracy(out.float(), target)

    def _fused_step(self, inp, target):
        out = self._forward(inp)
        loss = self.criterion(out, target)
        return out, loss.float(), accuracy(out.float(), target)

    def forward(self, inp):
        """Logits of the eval forward (fused or eager) — no graph."""
        with torch.no_grad():
            if self.fused and self._shape_fused(inp):
                try:
                    return self._forward(inp)
                except _Unfused:
                    self._shapes._eager_shapes.add(tuple(inp.shape))
            m = self.model
            return m(inp, end_point=m.layer_number, start_point=0)

    def _shape_fused(self, inp):
        return tuple(inp.shape) not in self._shapes._eager_shapes

    def evaluate(self, inp, target):
        """(loss, prec1) of one batch as device scalars; nothing is read back here."""
        with torch.no_grad():
            if not self.fused:
                out, loss, prec = self._eager(inp, target)
            else:
                key = (tuple(inp.shape), inp.dtype, tuple(target.shape), target.dtype)
                out, loss, prec = self._shapes(key, tuple(inp.shape), inp, target)
            self.last_logits = out
            return loss, prec


class Attacker:
    """Image-space L-inf PGD on the model in eval mode — the robust-accuracy counterpart of Evaluator, whose private weight
    copies and coefficient blocks it shares (refresh() rewrites both).  attack(inp, target) -> (x_adv, loss_adv, prec_adv) on the
    device.  The schedule is seg_attack_algo.adv_input's (Segmentation/attack_algo.py:86-105), built from pgd.py like it: pgd.start
    (the HOST draws the random start), `steps` projected sign steps, one clamp to [0, 1]; loss_adv / prec_adv are the criterion and
    top-1 precision of the model on x_adv.  eps and gamma are in pixel units ([0, 1] images).

    bf16 channels-last BasicBlock ResNets (ResNet-20s / -56s / -18) run fused: the forward is Evaluator's (one launch per convolution)
    with its activations kept, the backward one launch per convolution where a kernel has the form — the input gradient with the
    frozen BatchNorm + ReLU backward it runs into in its epilogue (ops.conv_dgrad_affine(any_kernel=True)), ops.conv_dgrad_dual where a
    residual joins, the two launches they stand for elsewhere — then the stem's input gradient on the general kernel, the
    normalisation's 1 / std and the sign step.  The whole attack (steps x (forward, loss, backward, step), the clamp, the final
    forward, loss and accuracy) is ONE hipGraph per batch shape, captured on the shape's second sight; nothing synchronises with the
    host.  Everything else (fp32, NCHW, another criterion, Bottleneck networks) runs attack_eager(): the same schedule through the
    model's own eval-mode autograd (resnet_s._BNEvalFn), which the fused path equals bit for bit.

    norm="l2": the same schedule under the L2 threat model — normalised-gradient steps projected onto the L2 ball of radius eps
    (pgd.step(norm="l2"), three launches inside the same graph), the host draws a Gaussian direction for the random start
    (pgd.start); eps and gamma are L2 lengths in the same pixel units.  norm="linf" (the default) is the attack described above."""

    def __init__(self, model, criterion, eps, gamma, steps, randinit=False, norm="linf"):
        pgd._check_norm(norm)
        self.norm = norm
        self.model, self.criterion = model, criterion
        self.eps, self.gamma, self.steps, self.randinit = float(eps), float(gamma), int(steps), bool(randinit)
        self.ev = evaluator_for(model, criterion)
        ev = self.ev
        self.fused = bool(ev.fused and not ev.pre and not ev.stem.stem7 and ev.stem.relu
                          and all(isinstance(blk, resnet_s.BasicBlock) for blk, _, _ in ev.blocks))
        self._shapes = _ShapeGraphs(self._fused_attack, self.attack_eager)
        self.inv_std = None

    def refresh(self):
        """Evaluator.refresh() plus the backward's operands: the transposed weight copies and 1 / std, rewritten in place."""
        self.ev.refresh()
        if not self.fused:
            return
        with torch.no_grad():
            for c in self.ev.convs[1:]:                 # (the stem's input gradient reads the untransposed weight)
                wt = c.w.permute(1, 0, 2, 3)
                if getattr(c, "wt", None) is None or c.wt.shape != wt.shape:
                    c.wt = torch.empty(wt.shape, dtype=wt.dtype, device=wt.device, memory_format=torch.channels_last)
                c.wt.copy_(wt)
            inv = (1.0 / self.ev.std.float()).contiguous()          # resnet_s._NormalizeFn's expression
            if self.inv_std is None:
                self.inv_std = inv
            else:
                self.inv_std.copy_(inv)

    # ------------------------------------------------------------------------------------------ fused passes
    def _forward(self, x):
        """Evaluator._forward with the activations the backward needs."""
        ev = self.ev
        xn = ops.normalize_nchw(x.contiguous().float(), ev.mean, ev.std, torch.bfloat16, True)
        h = ev.stem(xn)
        tape = []
        for blk, chain, sc in ev.blocks:
            a1 = chain[0](h)
            if sc is not None:
                res = sc(h)
            elif blk._sc_kind == "pad":
                res = blk.shortcut(h).contiguous(memory_format=torch.channels_last)
            else:
                res = h
            out = chain[1](a1, res)
            tape.append((h, a1, out))
            h = out
        xh = resnet_s._head_in(h)
        if not resnet_s._head_ok(xh, ev.lin):
            raise _Unfused
        logits, pooled = ops.head_forward(xh, ev.lin_w, ev.lin_b)
        return logits, (xn, tape, xh, pooled)

    def _backward(self, dlogits, saved):
        """d loss / d image (fp32 NCHW) from d loss / d logits: the eval-mode autograd graph's launches, fused where a kernel has the form."""
        ev = self.ev
        xn, tape, xh, pooled = saved
        g = ops.head_backward(dlogits, ev.lin_w, pooled, xh, True)
        pend = None                     # (gradient entering the block's last convolution's output, the shortcut's share)
        for bi in range(len(ev.blocks) - 1, -1, -1):
            blk, (c1, c2), sc = ev.blocks[bi]
            xin, a1, out = tape[bi]
            d_raw2, dres = pend if pend is not None else ops.affine_relu_backward(g, out, c2.coefs[2], True, True, True)
            d_raw1 = ops.conv_dgrad_affine(d_raw2, c2.wt, a1.shape[2:], c2.stride, c1.coefs[2], a1, any_kernel=True)
            if d_raw1 is None:
                d_raw1, _ = ops.affine_relu_backward(ops.conv_dgrad(d_raw2, c2.wt, a1.shape[2:], c2.stride), a1, c1.coefs[2], True)
            if sc is not None:          # projection shortcut: its BatchNorm (no ReLU), then its 1x1 input gradient
                d_sc, _ = ops.affine_relu_backward(dres, None, sc.coefs[2], False)
                add = ops.conv_dgrad(d_sc, sc.wt, xin.shape[2:], sc.stride)
            elif blk._sc_kind == "pad":  # option A: the middle channels of the share land on the even pixels
                pad = blk.shortcut.pad
                add = torch.zeros_like(xin)
                add[:, :, ::2, ::2] = dres[:, pad:pad + xin.shape[1]]
            else:
                add = dres
            # the two branches' sum at the block input, then the producer's (previous block's last / the stem's) BatchNorm + ReLU backward
            alpha = (ev.blocks[bi - 1][1][-1] if bi else ev.stem).coefs[2]
            pend = ops.conv_dgrad_dual(d_raw1, c1.wt, xin.shape[2:], c1.stride, add, alpha, xin)
            if pend is None:
                gin = ops.conv_dgrad(d_raw1, c1.wt, xin.shape[2:], c1.stride, addend=add)
                pend = ops.affine_relu_backward(gin, xin, alpha, True, True, bi > 0)
        st = ev.stem
        gx = ops.conv_general_dgrad(pend[0], st.w, xn.shape[2:], st.stride, int(st.conv.padding[0]), 1)
        return ops.affine_relu_backward(gx.float().contiguous(), None, self.inv_std, False)[0]

    def _fused_attack(self, x, target, u):
        x, x_adv = pgd.start(x, self.eps, self.randinit, u, norm=self.norm)
        for _ in range(self.steps):
            logits, saved = self._forward(x_adv)
            _, dlogits = ops.cross_entropy(logits, target)
            pgd.step(x_adv, self._backward(dlogits, saved), self.gamma, x, self.eps, True, norm=self.norm)
        pgd.clamp01_(x_adv)
        out = self.ev._forward(x_adv)
        return x_adv, self.criterion(out, target).float(), accuracy(out.float(), target)

    # ------------------------------------------------------------------------------------------- eager path
    def attack_eager(self, inp, target, u=None):
        """The same schedule through the model's own eval-mode forward and autograd (any dtype, layout and criterion)."""
        m = self.model
        x, x_adv = pgd.start(inp.detach().float().contiguous(), self.eps, self.randinit, u, norm=self.norm)
        crit = resnet_s.fused_criterion(self.criterion, m)
        loss_of = lambda t: crit(m(t, end_point=m.layer_number, start_point=0), target)
        for _ in range(self.steps):
            pgd.ascend(x_adv, loss_of, self.gamma, x, self.eps, True, norm=self.norm)
        pgd.clamp01_(x_adv)
        with torch.no_grad():
            out = m(x_adv, end_point=m.layer_number, start_point=0)
            return x_adv, self.criterion(out, target).float(), accuracy(out.float(), target)

    # ---------------------------------------------------------------------------------------------- attack
    def attack(self, inp, target):
        if self.model.training:
            raise ValueError("Attacker.attack: the model must be in eval mode (model.eval())")
        if inp.dim() != 4 or not inp.is_cuda:
            raise ops.AfanLibraryError("Attacker.attack: images [N, 3, H, W] on the MI355X")
        x = inp.detach().float().contiguous()
        # the host draws the random start (the reference's attack_algo.py:44), whichever path runs
        # (uniform for the L-inf box, a Gaussian direction for the L2 sphere)
        draw = torch.randn if self.norm == "l2" else torch.rand
        u = draw(x.shape).to(x.device, non_blocking=True) if self.randinit else None
        if not self.fused:
            return self.attack_eager(x, target, u)
        with torch.no_grad():
            return self._shapes((tuple(x.shape), tuple(target.shape), target.dtype), tuple(x.shape), x, target, u)


def evaluator_for(model, criterion):
    """The model's Evaluator for `criterion` (kept on the model, so its graphs serve every epoch)."""
    ev = getattr(model, "_afan_evaluator", None)
    if ev is None or ev.criterion is not criterion:
        ev = Evaluator(model, criterion)
        object.__setattr__(model, "_afan_evaluator", ev)
    return ev
