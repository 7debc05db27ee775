"""The frozen-BatchNorm ResNet bottleneck on the native sequencers, for both families that run it: Detection's backbone (BatchNorms
frozen by type, det_model.FrozenBatchNorm2d) and DeepLab's in eval mode (deeplab.FROZEN_EVAL).  One place owns

  * the coefficient block [4, C] of a frozen BatchNorm (`affine_coefs`, and its cached per-module form `bn_coefs`);
  * the launch plan of a block (`block_plan`: eligibility, ops.frozen_bottleneck_plan, one cache on the block with one validity
    stamp read from the live module attributes);
  * the autograd nodes over ops.frozen_bottleneck_fwd_plan / _bwd_plan: one per block (`_FrozenBlockFn`), one per stage
    (`_FrozenStageFn`, `_run_stage`, `stage_input_gradient`) and the stage replayed from hipGraphs (`_StageGraphs`);
  * the image end of the backbone as one node (`_FrozenStemFn`, `stem_node`: normaliser, 7x7 stem, frozen BatchNorm + ReLU, max pool)
    whose backward is ONE launch, behind the switch STEM_IMAGE_GRAD.

What differs between the callers are arguments of `block_plan` ("The frozen bottleneck path"); the switches stay with
their families (deeplab.FROZEN_EVAL / COEF_CACHE; AFAN_DET_BLOCK_NODE / _STAGE_NODE / _GRAPHS act on Detection's calls only)."""
import operator
import os

import torch
import torch.nn as nn

from . import ops
from .resnet_s import Conv2d, _accumulates_in_place, _Flags, _like_layout, _own_conv_ok, _WgradStream, dgrad_only


# ----------------------------------------------------------------------------------------------------- coefficient blocks
def _f32(t):
    return t.detach().float().contiguous()       # (a dense fp32 tensor comes back as it is)


def affine_coefs(weight, bias, running_mean, running_var, eps):
    """The ops.affine_coefs block [4, C] = mean | invstd | alpha | beta of a BatchNorm normalising with its running statistics:
    invstd = rsqrt(running_var + eps) in fp32, BatchNorm2d.fused's expression (the same values)."""
    return ops.affine_coefs(_f32(running_mean), torch.rsqrt(_f32(running_var) + eps), _f32(weight), _f32(bias))


def _bn_tensors(bn):
    p, b = bn._parameters, bn._buffers           # the live entries (a re-homed buffer, a dual-BN set swapped in: new tensors here)
    return p["weight"], p["bias"], b["running_mean"], b["running_var"]


def bn_coefs(bn, cache=True):
    """`affine_coefs` of the BatchNorm module `bn`, kept on the module until a tensor behind it changed (_version, address) or any
    BatchNorm was in training mode in between (_Flags.bn_epoch: the kernels move the running statistics through their own
    pointers).  cache False: rebuilt at this call."""
    ts = _bn_tensors(bn)
    key = None
    if cache:
        key = tuple(t._version for t in ts) + tuple(t.data_ptr() for t in ts) + (_Flags.bn_epoch,)
        hit = bn.__dict__.get("_frozen_coefs")
        if hit is not None and hit[0] == key:
            return hit[1]
    coefs = affine_coefs(*ts, bn.eps)
    bn.__dict__["_frozen_coefs"] = (key, coefs)
    return coefs


# ------------------------------------------------------------------------------------------------------------ block plans
class _ShapeOnly:
    """What the eligibility test looks at of a map that does not exist yet (a block's inner activations; the previous block's
    output inside a stage node)."""
    __slots__ = ("shape", "device", "dtype", "is_cuda")

    def __init__(self, shape, like):
        self.shape, self.device, self.dtype, self.is_cuda = torch.Size(shape), like.device, like.dtype, like.is_cuda

    def dim(self):
        return len(self.shape)

    def is_contiguous(self, memory_format=None):
        return True


def _layers(blk):
    """((conv1, conv2, conv3, projection | None), (bn1, bn2, bn3[, projection's])) from the block's live registrations."""
    m = blk._modules
    ds = m.get("downsample")
    if ds is None:
        return (m["conv1"], m["conv2"], m["conv3"], None), (m["bn1"], m["bn2"], m["bn3"])
    d = ds._modules
    return (m["conv1"], m["conv2"], m["conv3"], d["0"]), (m["bn1"], m["bn2"], m["bn3"], d["1"])


_version, _data_ptr = operator.attrgetter("_version"), torch.Tensor.data_ptr


def _stamp(convs, bns):
    """What a cached plan's pointers were read from, as it stands on the modules NOW: per convolution the master weight's version
    and the low-precision copy's address, per BatchNorm the versions and addresses of its four tensors, and the two epochs (an
    arena's SGD step and a training-mode BatchNorm write through pointers of their own).  Every lookup pays for this (Detection:
    388 a step), hence the C-level maps."""
    convs = [c for c in convs if c is not None]
    ts = []
    for b in bns:
        ts += _bn_tensors(b)
    return [_Flags.weight_epoch, _Flags.bn_epoch, *[c._parameters["weight"]._version for c in convs],
            *[c.lp_weight().data_ptr() for c in convs], *map(_version, ts), *map(_data_ptr, ts)]


def block_ok(convs, x, trains, pg):
    """Bias-free bf16 convolutions, each on the tuned kernels at the shape IT will see; with `trains`, weight gradients the
    sequencer can add straight into the arena (and no stash / side stream, which the sequencer does not know)."""
    c2 = convs[1]
    if not all(c is None or (c.bias is None and c.compute_dtype == torch.bfloat16) for c in convs):
        return False
    if tuple(c2.padding) != tuple(c2.dilation) or (c2.dilation[0] != 1 and c2.stride[0] != 1):
        return False
    n, _, h, w = x.shape
    ho, wo = (h - 1) // c2.stride[0] + 1, (w - 1) // c2.stride[0] + 1
    probes = (x, _ShapeOnly((n, c2.in_channels, h, w), x), _ShapeOnly((n, convs[2].in_channels, ho, wo), x), x)
    for c, t in zip(convs, probes):
        if c is None:
            continue
        if not _own_conv_ok(t, c.lp_weight(), c.stride, c.padding, c.dilation):
            return False
        if trains and not ops.conv_wgrad_supported(c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0]):
            return False
        if pg and c.weight.requires_grad and not (_accumulates_in_place(c.weight) and (
                c.weight.grad.is_contiguous(memory_format=torch.channels_last) or c.kernel_size[0] == 1)):
            return False
    return not (trains and (_Flags.wgrad_stash or _WgradStream.ON))


def block_plan(blk, x, trains=False, bn_ok=None, cache=True):
    """The ops.FrozenBlockPlan of the bottleneck `blk` (conv1, bn1, conv2, bn2, conv3, bn3, downsample; the 3x3's own dilation) for
    the bf16 channels-last input `x` (or its _ShapeOnly), or None where the one-node form does not apply — then the caller's
    layer-by-layer modules run.
      trains  the block's weights take gradients through the plan when _Flags.param_grads and grad mode are on (Detection);
              False: input gradients only (an eval-mode DeepLab);
      bn_ok   predicate every BatchNorm must pass to count as frozen (None: frozen by type);
      cache   False: eligibility, coefficient blocks and plan are rebuilt at this call (deeplab.COEF_CACHE = 0).
    Plans are kept on the block per (input shape, device, parameter-gradient mode, weight-gradient stash / side stream), each with
    the `_stamp` it was built under; a lookup whose stamp differs rebuilds that entry."""
    convs, bns = _layers(blk)
    if bn_ok is not None and not all(bn_ok(b) for b in bns):
        return None
    pg = bool(trains and _Flags.param_grads and torch.is_grad_enabled())
    if cache:
        key = (tuple(x.shape), x.device.index, pg, _Flags.wgrad_stash, _WgradStream.ON)
        stamp = _stamp(convs, bns)
        plans = blk.__dict__.get("_frozen_plans")
        if plans is None:
            plans = blk.__dict__["_frozen_plans"] = {}
        hit = plans.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
    plan = None
    if block_ok(convs, x, trains, pg):
        ks = tuple(bn_coefs(b, cache) for b in bns) + ((None,) if convs[3] is None else ())
        gws = tuple(c.weight.grad if (c is not None and pg and c.weight.requires_grad) else None for c in convs)
        plan = ops.frozen_bottleneck_plan(x, convs[0].out_channels, convs[1].stride[0],
                                          tuple(None if c is None else c.lp_weight() for c in convs), ks,
                                          tuple(None if c is None else c.lp_weight_t() for c in convs),
                                          tuple(None if k is None else k[2] for k in ks), gws, dilation=convs[1].dilation[0])
    if cache:
        plans[key] = (stamp, plan)
    return plan


class FrozenBottleneck(nn.Module):
    """What the two families' bottlenecks share (torchvision v1.5: the 3x3 carries the stride, and the dilation): the layers, in
    the reference's registration and construction order, with the BatchNorm class `norm` of the subclass; the plan cache leaves
    with pickling."""
    expansion = 4
    norm = None

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, kernel_size=1, stride=1, bias=False)
        self.bn1 = self.norm(planes)
        self.conv2 = Conv2d(planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = self.norm(planes)
        self.conv3 = Conv2d(planes, planes * 4, kernel_size=1, stride=1, bias=False)
        self.bn3 = self.norm(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def __getstate__(self):
        # launch plans hold ctypes pointer objects (not picklable, and meaningless in a copy): a deepcopy / torch.save of the
        # module starts without them and rebuilds them on its first forward
        d = dict(self.__dict__)
        d.pop("_frozen_plans", None)
        d.pop("_params", None)
        return d


# ---------------------------------------------------------------------------------------------------------- autograd nodes
class _FrozenBlockFn(torch.autograd.Function):
    """A frozen-BatchNorm bottleneck (Detection: backbone/resnet101_ori.py:78-127; Segmentation: DeepLab's eval-mode bottlenecks,
    atrous ones included, deeplab.Bottleneck) as ONE autograd node on the bf16 channels-last path:
    the same launches as the layer-by-layer form — three (four) tuned convolutions, three (four) fused affine(+residual)
    (+ReLU) launches forward; affine backward, input gradient and weight gradient per layer backward, the identity shortcut's
    gradient added in the first convolution's dgrad epilogue — but one `Function.apply`, one backward node and ONE native call
    each way (ops.frozen_bottleneck_fwd_plan / _bwd_plan: afan_frozen_bottleneck_fwd / _bwd issue the launches from C++) instead of seven of each: the Detection
    iteration is bound by Python dispatch (2 600 applies per iteration before this node)."""
    ON = os.environ.get("AFAN_DET_BLOCK_NODE", "1") != "0"      # Detection's switch (det_model.Bottleneck reads it); 0: layer-by-layer autograd nodes (A/B)

    @staticmethod
    def forward(ctx, x, blk, plan, *params):
        out, a1, a2 = ops.frozen_bottleneck_fwd_plan(x, plan)
        ctx.plan = plan
        ctx.save_for_backward(x, a1, a2, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, a1, a2, out = ctx.saved_tensors
        g = _like_layout(g, out)
        if g.dtype != out.dtype:
            g = g.to(out.dtype)
        dx = ops.frozen_bottleneck_bwd_plan(g, x, a1, a2, out, ctx.plan, ctx.needs_input_grad[0])
        return (dx, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


def _stage_backward(plans, saved, g, want_dx):
    """The blocks of a stage backwards.  Block i + 1's input is block i's output, so the first step of block i's backward — the
    gradient masked by that output's ReLU, once as it is (the shortcut's share) and once times the last BatchNorm's alpha — rides in
    the epilogue of block i + 1's last input-gradient launch (ops.frozen_bottleneck_bwd_plan `prev`): no launch of its own."""
    pre = None
    for i in range(len(plans) - 1, -1, -1):
        x, a1, a2, out = saved[4 * i:4 * i + 4]
        res = ops.frozen_bottleneck_bwd_plan(g if pre is None else None, x, a1, a2, out, plans[i], i > 0 or want_dx, pre=pre,
                                             prev=plans[i - 1] if i > 0 else None)
        if i > 0:
            pre = res
        else:
            g = res
    return g


def _stage_plans(stage, x):
    """One plan per block of `stage` (an nn.Sequential of bottlenecks with a `frozen_plan(x)` method), each for the shape it will
    see behind `x`, or None when a block declines."""
    plans, probe = [], x
    for blk in stage:
        plan = blk.frozen_plan(probe)
        if plan is None:
            return None
        plans.append(plan)
        probe = _ShapeOnly((plan.n, plan.co, plan.ho, plan.wo), x)
    return plans


def _dgrad_plans(stage, out):
    """The input-gradient-only launch plans of `stage` for the activations a one-node forward left on `out`, or None."""
    saved = getattr(out, "_afan_stage_saved", None)
    if saved is None or len(saved) != 4 * len(stage) - 1:          # (every activation but `out` itself: no reference cycle)
        return None
    with dgrad_only():
        return _stage_plans(stage, saved[0])


def stage_input_gradient(stage, out, g=None):
    """d(loss)/d(stage input) from g = d(loss)/d(stage output) and the activations a forward of `stage` left on its output tensor
    `out` (`_FrozenStageFn`), with no parameter gradient touched (the dgrad-only launch plans) — what back-propagating g through
    a SECOND forward of the same stage on the same input under `resnet_s.dgrad_only()` would give, bit for bit, without that
    forward.  g None: only answers whether that is possible (True / False); None when it is not."""
    plans = _dgrad_plans(stage, out)
    if g is None:
        return plans is not None
    if plans is None:
        return None
    saved = out._afan_stage_saved + (out,)
    last = saved[-1]
    g = _like_layout(g, last)
    if g.dtype != last.dtype:
        g = g.to(last.dtype)
    with torch.no_grad():
        return _stage_backward(plans, saved, g, True)


class _FrozenStageFn(torch.autograd.Function):
    """A whole stage (layer1 .. layer4: 3 / 4 / 23 / 3 frozen-BatchNorm bottlenecks) as ONE autograd node: the same native calls
    as one `_FrozenBlockFn` per block, issued in a loop — the per-node cost of `Function.apply` and of the engine's scheduling
    (~50 us a block and direction on this host) is paid once per stage instead of 33 times per backbone pass, 27 passes per
    Detection iteration."""
    ON = os.environ.get("AFAN_DET_STAGE_NODE", "1") != "0"      # Detection's switch (only its backbone calls _run_stage); 0: one node per block (A/B)

    @staticmethod
    def forward(ctx, x, plans, *params):
        saved = []
        for plan in plans:
            out, a1, a2 = ops.frozen_bottleneck_fwd_plan(x, plan)
            saved += [x, a1, a2, out]
            x = out
        ctx.plans = plans
        ctx.save_for_backward(*saved)
        if any(ctx.needs_input_grad):             # (references only, and only where a graph keeps them alive anyway:
            # stage_input_gradient reuses a clean pass's activations.)  Everything BUT the output itself: a tuple holding
            # `x` on `x.__dict__` is a cycle that only the cyclic collector frees — the stage's activations would outlive
            # their graph by however long that takes (~4 GB resident in a CPU simulation)
            x._afan_stage_saved = tuple(saved[:-1])
        return x

    @staticmethod
    def backward(ctx, g):
        saved, plans = ctx.saved_tensors, ctx.plans
        last = saved[-1]
        g = _like_layout(g, last)
        if g.dtype != last.dtype:
            g = g.to(last.dtype)
        g = _stage_backward(plans, saved, g, ctx.needs_input_grad[0])
        return (g, None) + (None,) * (len(ctx.needs_input_grad) - 2)


class _StageInst:
    __slots__ = ("x", "out", "saved", "fwd", "bwd", "g", "dx", "busy", "plans", "want_dx")


class _StageGraphs:
    """Captured hipGraphs of whole backbone stages (forward, and backward on first use) per (stage, input shape, plan signature,
    gradient mode): the Detection iteration is shaped by its proposals everywhere EXCEPT in the backbone, whose 27 passes per
    iteration issue the same ~30 native calls each from Python — replayed here as one graph launch each way.  An instance owns
    its activations (static buffers of the graph's pool), so a forward whose backward is still pending keeps its instance
    busy and the next forward of the same kind takes (or captures) another; `begin_iteration()` frees them all (forwards whose
    graph autograd never walks back: the detached head passes, the ROI dict's pass).  More than MAX_INST busy instances of one
    kind (a caller that never calls begin_iteration): the eager stage node runs instead."""
    # Measured (MI355X, 600 x 904, 20 iterations, interleaved): 123.7 / 120.4 ms replayed against 119.9 / 111.9 ms eager, losses
    # identical — after the per-block launch plans the backbone's launch cost is no longer what the iteration waits for (its ~50
    # host reads of proposal / sample counts are): OFF by default, AFAN_DET_GRAPHS=1 switches it on.
    ON = os.environ.get("AFAN_DET_GRAPHS", "0") == "1"
    MAX_INST = 12
    cache = {}
    warm = {}                                  # key -> eager runs seen (workspaces must exist before a capture)

    @classmethod
    def begin_iteration(cls):
        for insts in cls.cache.values():
            for it in insts:
                it.busy = False

    @classmethod
    def get(cls, stage, x, plans, want_dx):
        key = (id(stage), want_dx, tuple(p.sig for p in plans))
        if cls.warm.get(key, 0) < 2:           # two eager passes first
            cls.warm[key] = cls.warm.get(key, 0) + 1
            return None
        insts = cls.cache.setdefault(key, [])
        for it in insts:
            if not it.busy:
                return it
        if len(insts) >= cls.MAX_INST or torch.cuda.is_current_stream_capturing():
            return None
        it = cls._capture_fwd(x, plans, want_dx)
        insts.append(it)
        return it

    @classmethod
    def _capture_fwd(cls, x, plans, want_dx):
        it = _StageInst()
        it.plans, it.want_dx, it.busy, it.bwd, it.g, it.dx = plans, want_dx, False, None, None, None
        it.x = torch.empty_like(x)
        torch.cuda.synchronize(x.device)
        g = torch.cuda.CUDAGraph()
        # A PRIVATE memory pool per graph: instances are replayed in any order and keep their activations from forward to backward,
        # so a temporary freed inside one capture must never be handed to another graph as something long-lived (a shared pool
        # assumes graphs replay in capture order).
        with torch.no_grad(), ops.capturing(g):
            cur, saved = it.x, []
            for plan in plans:
                out, a1, a2 = ops.frozen_bottleneck_fwd_plan(cur, plan)
                saved += [cur, a1, a2, out]
                cur = out
        it.saved, it.out, it.fwd = saved, cur, g
        return it

    @classmethod
    def capture_bwd(cls, it):
        it.g = torch.empty_like(it.out)
        torch.cuda.synchronize(it.out.device)
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), ops.capturing(g):       # (runs on the engine's thread; private pool)
            cur = _stage_backward(it.plans, it.saved, it.g, it.want_dx)
        it.dx, it.bwd = cur, g


class _GraphedStageFn(torch.autograd.Function):
    """`_FrozenStageFn` as two graph replays (see _StageGraphs)."""

    @staticmethod
    def forward(ctx, x, inst, *params):
        inst.x.copy_(x, non_blocking=True)
        inst.fwd.replay()
        inst.busy = True
        ctx.inst = inst
        return inst.out.detach()

    @staticmethod
    def backward(ctx, g):
        it = ctx.inst
        if it.bwd is None:
            _StageGraphs.capture_bwd(it)
        it.g.copy_(g, non_blocking=True)          # (any dtype / layout of g: copy_ converts)
        it.bwd.replay()
        it.busy = False
        dx = it.dx.detach() if (it.want_dx and it.dx is not None) else None
        return (dx, None) + (None,) * (len(ctx.needs_input_grad) - 2)


def _run_stage(stage, x):
    """`stage(x)` for an nn.Sequential of bottlenecks: one `_FrozenStageFn` node when every block takes the one-call form at the
    shape it will see, else block by block."""
    if not (_FrozenStageFn.ON and x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_cuda and x.is_contiguous(memory_format=torch.channels_last)):
        return stage(x)
    plans = _stage_plans(stage, x)
    if plans is None:
        return stage(x)
    params = getattr(stage, "_stage_params", None)
    if params is None:
        params = stage._stage_params = tuple(p for blk in stage for p in blk._block_params())
    if _StageGraphs.ON:
        grad_on = torch.is_grad_enabled()
        inst = _StageGraphs.get(stage, x, plans, bool(grad_on and x.requires_grad))
        if inst is not None:
            if not grad_on:                          # (no graph to build: replay and hand the buffer out; freed by begin_iteration)
                inst.x.copy_(x, non_blocking=True)
                inst.fwd.replay()
                inst.busy = True
                return inst.out.detach()
            return _GraphedStageFn.apply(x, inst, *params)
    return _FrozenStageFn.apply(x, tuple(plans), *params)


# ------------------------------------------------------------------------------------------------------- the image end
# The stem of a frozen-BatchNorm backbone under an image attack (normaliser -> conv1 7x7 / 2 -> bn1 + ReLU -> max pool 3 / 2 / 1) as ONE
# autograd node whose backward is ONE launch (ops.frozen_stem_image_grad) instead of six (pool backward, affine backward, the 1x1 MFMA
# problem into a 41 MB column tensor at 600 x 904, col2im, the normaliser's division, a cast).  Off by default, read at call time; only
# det_eval.RobustEvaluator turns it on (`stem_image_grad()`), for the duration of its attack: Detection training's adv_input,
# Segmentation's image PGD and infer.Attacker keep the layer-by-layer nodes and their bits (the one-launch form rounds the gradient
# once where the chain rounds it four times).
STEM_IMAGE_GRAD = os.environ.get("AFAN_STEM_IMAGE_GRAD", "0") == "1"


class stem_image_grad:
    """`with frozen.stem_image_grad(True):` sets the switch for the block."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global STEM_IMAGE_GRAD
        self.old, STEM_IMAGE_GRAD = STEM_IMAGE_GRAD, self.on
        return self

    def __exit__(self, *exc):
        global STEM_IMAGE_GRAD
        STEM_IMAGE_GRAD = self.old
        return False


class _FrozenStemFn(torch.autograd.Function):
    """`BottleneckResNet._stem` on an image that carries a gradient: the forward issues that method's launches (normalise; im2col and
    the 1x1 MFMA problem of deeplab._Stem7Fn; the fused affine + ReLU; the max pool) and gives its bits, keeping the post-ReLU map y1
    instead of the column tensor; the backward is afan_frozen_stem_image_grad.  Input gradient only."""

    @staticmethod
    def forward(ctx, x, mean, std, w_lp, coefs):
        xn = ops.normalize_nchw(x.detach().contiguous().float(), mean, std, torch.bfloat16, True)
        cols = ops.conv_stem7_im2col(xn)
        k = cols.shape[1]
        wp = torch.zeros((64, k, 1, 1), dtype=torch.bfloat16, device=x.device)
        wp.view(64, k)[:, :147] = w_lp.permute(0, 2, 3, 1).reshape(64, 147)
        y1 = ops.affine_apply(ops.conv_fwd(cols, wp.contiguous(memory_format=torch.channels_last), 1), coefs, None, True)
        out, _ = ops.maxpool2d(y1, 3, 2, 1, want_idx=False)
        ctx.w_lp, ctx.alpha, ctx.in_hw = w_lp, coefs[2], tuple(x.shape[2:])
        ctx.inv_std = (1.0 / std.float()).contiguous()
        ctx.save_for_backward(y1, out)
        return out

    @staticmethod
    def backward(ctx, g):
        y1, out = ctx.saved_tensors
        g = _like_layout(g, out)
        if g.dtype != out.dtype:
            g = g.to(out.dtype)
        return ops.frozen_stem_image_grad(g, y1, ctx.w_lp, ctx.alpha, ctx.inv_std, ctx.in_hw), None, None, None, None


def stem_node(net, x, direct=False):
    """`net._stem(x)` as one `_FrozenStemFn` node, or None where that form does not apply: the switch is off, the image carries no
    gradient, the path is not bf16 channels-last, bn1 is not frozen by type, conv1 would take a weight gradient, or the stem runs its
    direct kernels (`direct`: deeplab._Stem7Fn.DIRECT)."""
    if not (STEM_IMAGE_GRAD and not direct and torch.is_grad_enabled() and x.requires_grad and x.is_cuda and x.dim() == 4 and x.shape[1] == 3):
        return None
    conv, bn, norm, pool = net.conv1, net.bn1, net.normal, net.maxpool
    if not (conv.compute_dtype == torch.bfloat16 and norm.channels_last and norm.out_dtype == torch.bfloat16 and conv.bias is None
            and callable(getattr(bn, "_coefs", None)) and (pool.kernel_size, pool.stride, pool.padding) == (3, 2, 1)):
        return None
    if (_Flags.param_grads and conv.weight.requires_grad) or bn.weight.requires_grad or bn.bias.requires_grad:
        return None
    w = conv.lp_weight()
    if not (tuple(w.shape) == (64, 3, 7, 7) and w.dtype == torch.bfloat16 and w.is_contiguous(memory_format=torch.channels_last)
            and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (3, 3)):
        return None
    return _FrozenStemFn.apply(x, norm.mean, norm.std, w.detach(), bn._coefs())
