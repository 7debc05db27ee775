"""Detection feature-space operators and training iteration — names, signatures and error
behaviour of the reference's `Detection/attack_algo.py`, and the loop body of `Detection/train_aug_sat_muti_advt.py:70-172`:

    compute_loss(l1, l2, l3, l4)                                                                          :21-27
    PGD(x, image_batch, y, model, steps, eps, gamma, idx, randinit, clip)                                 :48-74
    rpn_roi_PGD(layer, rpn_roi_output_dict, y, model, steps, eps, gamma, randinit, clip, only_roi_loss)   :77-150
    adv_input(x, y, model, steps, eps, gamma, randinit, clip)                                             :153-178
    eval_PGD(x, y, model, steps, eps, gamma, idx, randinit, clip)                                         :207-233
    get_sample_points / mix_feature / tensor_clamp / linfball_proj                      (shared with attack_algo.py)
    det_train_step(model, optimizer, image_batch, bboxes_batch, labels_batch, loss_settings)   train_aug_sat_muti_advt.py:70-172
    det_train_phases(...)                         the same iteration as a generator with the backward cut at the backbone's output
    det_final_step / det_base_step / det_adv_step      train_aug_final.py:78-163, train_baseline.py:76-89, train_baseline_advtrain.py:75-93

`model` is anything that follows the reference's protocol (`Detection/model.py:40-185`):
`model.train().forward({'x', 'adv', 'out_idx', 'flag'}, bboxes, labels)` -> four per-image loss tensors, a feature map
(flag 'head') or the ROI dict ('roi_head').  The attacks are pgd.py's loop around that protocol; the mix / sample-point arithmetic
runs in libafan_hip.so; NMS and ROIAlign for the model's own layers are in det_ops.py; the Faster-RCNN model is det_model.py."""
import os

import torch

from . import frozen, ops, pgd
from .attack_algo import get_sample_points, linfball_proj, mix_feature, sample_points_mixed, tensor_clamp  # noqa: F401
from .det_ops import PGD, sum_of_means  # noqa: F401  (Detection/attack_algo.py:48-74)
from .resnet_s import _dense, _like_layout


def compute_loss(loss1, loss2, loss3, loss4):
    """:21-27: the sum of the four means."""
    return sum_of_means(loss1, loss2, loss3, loss4)


BATCH_LAYER3 = os.environ.get("AFAN_DET_BATCH_L3", "1") != "0"      # 0: every final pass runs its own layer3 (A/B, tests)
BATCH_ROI_HEAD = os.environ.get("AFAN_DET_BATCH_ROI", "1") != "0"    # 0: every final pass runs its own ROI head (A/B, tests)
SHARE_PROPOSALS = os.environ.get("AFAN_DET_SHARE_PROPOSALS", "1") != "0"   # 0: every tail on the clean conv4 map computes its own labels / proposals (A/B, tests)
BATCH_PGD_TAILS = os.environ.get("AFAN_DET_BATCH_PGD", "1") != "0"   # 0: the three one-step feature PGDs run their tails one by one (A/B, tests)


class NoiseAhead:
    """The image PGD's random start (:159: `torch.rand(x.shape)` on the CPU default generator, 1.6 M numbers for a 600 x 904 image:
    2.5 ms of host time with the device idle behind it) drawn at the END of the previous iteration instead, while the device still
    runs that iteration's backward.  The generator's stream is unchanged as long as the caller draws nothing from it between two
    iterations (a synthetic loop, a loader with its own generator): the iteration's first draw IS this one.  Opt-in
    (det_trainer.DetTrainer(noise_ahead=True)); `take(shape)` hands the stored draw back, or None."""

    def __init__(self):
        self.u = None

    def draw(self, shape):
        self.u = torch.rand(tuple(shape)).pin_memory()

    def take(self, shape):
        u, self.u = self.u, None
        return u if (u is not None and tuple(u.shape) == tuple(shape)) else None


def _pgd1_from_clean(model, col, idx, image_batch, y, eps, gamma):
    """`PGD(fm[idx - 1], ..., steps=1, idx=idx)` without a random start (:84-86) when the clean pass's own activations are at hand:
    its one forward runs the backbone's remaining stages on the CLEAN feature map — the numbers the clean ROI-head pass already
    computed — so only the part behind the backbone is run again (RPN, proposals, ROI head: their sampling draws are this call's
    own, as in the reference), and its gradient is carried back through the clean pass's stored activations with the
    input-gradient-only launches (frozen.stage_input_gradient).  Same values as PGD(); None where the stages did not run in the
    one-node form (fp32, NCHW: PGD() itself then runs)."""
    stages = [model.features.layer1, model.features.layer2, model.features.layer3]
    outs = [col.get(("out", i)) for i in (1, 2, 3)]
    if not all(frozen.stage_input_gradient(stages[i - 1], outs[i - 1]) for i in range(idx + 1, 4)):
        return None                  # (decided before anything is drawn from the host generator)
    x, x_adv = pgd.start(col[idx], eps, False)
    g = pgd.input_gradient(lambda t: sum_of_means(*model.train().forward({"x": image_batch, "adv": t, "out_idx": 3, "flag": "tail"}, y["bb"], y["lb"])),
                           col[3].detach().requires_grad_(True))
    for i in range(3, idx, -1):
        g = frozen.stage_input_gradient(stages[i - 1], outs[i - 1], g)
    pgd.step(x_adv, g, gamma, x, eps, False)
    return x_adv.requires_grad_(True)


def _pgd_three_from_clean(model, col, image_batch, y, specs, share=None):
    """The three one-step feature PGDs of :84-88 — `PGD(fm[0], idx=1)`, `PGD(fm[1], idx=2)`, `PGD(fm[2], idx=3)`, no random start — in ONE
    tail: each of them runs RPN + proposals + ROI head on the CLEAN conv4 map (their forwards differ only in the host generator's
    sampling draws) and takes the gradient back to its own layer.  Here the three tails are `Model.forward_heads_many` on three leaves of
    that map (the RPN trunk, ROIAlign, layer4 and the Linear pairs run once on three passes' rows; sampling pass by pass in the
    reference's order), one backward of the three losses' sum gives each leaf its own gradient (a pass's loss depends on its leaf only),
    and the first two are carried back through the clean pass's stored activations as in _pgd1_from_clean.  specs: [(idx, eps, gamma)]
    for idx 1, 2, 3.  None where the one-node stages or forward_heads_many are not there (the caller runs the three calls)."""
    if not hasattr(model, "forward_heads_many"):
        return None
    stages = [model.features.layer1, model.features.layer2, model.features.layer3]
    outs = [col.get(("out", i)) for i in (1, 2, 3)]
    if not all(frozen.stage_input_gradient(stages[i - 1], outs[i - 1]) for i in (2, 3)):
        return None                  # (decided before anything is drawn from the host generator)
    def loss_of(xins):
        res = model.train().forward_heads_many([{"x": image_batch, "adv": xi, "out_idx": 3, "flag": "tail"} for xi in xins], y["bb"], y["lb"],
                                               share=share)
        losses = [sum_of_means(*r) for r in res]
        total = losses[0]
        for l in losses[1:]:
            total = total + l
        return total
    grads = pgd.input_gradient(loss_of, [col[3].detach().requires_grad_(True) for _ in specs])
    advs = []
    for (idx, eps, gamma), g in zip(specs, grads):
        for i in range(3, idx, -1):
            g = frozen.stage_input_gradient(stages[i - 1], outs[i - 1], g)
        x, x_adv = pgd.start(col[idx], eps, False)
        pgd.step(x_adv, g, gamma, x, eps, False)
        advs.append(x_adv.requires_grad_(True))
    return advs


def rpn_roi_PGD(layer="roi", rpn_roi_output_dict=None, y=None, model=None, steps=1, eps=None, gamma=None, randinit=False,
                clip=False, only_roi_loss=True):
    """:77-150.  layer 'roi': perturbs rpn_roi_output_dict['roi_output_dict']['roi_feature_map'] in the dict (loss = the two
    proposal losses, or all four).  clip=True names an undefined `rpn_feature1` in the reference (:110) and raises
    NameError after the first step — so does this.  layer 'rpn': the reference runs `steps` forwards and never moves the
    feature (:129-146: the update is commented out) — the dict comes back with an unperturbed requires_grad copy."""
    d = rpn_roi_output_dict
    if layer == "roi":
        _, x_adv = pgd.start(d["roi_output_dict"]["roi_feature_map"], eps, randinit)
        d["roi_output_dict"]["roi_feature_map"] = x_adv

        def loss_of(t):
            d["roi_output_dict"]["roi_feature_map"] = t
            ao, at, pc, pt = model.train().forward({"adv": d, "out_idx": "roi_tail", "flag": "clean"}, y["bb"], y["lb"])
            return sum_of_means(pc, pt) if only_roi_loss else sum_of_means(ao, at, pc, pt)
        for _ in range(steps):
            pgd.ascend(x_adv, loss_of, gamma, None, None, False)
            if clip:
                raise NameError("name 'rpn_feature1' is not defined")
        d["roi_output_dict"]["roi_feature_map"] = x_adv.requires_grad_(True)
        return d
    if layer == "rpn":
        _, x_adv = pgd.start(d["rpn_feature_map_dict"]["rpn_feature"], eps, randinit)
        x_adv.requires_grad_(True)
        d["rpn_feature_map_dict"]["rpn_feature"] = x_adv
        for _ in range(steps):
            model.train().forward({"adv": d, "out_idx": "rpn_tail", "flag": "clean"}, y["bb"], y["lb"])
        return d
    assert False


# The image attack's last step and its final clamp in one launch (pgd.step(clamp=(0, 1)): afan_pgd_step_clamp) instead of the step,
# two fills and afan_tensor_clamp; the same bits.  The module attribute is read at call time.  Decided by the project's rule for every
# switch — on only where the iteration gains more than the two arms' combined min-max spread (tools/probe/det_adv_time.py,
# profiles/det_adv_time.jsonl; README "Detection PGD training").  Measured: the launch alone 0.047 ms against 0.100 ms at 8 x 3 x 600 x 904, but
# on a 30 - 68 ms iteration that gain (0.05 ms) is below every pair's spread (1.2 - 18 ms), so OFF; AFAN_DET_ADV_CLAMP=1 turns it on.
ADV_FUSED_CLAMP = os.environ.get("AFAN_DET_ADV_CLAMP", "0") == "1"


def adv_input(x=None, y=None, model=None, steps=3, eps=None, gamma=None, randinit=False, clip=False, noise_ahead=None, noise="host",
              start=None, clamp=True):
    """:153-178: image-space PGD under the sum of the four losses, clamped to [0, 1] at the end.  Additions, each with a default that
    keeps the reference's behaviour: noise ("host" | "device": where the random start is drawn, pgd.start); start: the iterate to
    continue from instead of x (+ the random start), as eval_PGD has it; clamp=False: no final clamp, so that a run can be cut into
    steps.  With ADV_FUSED_CLAMP the last step carries the clamp (steps = 0: one gradient-less launch)."""
    fresh = randinit and start is None
    # (the random start's draw may have been made ahead of time: NoiseAhead)
    u = noise_ahead.take(x.shape) if (fresh and noise == "host" and noise_ahead is not None) else None
    x, x_adv = pgd.start(x, eps, fresh, u, noise=noise)
    if start is not None:
        x_adv.copy_(start)
    loss_of = lambda t: compute_loss(*model.train().forward({"x": t, "adv": None, "out_idx": -1, "flag": "clean"}, y["bb"], y["lb"]))
    if not (clamp and ADV_FUSED_CLAMP):
        for _ in range(steps):
            pgd.ascend(x_adv, loss_of, gamma, x, eps, clip)
        return (pgd.clamp01_(x_adv) if clamp else x_adv).requires_grad_(True)
    for t in range(steps):
        pgd.ascend(x_adv, loss_of, gamma, x, eps, clip, clamp=(0.0, 1.0) if t == steps - 1 else None)
    if steps == 0:      # (:174-175 projects inside the loop only: no projection here)
        pgd.step(x_adv, None, 0.0, None, None, False, clamp=(0.0, 1.0))
    return x_adv.requires_grad_(True)


def eval_PGD(x, y=None, model=None, steps=3, eps=None, gamma=None, idx=1, randinit=False, clip=False, start=None):
    """:207-233: the image-space PGD of the robust evaluation (eval_rob_ori.py -> evaluator.py:90-128) under the sum of the four
    losses' means, train-mode forward, dict {'x': x_adv, 'adv': None, 'out_idx': 0, 'flag': 'clean'}; the random start is drawn on the
    host.  Unlike adv_input there is NO final clamp to [0, 1], and without `clip` nothing projects.  `idx` is accepted and unused, as
    in the reference.  start (an addition): the iterate to continue from instead of x (+ the random start): a run cut into pieces."""
    x, x_adv = pgd.start(x, eps, randinit and start is None)
    if start is not None:
        x_adv.copy_(start)
    loss_of = lambda t: compute_loss(*model.train().forward({"x": t, "adv": None, "out_idx": 0, "flag": "clean"}, y["bb"], y["lb"]))
    for _ in range(steps):
        pgd.ascend(x_adv, loss_of, gamma, x, eps, clip)
    return x_adv.requires_grad_(True)


# The layer-wise SAT evaluation's points in one launch (ops.sat_points_block) where the layout allows it; the module attribute is read at
# call time.  Decided by the project's rule for every switch — on only where one single-setting image gains more than the two arms'
# combined min-max spread (tools/probe/det_sat_time.py (c), profiles/det_sat_time.jsonl; README "Detection layer-wise SAT evaluation").
# Measured: 0.015 ms against a spread of 0.39 ms on a 31 ms image, so OFF; AFAN_DET_SAT_POINTS=1 turns it on.  The evaluator's table asks
# for the one launch itself (fused=True): there it replaces 16 launches, not three.
SAT_POINTS_FUSED = os.environ.get("AFAN_DET_SAT_POINTS", "0") == "1"


SAT_NUMBER = 5                                   # evaluator.py:154: get_sample_points(feature_map, feature_adv, 5)


def sat_layer_points(feature_map, feature_adv, settings, out_dtype=torch.float32, fused=None):
    """evaluator.py:154-159 for every (sat_layer, mix) of `settings`: `get_sample_points(feature_map, feature_adv, 5)[sat_layer]`, then
    with mix the REVERSED `mix_feature(point, feature_map)` — the point is normalised, the clean map's per-pixel channel statistics are
    the target — in out_dtype (the model's compute dtype: what the tail's entry would cast to).  The weight of point j is
    j * (1.0 / 4), a Python double, as the reference computes it.  fused (None: SAT_POINTS_FUSED, read at call time): one launch for all settings where
    the maps are channels-last or hw == 1; else, and in NCHW, the existing launches composed (ops.sat_points)."""
    settings = [(int(j), bool(m)) for j, m in settings]
    if any(not 0 <= j < SAT_NUMBER for j, _ in settings):
        raise ValueError(f"sat_layer: a sample point 0..{SAT_NUMBER - 1}")
    percent = 1.0 / (SAT_NUMBER - 1)
    px, py = _dense(feature_map.detach().float()), _dense(feature_adv.detach().float())
    if py.stride() != px.stride():
        py = _like_layout(py, px)
    return ops.sat_points(px, py, [j * percent for j, _ in settings], [m for _, m in settings], out_dtype,
                          fused=SAT_POINTS_FUSED if fused is None else bool(fused))


def sat_layer_point(feature_map, feature_adv, sat_layer, mix, out_dtype=torch.float32, fused=None):
    """One setting of sat_layer_points."""
    return sat_layer_points(feature_map, feature_adv, [(sat_layer, mix)], out_dtype, fused)[0]


def det_train_step(model, optimizer, image_batch, bboxes_batch, labels_batch, loss_settings=1):
    """One iteration of Detection/train_aug_sat_muti_advt.py:70-172 (see det_train_phases)."""
    out = {}
    for _ in det_train_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out, loss_settings=loss_settings):
        pass
    return out


def det_train_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out, *, loss_settings=1, cut=False, defer_step=False,
                     noise_ahead=None):
    """One iteration of Detection/train_aug_sat_muti_advt.py:70-172 as a generator: adversarial image (5 steps, randinit,
    clip), the three backbone feature maps and the ROI dict, three one-step feature PGDs (`multi-layer`), five SAT sample
    points of the deepest one with points 1 and 2 re-normalised by mix_feature (one fused launch), the one-step ROI feature
    PGD + mix_feature, eight forwards, and the weighted loss of :141-153 (loss_settings 1-4).

    cut=True (data-parallel callers, det_trainer.DetTrainer; needs a model with `cut_features`): the eight training forwards'
    graphs are cut at the backbone's output (the conv4 feature map every forward hands to the RPN and the ROI head), the joint
    backward runs in two parts — everything behind the cuts (RPN, ROIAlign, layer4, the two heads: 8 passes), then the
    backbone (layer3 / layer2: the passes that reach it) — and the generator yields "tail" in between: the gradients of
    layer4 / rpn / detection heads (the arena's suffix) are final there and their all-reduce can fly under the backbone's
    backward.  Same arithmetic: what the tails leave at the cuts enters the backbone graph as its output gradient."""
    y = {"bb": bboxes_batch, "lb": labels_batch}
    fwd = lambda d: model.train().forward(d, bboxes_batch, labels_batch)
    if hasattr(model, "begin_iteration"):
        model.begin_iteration()
    adv_image = adv_input(x=image_batch, y=y, model=model, steps=5, eps=(2.0 / 255), gamma=(0.3 / 255), randinit=True, clip=True,
                          noise_ahead=noise_ahead)
    col = None
    if getattr(model, "collects_head_features", False):
        # the three head passes (:78-80) and the clean ROI-head pass (:81) run the same backbone on the same images (frozen
        # BatchNorm, no dropout, no random draw before the RPN): the head passes' values are that pass's stage outputs
        col = {}
        rpn_share = {} if SHARE_PROPOSALS else None      # the clean pass's anchor labels / proposals / candidate lists: the feature PGDs' tails see the same map
        rr = fwd({"x": image_batch, "adv": None, "out_idx": "roi_head", "flag": "clean", "collect": col, "rpn_share": rpn_share})
        fm = [col[i] for i in (1, 2, 3)]
    else:
        if hasattr(model, "head_features"):      # prefixes of one another: one pass, no graph
            fm = model.train().head_features(image_batch, (1, 2, 3))
        else:
            fm = [fwd({"x": image_batch, "adv": None, "out_idx": i, "flag": "head"}).detach() for i in (1, 2, 3)]
        rr = fwd({"x": image_batch, "adv": None, "out_idx": "roi_head", "flag": "clean"})
    clean_sd = rr["roi_output_dict"]["roi_feature_map"].detach()
    fold = col is not None and os.environ.get("AFAN_DET_FOLD_PGD", "1") != "0"      # 0: PGD() as written (A/B, tests)
    three = (_pgd_three_from_clean(model, col, image_batch, y, [(1, 0.1 / 255, 0.001 / 255), (2, 0.1 / 255, 0.001 / 255), (3, 2.0 / 255, 1.0 / 255)],
                                   share=rpn_share if SHARE_PROPOSALS else None)
             if (fold and BATCH_PGD_TAILS) else None)
    if three is not None:
        adv1, adv2, adv3 = three
    else:
        adv1 = _pgd1_from_clean(model, col, 1, image_batch, y, 0.1 / 255, 0.001 / 255) if fold else None
        adv2 = _pgd1_from_clean(model, col, 2, image_batch, y, 0.1 / 255, 0.001 / 255) if fold else None
        if adv1 is None:
            adv1 = PGD(fm[0], image_batch, y=y, model=model, steps=1, eps=(0.1 / 255), gamma=(0.001 / 255), idx=1)
        if adv2 is None:
            adv2 = PGD(fm[1], image_batch, y=y, model=model, steps=1, eps=(0.1 / 255), gamma=(0.001 / 255), idx=2)
        adv3 = PGD(fm[2], image_batch, y=y, model=model, steps=1, eps=(2.0 / 255), gamma=(1.0 / 255), idx=3)
    pts = sample_points_mixed(fm[2].float(), adv3.detach(), 5, (True, True, False, False))       # :95-97 in one launch
    adv_rr = rpn_roi_PGD(rpn_roi_output_dict=rr, y=y, model=model, steps=1, eps=(2.0 / 255), gamma=(0.2 / 255), only_roi_loss=False)
    adv_sd = mix_feature(clean_sd.float(), adv_rr["roi_output_dict"]["roi_feature_map"].detach())
    adv_rr["roi_output_dict"]["roi_feature_map"] = adv_sd
    dicts = [{"x": adv_image.detach(), "adv": None, "out_idx": 0, "flag": "clean"},
             {"x": image_batch, "adv": adv1, "out_idx": 1, "flag": "tail"},
             {"x": image_batch, "adv": adv2, "out_idx": 2, "flag": "tail"}] + \
            [{"x": image_batch, "adv": pts[j], "out_idx": 3, "flag": "tail"} for j in (1, 2, 3, 4)] + \
            [{"adv": adv_rr, "out_idx": "roi_tail", "flag": "clean"}]
    if BATCH_LAYER3 and hasattr(getattr(model, "features", None), "forward_many"):
        # (round 6) the three passes that reach the backbone are independent of one another until their RPN: their layer3 runs once on the
        # three feature maps' batch (det_model backbone.forward_many), each pass then enters behind it like the sample-point passes do
        f3 = model.train().features.forward_many(dicts[:3])
        if f3 is not None:
            dicts[:3] = [{"x": image_batch, "adv": f, "out_idx": 3, "flag": "tail"} for f in f3]
    cuts = []
    def run_all():
        # (round 6) the seven passes in front of the ROI-tail pass are independent of one another: their ROI heads run as one
        if BATCH_ROI_HEAD and hasattr(model, "forward_heads_many"):
            outs = model.train().forward_heads_many(dicts[:7], bboxes_batch, labels_batch)
            return [compute_loss(*o) for o in outs] + [compute_loss(*fwd(d)) for d in dicts[7:]]
        return [compute_loss(*fwd(d)) for d in dicts]

    if cut:
        if not hasattr(model, "cut_features"):
            raise ops.AfanLibraryError("det_train_phases(cut=True) needs a model with cut_features() (det_model.Model)")
        with model.cut_features(cuts):
            L = run_all()
    else:
        L = run_all()
    loss_clean_adv = 0.9 * (0.2333 * (L[0] + L[3] + L[4] + L[5] + L[6]) + 0.1 * L[7]) + 0.05 * (L[1] + L[2])
    if loss_settings == 1:
        loss = loss_clean_adv
    elif loss_settings in (2, 3, 4):
        a, b = {2: (0.5, 0.5), 3: (0.4, 0.6), 4: (0.3, 0.7)}[loss_settings]
        loss = a * loss_clean_adv + b * L[0]
    else:
        assert False
    optimizer.zero_grad()
    loss.backward()
    if cut:
        yield "tail"            # behind the cuts everything is final
        live = [(f, c.grad) for f, c in cuts if c.grad is not None]
        if live:
            torch.autograd.backward([f for f, _ in live], [g for _, g in live])         # the backbone, every pass at once
    if noise_ahead is not None:      # every draw of this iteration is behind us; the device is busy with the backward just issued
        noise_ahead.draw(image_batch.shape)
    if not defer_step:
        optimizer.step()
    out.update({"loss": loss.detach(), "losses": torch.stack(L).detach(), "adv_image": adv_image.detach(), "adv1": adv1.detach(),
                "adv2": adv2.detach(), "adv3": adv3.detach(), "adv_sd": adv_sd.detach(), "fm3": fm[2], "cuts": len(cuts)})


def parse_mix_layer(mix_layer):
    """`--mix_layer` of Detection/train_aug_final.py:67-68: four 0/1 digits, one per sample point 1..4."""
    s = str(mix_layer)
    if len(s) != 4 or any(c not in "01" for c in s):
        raise ValueError(f"mix_layer: four 0/1 digits, one per sample point (train_aug_final.py:67-68), not {mix_layer!r}")
    return tuple(c == "1" for c in s)


def det_final_step(model, optimizer, image_batch, bboxes_batch, labels_batch, **settings):
    """One iteration of Detection/train_aug_final.py:78-163 (see det_final_phases)."""
    out = {}
    for _ in det_final_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out, **settings):
        pass
    return out


def det_final_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out, *, pertub_idx_se, mix_layer, gamma_se=0.5, gamma_sd=0.1,
                     sd_adv_loss_weight=0.5, only_roi_sd=False, mix_sd=False, noise_sd=0, randinit=False, clip=False, defer_step=False):
    """One iteration of Detection/train_aug_final.py:78-163 — the reference README's recipe — as a generator (it yields nothing: the
    two-part backward of det_train_phases is not built for it): the backbone feature map behind layer `pertub_idx_se` and the ROI dict
    (:78-85), a one-step feature PGD (eps 2/255, gamma_se/255, :87-95), a one-step ROI-feature PGD (gamma_sd/255, the two proposal
    losses or all four, :97-107), optionally mix_feature and noise (2u - 1) * gamma_sd * noise_sd on it (:111-114, u drawn from the host
    generator there), five sample points with points 1..4 re-normalised where the `mix_layer` digit is set (:117-126, one fused
    launch), six forwards (:128-146) and loss = (L0 + .. + L4) / 3 * (1 - w) + L5 / 3 * w (:156).  The host generator's draws come in
    the reference's order, pass by pass.  The sharing forms are det_train_phases', behind the same switches: the head pass's value
    from the clean ROI-head pass (`collect`) or head_features; layer3 once for the clean pass and the tails entering behind layer 1 or
    2 (BATCH_LAYER3); the ROI heads of the five passes in front of the ROI-tail pass as one (BATCH_ROI_HEAD)."""
    if pertub_idx_se not in (1, 2, 3):
        raise ValueError(f"pertub_idx_se: a backbone layer 1..3, not {pertub_idx_se!r}")
    idx = int(pertub_idx_se)
    mix = parse_mix_layer(mix_layer)
    y = {"bb": bboxes_batch, "lb": labels_batch}
    fwd = lambda d: model.train().forward(d, bboxes_batch, labels_batch)
    if hasattr(model, "begin_iteration"):
        model.begin_iteration()
    if getattr(model, "collects_head_features", False):
        col = {}
        rr = fwd({"x": image_batch, "adv": None, "out_idx": "roi_head", "flag": "clean", "collect": col})
        fm_se = col[idx]
    else:
        if hasattr(model, "head_features"):
            fm_se = model.train().head_features(image_batch, (idx,))[0]
        else:
            fm_se = fwd({"x": image_batch, "adv": None, "out_idx": idx, "flag": "head"}).detach()
        rr = fwd({"x": image_batch, "adv": None, "out_idx": "roi_head", "flag": "clean"})
    clean_sd = rr["roi_output_dict"]["roi_feature_map"].detach()
    adv_se = PGD(fm_se, image_batch, y=y, model=model, steps=1, eps=(2.0 / 255), gamma=(gamma_se / 255), idx=idx, randinit=randinit, clip=clip)
    adv_rr = rpn_roi_PGD(layer="roi", rpn_roi_output_dict=rr, y=y, model=model, steps=1, eps=(2.0 / 255), gamma=(gamma_sd / 255),
                         randinit=randinit, clip=clip, only_roi_loss=only_roi_sd)
    adv_sd = adv_rr["roi_output_dict"]["roi_feature_map"].detach()
    if mix_sd:
        adv_sd = mix_feature(clean_sd.float(), adv_sd)
    if noise_sd != 0:
        if not mix_sd:
            adv_sd = adv_sd.clone()
        ops.axpy_noise_(adv_sd, torch.rand(adv_sd.shape).to(adv_sd.device, non_blocking=True), gamma_sd * noise_sd)
    adv_rr["roi_output_dict"]["roi_feature_map"] = adv_sd
    pts = sample_points_mixed(fm_se.float(), adv_se.detach(), 5, mix)                     # :117-126 in one launch
    dicts = [{"x": image_batch, "adv": None, "out_idx": 0, "flag": "clean"}] + \
            [{"x": image_batch, "adv": pts[j], "out_idx": idx, "flag": "tail"} for j in (1, 2, 3, 4)] + \
            [{"adv": adv_rr, "out_idx": "roi_tail", "flag": "clean"}]
    if idx in (1, 2) and BATCH_LAYER3 and hasattr(getattr(model, "features", None), "forward_many"):
        f3 = model.train().features.forward_many(dicts[:5])
        if f3 is not None:
            dicts[:5] = [{"x": image_batch, "adv": f, "out_idx": 3, "flag": "tail"} for f in f3]
    if BATCH_ROI_HEAD and hasattr(model, "forward_heads_many"):
        L = [compute_loss(*o) for o in model.train().forward_heads_many(dicts[:5], bboxes_batch, labels_batch)] + [compute_loss(*fwd(dicts[5]))]
    else:
        L = [compute_loss(*fwd(d)) for d in dicts]
    w = sd_adv_loss_weight
    loss = ((L[0] + L[1] + L[2] + L[3] + L[4]) / 3.0) * (1 - w) + (L[5] / 3.0) * w
    optimizer.zero_grad()
    loss.backward()
    if not defer_step:
        optimizer.step()
    out.update({"loss": loss.detach(), "losses": torch.stack(L).detach(), "adv_se": adv_se.detach(), "adv_sd": adv_sd.detach(), "fm_se": fm_se})
    return
    yield


def det_base_step(model, optimizer, image_batch, bboxes_batch, labels_batch):
    """One iteration of Detection/train_baseline.py:76-89 (see det_base_phases)."""
    out = {}
    for _ in det_base_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out):
        pass
    return out


def det_base_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out, *, defer_step=False):
    """One iteration of Detection/train_baseline.py:76-89 as a generator (it yields nothing): one clean forward, the sum of the four
    losses' means, backward, the step."""
    if hasattr(model, "begin_iteration"):
        model.begin_iteration()
    four = model.train().forward({"x": image_batch, "adv": None, "out_idx": 0, "flag": "clean"}, bboxes_batch, labels_batch)
    loss = compute_loss(*four)
    optimizer.zero_grad()
    loss.backward()
    if not defer_step:
        optimizer.step()
    out.update({"loss": loss.detach(), "losses": torch.stack([t.detach().mean() for t in four])})
    return
    yield


def det_adv_step(model, optimizer, image_batch, bboxes_batch, labels_batch, **settings):
    """One iteration of Detection/train_baseline_advtrain.py:75-93 (see det_adv_phases)."""
    out = {}
    for _ in det_adv_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out, **settings):
        pass
    return out


def det_adv_phases(model, optimizer, image_batch, bboxes_batch, labels_batch, out, *, steps=1, eps=2.0, gamma=0.5, randinit=False, clip=False,
                   noise="host", noise_ahead=None, defer_step=False):
    """One iteration of Detection/train_baseline_advtrain.py:75-93 — PGD training, the model a robust mAP is compared against — as a
    generator (it yields nothing): adv_input on the batch with eps / 255 and gamma / 255 (`steps` attack passes, each a train-mode
    forward and an input gradient under dgrad_only on frozen BatchNorm: no parameter gradient, no running statistic, nothing left
    behind), ONE train-mode forward {'x': adv, 'adv': None, 'out_idx': -1, 'flag': 'clean'}, the sum of the four losses' means,
    zero_grad, backward, the step.  The host generator is read in the reference's order: the random start first (noise="host"), then
    each pass's sampling draws.  noise="device": the start is drawn inside its own launch from the device's generator (pgd.start), the
    host generator sees the sampling draws only, and the seed of the draw comes back as out["noise_seed"].  noise_ahead (host noise
    with randinit): the next iteration's start is drawn behind this iteration's backward (NoiseAhead).
    out: loss, losses (the four means), adv (the adversarial batch) and, with noise="device" and randinit, noise_seed."""
    y = {"bb": bboxes_batch, "lb": labels_batch}
    if hasattr(model, "begin_iteration"):
        model.begin_iteration()
    adv = adv_input(x=image_batch, y=y, model=model, steps=steps, eps=(eps / 255), gamma=(gamma / 255), randinit=randinit, clip=clip,
                    noise_ahead=noise_ahead, noise=noise)
    seed = getattr(adv, "_afan_noise_seed", None)
    adv = adv.detach()          # (the reference carries the clamp's graph back to the image: a gradient nobody reads)
    four = model.train().forward({"x": adv, "adv": None, "out_idx": -1, "flag": "clean"}, bboxes_batch, labels_batch)
    loss = compute_loss(*four)
    optimizer.zero_grad()
    loss.backward()
    if noise_ahead is not None and randinit and noise == "host":      # every draw of this iteration is behind us
        noise_ahead.draw(image_batch.shape)
    if not defer_step:
        optimizer.step()
    out.update({"loss": loss.detach(), "losses": torch.stack([t.detach().mean() for t in four]), "adv": adv})
    if seed is not None:
        out["noise_seed"] = seed
    return
    yield
