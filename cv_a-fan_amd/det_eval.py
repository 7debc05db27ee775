"""Detection evaluation: the VOC 2007 mean AP of the reference (Detection/voc_eval.py, dataset/voc2007.py:118-161, evaluator.py:20-47,
eval.py) on in-memory arrays, the evaluator around Model.forward in eval mode, the robust evaluator (evaluator.py:90-128: an image PGD
in front of that forward) and the drivers of eval.py and eval_rob_ori.py.

The metric runs on the host in numpy, float64, operation by operation as the reference does.  What the reference does on the way
is part of its number and kept:
  * detections make a round trip through `comp3_det_test_{category}.txt` written with `{:f}`: confidences and coordinates are rounded to
    six decimals before they are sorted and matched (`round_trip`); with a results directory the files are written as well;
  * the ground truth of the matching is the XML's raw integer box (voc_eval.py:23-26, no `- 1`) while detections come from 0-based
    boxes divided by the scale;
  * difficult objects stay in the ground truth: a detection whose best match is one counts neither way, and npos counts the others;
  * `np.argsort(-confidence)`, `np.maximum(tp + fp, eps)`, the 11-point metric;
  * a class without any detection gets AP 0 (voc2007.py:138-139: the reference's indexing of an empty array raises)."""
import argparse
import os
import time
import uuid
import warnings

import numpy as np

from .det_data import CATEGORY_TO_LABEL_DICT

LABEL_TO_CATEGORY_DICT = {v: k for k, v in CATEGORY_TO_LABEL_DICT.items()}
NUM_CLASSES = 21
MIN_PROB = 0.05                           # evaluator.py:35


def round_trip(v):
    """A value written with `{:f}` and read back (voc2007.py:157 -> voc_eval.py:140-141)."""
    return float('{:f}'.format(v))


def voc_ap(rec, prec, use_07_metric=False):
    """voc_eval.py:31-62: the 11-point average of the VOC 2007 devkit (the largest precision at recall >= 0, 0.1, ..., 1, each
    divided by 11 and added in that order; 0 where no recall reaches the point), or the area under the precision envelope."""
    if use_07_metric:
        total = 0.
        for point in np.arange(0., 1.1, 0.1):
            reached = rec >= point
            best = 0 if np.sum(reached) == 0 else np.max(prec[reached])
            total = total + best / 11.
        return total
    r = np.concatenate(([0.], rec, [1.]))
    p = np.concatenate(([0.], prec, [0.]))
    for k in range(p.size - 1, 0, -1):                      # the envelope: every precision at least the ones right of it
        p[k - 1] = np.maximum(p[k - 1], p[k])
    steps = np.where(r[1:] != r[:-1])[0]
    return np.sum((r[steps + 1] - r[steps]) * p[steps + 1])


def _overlaps(gt, det):
    """IoU of one detection with an image's ground-truth boxes [g, 4], pixel-inclusive (+ 1), float64, in voc_eval.py:162-175's order
    of operations: (detection area + ground-truth areas) - intersections."""
    w = np.maximum(np.minimum(gt[:, 2], det[2]) - np.maximum(gt[:, 0], det[0]) + 1., 0.)
    h = np.maximum(np.minimum(gt[:, 3], det[3]) - np.maximum(gt[:, 1], det[1]) + 1., 0.)
    inter = w * h
    union = ((det[2] - det[0] + 1.) * (det[3] - det[1] + 1.) + (gt[:, 2] - gt[:, 0] + 1.) * (gt[:, 3] - gt[:, 1] + 1.) - inter)
    return inter / union


def voc_eval(ground_truth, label, det_image_ids, det_confidence, det_boxes, ovthresh=0.5, use_07_metric=False):
    """voc_eval.py:120-198 for one class.  ground_truth: {image id: (classes int64 [g], difficult bool [g], boxes int64 [g, 4] = the
    XML's xmin, ymin, xmax, ymax)} over every image of the list; det_*: the class's detections as read back from the results file
    (`round_trip` applied).  -> (rec, prec, ap).  No detection at all raises IndexError, as the reference's indexing of its empty
    array does (VOC2007.evaluate turns it into AP 0)."""
    per_image, npos = {}, 0
    for image_id, (classes, difficult, boxes) in ground_truth.items():
        own = np.asarray(classes).reshape(-1) == label
        hard = np.asarray(difficult).reshape(-1)[own].astype(bool)
        npos = npos + int(np.sum(~hard))                        # difficult objects are nobody's positive
        per_image[image_id] = (np.asarray(boxes).reshape(-1, 4)[own].astype(float), hard, [False] * int(own.sum()))

    if len(det_image_ids) == 0:
        raise IndexError("no detection of this class")
    confidence = np.array([float(v) for v in det_confidence])
    order = np.argsort(-confidence)
    dets = np.array([[float(v) for v in row] for row in det_boxes])[order, :]
    ids = [det_image_ids[k] for k in order]

    tp, fp = np.zeros(len(ids)), np.zeros(len(ids))
    for k, image_id in enumerate(ids):
        gt, hard, claimed = per_image[image_id]
        best, arg = -np.inf, -1
        if gt.size > 0:
            iou = _overlaps(gt, dets[k, :].astype(float))
            best, arg = np.max(iou), np.argmax(iou)
        if not best > ovthresh:
            fp[k] = 1.
        elif hard[arg]:
            pass                                                # the best match is a difficult object: neither true nor false
        elif claimed[arg]:
            fp[k] = 1.                                          # a duplicate of an object already found
        else:
            tp[k] = 1.
            claimed[arg] = True

    fp, tp = np.cumsum(fp), np.cumsum(tp)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # npos = 0 (a class without ground truth): the reference divides by zero too
        rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def result_line(image_id, prob, bbox):
    """voc2007.py:157-158"""
    return '{:s} {:f} {:f} {:f} {:f} {:f}\n'.format(image_id, prob, bbox[0], bbox[1], bbox[2], bbox[3])


def write_results(path_to_results_dir, image_ids, bboxes, classes, probs):
    """voc2007.py:151-161: one `comp3_det_test_{category}.txt` per foreground class."""
    files = {c: open(os.path.join(path_to_results_dir, 'comp3_det_test_{:s}.txt'.format(LABEL_TO_CATEGORY_DICT[c])), 'w')
             for c in range(1, NUM_CLASSES)}
    try:
        for image_id, bbox, cls, prob in zip(image_ids, bboxes, classes, probs):
            files[cls].write(result_line(image_id, prob, bbox))
    finally:
        for f in files.values():
            f.close()


def evaluate_detail(ground_truth, image_ids, bboxes, classes, probs, path_to_results_dir=None):
    """VOC2007.evaluate (voc2007.py:118-149) -> (mean_ap, detail, {label: (rec, prec, ap)}); rec and prec are None for a class whose AP
    is the reference's `except IndexError` 0."""
    if path_to_results_dir is not None:
        write_results(path_to_results_dir, image_ids, bboxes, classes, probs)
    per_class = {c: ([], [], []) for c in range(1, NUM_CLASSES)}
    for image_id, bbox, cls, prob in zip(image_ids, bboxes, classes, probs):
        ids, conf, bbs = per_class[cls]
        ids.append(image_id)
        conf.append(round_trip(prob))
        bbs.append([round_trip(bbox[0]), round_trip(bbox[1]), round_trip(bbox[2]), round_trip(bbox[3])])
    results, class_to_ap_dict = {}, {}
    for c in range(1, NUM_CLASSES):
        try:
            rec, prec, ap = voc_eval(ground_truth, c, *per_class[c], ovthresh=0.5, use_07_metric=True)
        except IndexError:
            rec, prec, ap = None, None, 0
        results[c] = (rec, prec, ap)
        class_to_ap_dict[c] = ap
    mean_ap = np.mean([v for k, v in class_to_ap_dict.items()]).item()
    detail = ''
    for c in range(1, NUM_CLASSES):
        detail += '{:d}: {:s} AP = {:.4f}\n'.format(c, LABEL_TO_CATEGORY_DICT[c], class_to_ap_dict[c])
    return mean_ap, detail, results


def evaluate(ground_truth, image_ids, bboxes, classes, probs, path_to_results_dir=None):
    """VOC2007.evaluate -> (mean_ap, detail)."""
    mean_ap, detail, _ = evaluate_detail(ground_truth, image_ids, bboxes, classes, probs, path_to_results_dir)
    return mean_ap, detail


# ------------------------------------------------------------------------------------ the evaluator
class Evaluator:
    """evaluator.py:12-47.  loader: a det_data.DetDeviceLoader(train=False, batch=1) over the images of `ground_truth` =
    (image ids, {image id: (classes, difficult, raw boxes)}) in list order.  Per image: the eval-mode forward with the 0.05 bound
    passed down as min_prob, the boxes divided by the image's scale on the device, and ONE copy to the host of boxes | probs."""

    def __init__(self, loader, ground_truth, results_dir=None):
        if loader.train or loader.batch != 1:
            raise ValueError("do not use batch size more than 1 on evaluation: the loader is DetDeviceLoader(train=False, batch=1)")
        self.loader = loader
        self.image_ids, self.ground_truth = ground_truth
        if len(self.image_ids) != loader.n:
            raise ValueError("the ground truth names one image per image of the loader")
        self.results_dir = results_dir

    def attack(self, model, index, image_batch, bboxes_batch, labels_batch):
        """The image the eval-mode forward sees for image `index` of the list: the clean one here."""
        return image_batch

    def eval_inputs(self, model, index, image_batch, bboxes_batch, labels_batch):
        """The dict of the eval-mode forward for image `index` of the list (called with gradients as the caller left them)."""
        image_batch = self.attack(model, index, image_batch, bboxes_batch, labels_batch)
        return {"x": image_batch, "adv": None, "out_idx": None, "flag": 'clean', "min_prob": MIN_PROB}

    @staticmethod
    def score(model, lists, image_id, inputs_all, scale_batch):
        """One eval-mode forward, the boxes divided by the scale, the image's one host copy; appends to lists = (ids, boxes, classes, probs)."""
        import torch
        all_image_ids, all_bboxes, all_classes, all_probs = lists
        with torch.no_grad():
            bboxes, classes, probs, batch_indices = model.eval().forward(inputs_all)
            bboxes = bboxes / scale_batch[batch_indices.to(scale_batch.device)].unsqueeze(dim=-1).expand_as(bboxes)
            host = torch.cat([bboxes, probs.unsqueeze(dim=-1).to(bboxes.dtype)], dim=1).cpu()       # the image's one copy
            classes = classes.cpu()
            keep = (host[:, 4] > MIN_PROB).nonzero().view(-1)       # evaluator.py:35 (nothing left to drop where the model took min_prob)
            host, classes = host[keep], classes[keep]
            all_bboxes.extend(host[:, :4].tolist())
            all_probs.extend(host[:, 4].tolist())
            all_classes.extend(classes.tolist())
            all_image_ids.extend([image_id] * host.shape[0])

    def detect(self, model):
        """-> (image ids, boxes, classes, probs) as the lists evaluator.py:41-44 builds."""
        lists = ([], [], [], [])
        for index, (image_id, (image_batch, bboxes_batch, labels_batch, scale_batch)) in enumerate(zip(self.image_ids, self.loader)):
            inputs_all = self.eval_inputs(model, index, image_batch, bboxes_batch, labels_batch)
            self.score(model, lists, image_id, inputs_all, scale_batch)
        return lists

    def evaluate(self, model):
        return evaluate(self.ground_truth, *self.detect(model), path_to_results_dir=self.results_dir)


# The one-launch stem image gradient (frozen.STEM_IMAGE_GRAD) during the robust evaluation's attack.  Decided by the project's rule for
# every switch — on only where the measured gain of one image's attack + detection exceeds the two arms' combined min-max spread
# (tools/probe/det_rob_time.py, profiles/det_rob_time.jsonl; README "Detection robust mAP").  Measured: no gain, so OFF here too;
# AFAN_DET_ROB_STEM=1 (or RobustEvaluator(stem_image_grad=True)) turns it on.
ROB_STEM_IMAGE_GRAD = os.environ.get("AFAN_DET_ROB_STEM", "0") == "1"


class RobustEvaluator(Evaluator):
    """evaluator.py:90-128 (`ori_rob_evaluate`): per image attack_algo.eval_PGD with gradients enabled — steps, eps / 255, gamma / 255,
    randinit, clip — then Evaluator.detect's eval-mode forward, scale division, single host copy and lists on the adversarial image.
    An image without a non-difficult object has no loss (the reference raises on it): it is scored unattacked and counted
    (`self.unattacked`; one log line with the count).  stem_image_grad (None: ROB_STEM_IMAGE_GRAD): frozen.STEM_IMAGE_GRAD for the
    attack's duration.  steps = 0 without randinit hands the forward the clean image's values: Evaluator.detect's lists."""

    def __init__(self, loader, ground_truth, results_dir=None, steps=10, eps=2.0, gamma=0.5, randinit=False, clip=False,
                 stem_image_grad=None, log=None):
        super().__init__(loader, ground_truth, results_dir)
        self.steps, self.eps, self.gamma, self.randinit, self.clip = int(steps), float(eps), float(gamma), bool(randinit), bool(clip)
        self.stem_image_grad = ROB_STEM_IMAGE_GRAD if stem_image_grad is None else bool(stem_image_grad)
        self.log, self.unattacked, self.attacked = log, 0, 0

    def attack(self, model, index, image_batch, bboxes_batch, labels_batch):
        import torch
        from . import det_attack_algo, frozen
        if int(self.loader.counts[index]) == 0:      # (the host's own count: no read of the device)
            self.unattacked += 1
            return image_batch
        self.attacked += 1
        with torch.enable_grad(), frozen.stem_image_grad(self.stem_image_grad):
            adv = det_attack_algo.eval_PGD(x=image_batch, y={'bb': bboxes_batch, 'lb': labels_batch}, model=model, steps=self.steps,
                                           eps=(self.eps / 255), gamma=(self.gamma / 255), randinit=self.randinit, clip=self.clip)
        return adv.detach()

    def detect(self, model):
        self.unattacked = self.attacked = 0
        out = super().detect(model)
        line = 'Scored {:d} images without a non-difficult object unattacked (no loss to ascend)'.format(self.unattacked)
        if self.log is not None:
            self.log.i(line)
        else:
            print(line, flush=True)
        return out


SAT_TABLE = tuple((j, m) for j in range(5) for m in (False, True))      # the ten settings of eval_sat_layers.py: --sat_layer 0..4, without / with --mix


class SatLayerEvaluator(Evaluator):
    """evaluator.py:131-180 (`sat_layer_evaluate`): how the detections move as the backbone feature map behind layer `pertub_idx` is pushed
    along the line from its clean value to its PGD-adversarial value.  Per image, with gradients enabled: one train-mode `flag: 'head'`
    pass, det_ops.PGD on that feature map (steps, eps / 255, gamma / 255, randinit, clip), the sample point `sat_layer` of five
    (det_attack_algo.sat_layer_point; with mix re-normalised by the REVERSED mix_feature(point, feature_map)) in the model's compute
    dtype, then the eval-mode `flag: 'tail'` forward from it and Evaluator's scale division, single host copy and lists.  An image
    without a non-difficult object has no loss: it is scored from its clean feature and counted (`self.unattacked`; one log line).
    The model is left in eval mode.

    table=True (an addition): ONE attack per image and one sat_layer_points call for all ten settings (SAT_TABLE; the one-launch form
    wherever the layout allows it), then ten eval-mode tails one after another; detect -> {(sat_layer, mix): lists}, evaluate ->
    {(sat_layer, mix): (mean_ap, detail)}; the results files are those of the constructor's (sat_layer, mix).  The eval tails draw
    nothing from the host generator, so every row equals the single-setting run's lists from the same generator state."""

    def __init__(self, loader, ground_truth, results_dir=None, steps=10, eps=2.0, gamma=0.5, pertub_idx=1, sat_layer=1, mix=False,
                 randinit=False, clip=False, table=False, log=None):
        super().__init__(loader, ground_truth, results_dir)
        check_sat_settings(pertub_idx, sat_layer)
        self.steps, self.eps, self.gamma, self.randinit, self.clip = int(steps), float(eps), float(gamma), bool(randinit), bool(clip)
        self.pertub_idx, self.sat_layer, self.mix, self.table = int(pertub_idx), int(sat_layer), bool(mix), bool(table)
        self.log, self.unattacked, self.attacked = log, 0, 0

    def points(self, model, index, image_batch, bboxes_batch, labels_batch, settings, fused=None):
        """-> one entering feature per (sat_layer, mix) of settings, from one head pass and one attack."""
        import torch
        from . import det_attack_algo, det_ops
        idx = self.pertub_idx
        with torch.enable_grad():
            feature_map = model.train().forward({"x": image_batch, "adv": None, "out_idx": idx, "flag": 'head'}, bboxes_batch, labels_batch).detach()
            if int(self.loader.counts[index]) == 0:      # (the host's own count: no read of the device)
                self.unattacked += 1
                return [feature_map] * len(settings)
            self.attacked += 1
            feature_adv = det_ops.PGD(feature_map, image_batch, y={'bb': bboxes_batch, 'lb': labels_batch}, model=model, steps=self.steps,
                                      eps=(self.eps / 255), gamma=(self.gamma / 255), idx=idx, randinit=self.randinit, clip=self.clip)
        return det_attack_algo.sat_layer_points(feature_map, feature_adv.detach(), settings, getattr(model, "compute_dtype", torch.float32), fused)

    def eval_inputs(self, model, index, image_batch, bboxes_batch, labels_batch, point=None):
        if point is None:
            point = self.points(model, index, image_batch, bboxes_batch, labels_batch, [(self.sat_layer, self.mix)])[0]
        return {"x": image_batch, "adv": point, "out_idx": self.pertub_idx, "flag": 'tail', "min_prob": MIN_PROB}

    def _count_line(self):
        line = 'Scored {:d} images without a non-difficult object from their clean feature (no loss to ascend)'.format(self.unattacked)
        if self.log is not None:
            self.log.i(line)
        else:
            print(line, flush=True)

    def detect(self, model):
        self.unattacked = self.attacked = 0
        if not self.table:
            out = super().detect(model)
            self._count_line()
            return out
        rows = {s: ([], [], [], []) for s in SAT_TABLE}
        for index, (image_id, (image_batch, bboxes_batch, labels_batch, scale_batch)) in enumerate(zip(self.image_ids, self.loader)):
            pts = self.points(model, index, image_batch, bboxes_batch, labels_batch, SAT_TABLE, fused=True)
            for s, point in zip(SAT_TABLE, pts):
                self.score(model, rows[s], image_id, self.eval_inputs(model, index, image_batch, bboxes_batch, labels_batch, point), scale_batch)
        self._count_line()
        return rows

    def evaluate(self, model):
        if not self.table:
            return super().evaluate(model)
        own = (self.sat_layer, self.mix)
        return {s: evaluate(self.ground_truth, *lists, path_to_results_dir=self.results_dir if s == own else None)
                for s, lists in self.detect(model).items()}


def check_sat_settings(pertub_idx, sat_layer):
    """The two refusals of eval_sat_layers.py, before any work."""
    if pertub_idx not in (1, 2, 3):
        raise ValueError(f"--pertub_idx: a backbone layer 1..3, not {pertub_idx!r} (the reference's default 0 asserts in "
                         "backbone/resnet101_ori.py:236)")
    if sat_layer not in (0, 1, 2, 3, 4):
        raise ValueError(f"--sat_layer: one of the five sample points 0..4, not {sat_layer!r}")


# ------------------------------------------------------------------------------------ the driver of eval.py
def get_argparser():
    """eval.py:42-54, flag for flag."""
    from . import det_entry
    d = eval_defaults()
    parser = argparse.ArgumentParser()
    parser.add_argument('-s', '--dataset', type=str, choices=det_entry.DATASET_OPTIONS, required=True, help='name of dataset')
    parser.add_argument('-b', '--backbone', type=str, choices=det_entry.BACKBONE_OPTIONS, required=True, help='name of backbone model')
    parser.add_argument('-d', '--data_dir', type=str, default='./data', help='path to data directory')

    parser.add_argument('--image_min_side', type=float, help='default: {:g}'.format(d["image_min_side"]))
    parser.add_argument('--image_max_side', type=float, help='default: {:g}'.format(d["image_max_side"]))
    parser.add_argument('--anchor_ratios', type=str, help='default: "{!s}"'.format(d["anchor_ratios"]))
    parser.add_argument('--anchor_sizes', type=str, help='default: "{!s}"'.format(d["anchor_sizes"]))
    parser.add_argument('--pooler_mode', type=str, choices=det_entry.POOLER_OPTIONS, help='default: {:s}'.format(d["pooler_mode"]))
    parser.add_argument('--rpn_pre_nms_top_n', type=int, help='default: {:d}'.format(d["rpn_pre_nms_top_n"]))
    parser.add_argument('--rpn_post_nms_top_n', type=int, help='default: {:d}'.format(d["rpn_post_nms_top_n"]))
    parser.add_argument('checkpoint', type=str, help='path to evaluating checkpoint')
    return parser


ADDITIONS = ("synthetic", "dtype", "layout")
_EVAL_KEYS = ("image_min_side", "image_max_side", "anchor_ratios", "anchor_sizes", "pooler_mode", "rpn_pre_nms_top_n", "rpn_post_nms_top_n")


def eval_defaults():
    """config/config.py:9-14 with config/eval_config.py:8-9 on top."""
    from . import det_entry
    d = {k: det_entry.DEFAULTS[k] for k in _EVAL_KEYS}
    d.update(rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300)
    return d


def get_full_argparser():
    parser = get_argparser()
    parser.add_argument("--synthetic", type=int, default=0, help="evaluate on N synthetic images with boxes instead of VOC's test list")
    parser.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="backbone compute dtype")
    parser.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"], help="internal activation / weight layout")
    return parser


def config(args):
    """EvalConfig.setup (config/eval_config.py:11-20): the defaults, each replaced by its flag where one was given."""
    import ast
    cfg = eval_defaults()
    for k in cfg:
        v = getattr(args, k, None)
        if v is not None:
            cfg[k] = ast.literal_eval(v) if k in ("anchor_ratios", "anchor_sizes") else v
    return cfg


def check_unbuilt(args):
    """det_entry.check_unbuilt's refusals (the evaluation has no loss setting)."""
    from . import det_entry
    det_entry.check_unbuilt(argparse.Namespace(backbone=args.backbone, dataset=args.dataset, loss_settings=1))


def results_dir(path_to_checkpoint):
    """eval.py:62-64"""
    return os.path.join(os.path.dirname(path_to_checkpoint), 'results-{:s}-{:s}-{:s}'.format(
        time.strftime('%Y%m%d%H%M%S'), path_to_checkpoint.split(os.path.sep)[-1].split(os.path.curdir)[0],
        str(uuid.uuid4()).split('-')[0]))


def build_eval_split(args, cfg):
    """-> (images, boxes for the loader, classes for the loader, (image ids, ground truth), num_classes)."""
    from . import det_data
    if args.synthetic:
        hi = max(int(cfg["image_max_side"] * 0.5), 8)
        lo = max(min(int(cfg["image_min_side"] * 0.625), hi - 1), 7)
        s = det_data.SyntheticDetSplit(args.synthetic, seed=0, min_side=lo, max_side=hi)
        return s.images, s.boxes, s.classes, (s.image_ids, s.ground_truth()), s.num_classes
    images, boxes, classes, image_ids, ground_truth = det_data.load_voc_det_eval(args.data_dir, args.dataset)
    return images, boxes, classes, (image_ids, ground_truth), NUM_CLASSES


def get_rob_argparser(full=True):
    """eval_rob_ori.py:41-60, flag for flag (the PGD settings, --convert, then eval.py's flags); full: the project's additions too."""
    parser = get_full_argparser() if full else get_argparser()
    eval_actions = parser._actions[1:]                                   # (behind -h) eval.py's flags, in their order
    rob = argparse.ArgumentParser()
    # PGD Setting
    rob.add_argument('--steps', default=10, type=int, help='PGD-steps')
    rob.add_argument('--gamma', help='index of PGD gamma', default=0.5, type=float)
    rob.add_argument('--eps', default=2, type=float)
    rob.add_argument('--randinit', action="store_true", help="random start inside the eps-ball")
    rob.add_argument('--clip', action="store_true", help="project onto the eps-ball after every step")
    rob.add_argument('--convert', action="store_true", help="rename the keys of a Sequential-backbone checkpoint (model.py:420-437)")
    for a in eval_actions:
        rob._add_action(a)
    return rob


def main_rob(program, argv=None):
    """eval_rob_ori.py: robust mAP under an image PGD."""
    from . import det_data, det_entry
    args = get_rob_argparser().parse_args(argv)
    det_entry.print_args(args)
    check_unbuilt(args)
    cfg = config(args)
    device = det_entry.setup_device(program)

    path_to_checkpoint = args.checkpoint
    path_to_results_dir = results_dir(path_to_checkpoint)
    os.makedirs(path_to_results_dir)
    log = det_entry.Log(os.path.join(path_to_results_dir, 'eval.log'))
    log.i('Arguments:')
    for k, v in vars(args).items():
        log.i(f'\t{k} = {v}')
    log.i(det_entry.describe(cfg))

    images, boxes, classes, ground_truth, num_classes = build_eval_split(args, cfg)
    loader = det_data.DetDeviceLoader(images, boxes, classes, 1, device, False, cfg["image_min_side"], cfg["image_max_side"])
    evaluator = RobustEvaluator(loader, ground_truth, path_to_results_dir, steps=args.steps, eps=args.eps, gamma=args.gamma,
                                randinit=args.randinit, clip=args.clip, log=log)
    log.i('Found {:d} samples'.format(len(images)))

    model_cfg = dict(det_entry.DEFAULTS)
    model_cfg.update(cfg)
    model = det_entry.build_model(args, model_cfg, num_classes).to(device)
    det_entry.load_checkpoint(path_to_checkpoint, model, convert=args.convert)

    log.i('Start evaluating Robustness with 1 GPU (1 batch per GPU)')
    mean_ap, detail = evaluator.evaluate(model)
    log.i('Done')
    log.i('syd: pgd attack mean AP = {:.4f}'.format(mean_ap))
    log.i('\n' + detail)
    return mean_ap, detail


SAT_ADDITIONS = ADDITIONS + ("table",)


def get_sat_argparser(full=True):
    """eval_sat_layers.py:40-61, flag for flag (the PGD settings, --pertub_idx / --sat_layer / --mix, then eval.py's flags); full: the
    project's additions too (--synthetic --dtype --layout, then --table)."""
    parser = get_full_argparser() if full else get_argparser()
    eval_actions = parser._actions[1:]                                   # (behind -h) eval.py's flags, in their order
    sat = argparse.ArgumentParser()
    # PGD Setting
    sat.add_argument('--steps', default=10, type=int, help='PGD-steps')
    sat.add_argument('--gamma', help='index of PGD gamma', default=0.5, type=float)
    sat.add_argument('--eps', default=2, type=float)
    sat.add_argument('--randinit', action="store_true", help="random start inside the eps-ball")
    sat.add_argument('--clip', action="store_true", help="project onto the eps-ball after every step")
    sat.add_argument('--pertub_idx', help='the backbone layer (1..3) whose output is perturbed; the default 0 is refused, as the '
                     'reference asserts on it', default=0, type=int)
    sat.add_argument('--sat_layer', help='which of the five sample points clean .. adversarial (0..4) enters the tail', default=1, type=int)
    sat.add_argument('--mix', action="store_true", help="re-normalise the point onto the clean map's channel statistics")
    for a in eval_actions:
        sat._add_action(a)
    if full:
        sat.add_argument('--table', action="store_true", help="all ten (sat_layer, mix) settings from one attack per image")
    return sat


def main_sat(program, argv=None):
    """eval_sat_layers.py: mean AP at a sample point of the line clean feature -> PGD-adversarial feature."""
    from . import det_data, det_entry
    args = get_sat_argparser().parse_args(argv)
    det_entry.print_args(args)
    check_sat_settings(args.pertub_idx, args.sat_layer)
    check_unbuilt(args)
    cfg = config(args)
    device = det_entry.setup_device(program)

    path_to_checkpoint = args.checkpoint
    path_to_results_dir = results_dir(path_to_checkpoint)
    os.makedirs(path_to_results_dir)
    log = det_entry.Log(os.path.join(path_to_results_dir, 'eval.log'))
    log.i('Arguments:')
    for k, v in vars(args).items():
        log.i(f'\t{k} = {v}')
    log.i(det_entry.describe(cfg))
    print("SAT LAYER:[{}] MIX:[{}]".format(args.sat_layer, args.mix))

    images, boxes, classes, ground_truth, num_classes = build_eval_split(args, cfg)
    loader = det_data.DetDeviceLoader(images, boxes, classes, 1, device, False, cfg["image_min_side"], cfg["image_max_side"])
    evaluator = SatLayerEvaluator(loader, ground_truth, path_to_results_dir, steps=args.steps, eps=args.eps, gamma=args.gamma,
                                  pertub_idx=args.pertub_idx, sat_layer=args.sat_layer, mix=args.mix, randinit=args.randinit, clip=args.clip,
                                  table=args.table, log=log)
    log.i('Found {:d} samples'.format(len(images)))

    model_cfg = dict(det_entry.DEFAULTS)
    model_cfg.update(cfg)
    model = det_entry.build_model(args, model_cfg, num_classes).to(device)
    det_entry.load_checkpoint(path_to_checkpoint, model)

    log.i('Start evaluating Robustness with 1 GPU (1 batch per GPU)')
    out = evaluator.evaluate(model)
    log.i('Done')
    if args.table:
        for (j, m), (ap, _) in out.items():
            log.i('SAT LAYER:[{}] MIX:[{}] mean AP = {:.4f}'.format(j, m, ap))
        mean_ap, detail = out[(args.sat_layer, args.mix)]
    else:
        mean_ap, detail = out
    log.i('mean AP = {:.4f}'.format(mean_ap))
    log.i('\n' + detail)
    return mean_ap, detail


def main(program, argv=None):
    from . import det_data, det_entry
    args = get_full_argparser().parse_args(argv)
    check_unbuilt(args)
    cfg = config(args)
    device = det_entry.setup_device(program)

    path_to_checkpoint = args.checkpoint
    path_to_results_dir = results_dir(path_to_checkpoint)
    os.makedirs(path_to_results_dir)
    log = det_entry.Log(os.path.join(path_to_results_dir, 'eval.log'))
    log.i('Arguments:')
    for k, v in vars(args).items():
        log.i(f'\t{k} = {v}')
    log.i(det_entry.describe(cfg))

    images, boxes, classes, ground_truth, num_classes = build_eval_split(args, cfg)
    loader = det_data.DetDeviceLoader(images, boxes, classes, 1, device, False, cfg["image_min_side"], cfg["image_max_side"])
    evaluator = Evaluator(loader, ground_truth, path_to_results_dir)
    log.i('Found {:d} samples'.format(len(images)))

    model_cfg = dict(det_entry.DEFAULTS)
    model_cfg.update(cfg)
    model = det_entry.build_model(args, model_cfg, num_classes).to(device)
    det_entry.load_checkpoint(path_to_checkpoint, model)

    log.i('Start evaluating with 1 GPU (1 batch per GPU)')
    mean_ap, detail = evaluator.evaluate(model)
    log.i('Done')
    print("-" * 36)
    print("[{}]".format(path_to_checkpoint))
    log.i('mean AP = {:.4f}'.format(mean_ap))
    print("-" * 36)
    log.i('\n' + detail)
    return mean_ap, detail
