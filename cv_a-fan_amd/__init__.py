"""cv_a-fan_amd — the A-FAN training hot path (feature-space PGD + joint clean/adv step), MI355X-native.

The directory name carries a hyphen (it is fixed by the build contract), so import it with
    import importlib; afan = importlib.import_module("cv_a-fan_amd")
Sub-modules: attack_algo (PGD & friends, reference signatures), pgd (the sign-PGD core every attack path is built from), resnet_s (slice-protocol models),
arena (flat parameter arena + fused SGD), train_step (the joint step, data parallel), ops (tensor
wrappers over the C-ABI in include/afan_hip.h), cls_data (DeviceLoader: one-launch CIFAR batches), cls_entry (what the Classification entry points share: flags, set-up, the train / evaluation / epoch loops, the
checkpoint files; main_perturb for cmd/run_perturb.sh, main_base for cmd/run_base.sh, main_learnable, main_inference), infer (the fused, graph-replayed eval forward; main_inference evaluates a checkpoint), deeplab (the
DeepLabv3+ split-forward network), seg_attack_algo / seg_trainer (the Segmentation A-FAN operators and iteration), seg_data (SegDeviceLoader: one-launch
segmentation batches; main_aug_final is the entry point for cmd/run_seg.sh, main_ori for cmd/run_seg_base.sh), seg_entry (what the Segmentation entry
points share: the parser, set-up, checkpoint and restore, the iteration loop), seg_eval (StreamSegMetrics with a one-launch confusion
matrix, validate; main_seg_val scores a checkpoint, cmd/run_seg_val.sh), det_ops / det_attack_algo / det_model / det_trainer
(the Detection operators, iteration, the Faster-RCNN / ResNet-101 model and its data-parallel trainer), det_data (DetDeviceLoader: one-launch
detection batches with their boxes), det_entry (the Detection parser, learning-rate schedule, checkpoint and iteration loop;
train_aug_sat_muti_advt is the entry point for cmd/run_det.sh), det_eval (the VOC 2007 mean AP, the evaluator and the driver of eval.py, cmd/run_det_eval.sh).
"""
from . import _lib, ops  # noqa: F401
from ._lib import AfanLibraryError, LIB_PATH  # noqa: F401
from . import resnet_s, frozen, pgd, attack_algo, arena, grid_guard, train_step, learnable, seg_attack_algo, deeplab, seg_trainer, seg_data, seg_eval, det_ops, det_attack_algo, det_model, det_trainer, det_data, det_entry, det_eval, host, infer  # noqa: F401
from .attack_algo import PGD, get_sample_points, l2ball_proj, linfball_proj, mix_feature, tensor_clamp  # noqa: F401

__version__ = "0.1.0"
