"""The Detection multi-layer SAT iteration (Detection/train_aug_sat_muti_advt.py:26-209) on one MI355X per rank: owner of the
parameter arena and the SGD around `det_attack_algo.det_train_phases`, and of the data-parallel exchange.

The reference shards this step with `nn.DataParallel(Model(...).cuda())` (:36-43): one process, replicas rebuilt every forward,
gradients reduced onto GPU 0.  Here: one process per GPU (torch.distributed, RCCL over xGMI), minibatch sharding, frozen
BatchNorm (nothing to synchronise), ONE exchange per iteration — the fp32 gradient arena summed over the ranks, 1/world folded
into the SGD kernel — started TAIL FIRST: the joint backward is cut at the backbone's output, so the gradients of layer4 / RPN /
the two heads (the arena's suffix, `tail_range`) are final
while the backbone's backward (layer3 / layer2 over the three passes that reach it) still runs, and their all-reduce flies on a
side stream under it; the backbone's gradients follow at finish().  SGD(lr 0.001, momentum 0.9, weight decay 5e-4) as
config/train_config.py; the learning-rate schedule (WarmUpMultiStepLR, :48) steps outside, once per iteration."""
import torch

from .arena import ArenaSGD, ParamArena
from .det_attack_algo import det_adv_phases, det_base_phases, det_final_phases, det_train_phases, parse_mix_layer
from .train_step import StepTrainer

# everything behind the conv4 feature map: layer4 (= detection.hidden), the RPN and the two heads.  The backbone's unused ImageNet
# classifier `features.fc` sits between them in the reference's parameter order and never receives a gradient: optim.SGD skips a
# tensor whose .grad is None (no weight decay, no momentum: it keeps its values), so it stays OUTSIDE the arena (UNUSED_PARAMS) —
# the prefix is kept for arenas built with skip=() by callers that want the reference's full parameter list.
TAIL_PREFIXES = ("features.layer4.", "features.fc.", "rpn.", "detection.")
UNUSED_PARAMS = ("features.fc.weight", "features.fc.bias")


class DetTrainer(StepTrainer):
    """Of StepTrainer only the exchange set-up: frozen BatchNorm (no grid barrier on this path: flush_guard() is the uniform no-op),
    no graph of its own, and a step of three inputs."""

    PHASES = ("sat", "final", "base", "adv")
    ADV_DEFAULTS = dict(steps=1, eps=2.0, gamma=0.5, randinit=False, clip=False, noise="host")

    def __init__(self, model, *, lr=0.001, momentum=0.9, weight_decay=0.0005, loss_settings=1, group=None, allreduce_chunks=4,
                 segmented=None, arena=None, noise_ahead=False, phases="sat", final=None, adv=None):
        """phases: which iteration step() runs on the same arena, SGD and exchange — "sat" (train_aug_sat_muti_advt.py, the default),
        "final" (train_aug_final.py:78-163 with the keyword settings of det_attack_algo.det_final_phases in `final`), "base"
        (train_baseline.py:76-89) or "adv" (train_baseline_advtrain.py:75-93, PGD training, with the settings of
        det_attack_algo.det_adv_phases in `adv`: steps, eps, gamma, randinit, clip, noise; noise_ahead=True draws the next iteration's
        host random start behind this one's backward, as for "sat").  These three run their backward in one part: with a process
        group the whole arena is reduced at finish()."""
        if phases not in self.PHASES:
            raise ValueError(f"phases: one of {self.PHASES}, not {phases!r}")
        self.phases = phases
        self.final = dict(final or {})
        if phases == "final":
            if self.final.get("pertub_idx_se") not in (1, 2, 3):
                raise ValueError(f"final['pertub_idx_se']: a backbone layer 1..3, not {self.final.get('pertub_idx_se')!r}")
            parse_mix_layer(self.final.get("mix_layer"))
        self.adv = dict(self.ADV_DEFAULTS, **(adv or {}))
        if phases == "adv":
            unknown = sorted(set(self.adv) - set(self.ADV_DEFAULTS))
            if unknown:
                raise ValueError(f"adv: unknown settings {unknown} (known: {sorted(self.ADV_DEFAULTS)})")
            if isinstance(self.adv["steps"], bool) or not isinstance(self.adv["steps"], int) or self.adv["steps"] < 0:
                raise ValueError(f"adv['steps']: a number of PGD steps >= 0, not {self.adv['steps']!r}")
            if self.adv["noise"] not in ("host", "device"):
                raise ValueError(f"adv['noise']: 'host' or 'device', not {self.adv['noise']!r}")
        self.loss_settings = int(loss_settings)
        self.arena = arena if arena is not None else ParamArena(model, skip=UNUSED_PARAMS)
        self.optimizer = ArenaSGD(self.arena, lr, momentum, weight_decay)
        self._init_exchange(model, group, allreduce_chunks)
        # the next iteration's image-PGD noise drawn behind this iteration's backward (det_attack_algo.NoiseAhead): same generator
        # stream provided the caller draws nothing from the host generator between iterations
        from .det_attack_algo import NoiseAhead
        self.noise_ahead = NoiseAhead() if noise_ahead else None
        self.segmented = bool(segmented)        # True: run the two-part backward on one GPU too (tests)
        self._graph = None                      # (bench.py asks every trainer whether its step is a hipGraph replay)

    def tail_range(self):
        """[lo, hi) in arena-parameter order of everything behind the backbone's output — a suffix, or None if the model's
        parameter order does not make it one (then the whole arena is exchanged at finish())."""
        return tail_range(self.arena.names)

    def _phased(self):
        return self.segmented or self.reducer is not None

    def step(self, images, bboxes, labels):
        if self.phases != "sat":
            out = {}
            if self.reducer is not None:
                self.reducer.begin(explicit=True)
            if self.phases == "final":
                gen = det_final_phases(self.model, self.optimizer, images, bboxes, labels, out, defer_step=True, **self.final)
            elif self.phases == "adv":
                gen = det_adv_phases(self.model, self.optimizer, images, bboxes, labels, out, defer_step=True, noise_ahead=self.noise_ahead,
                                     **self.adv)
            else:
                gen = det_base_phases(self.model, self.optimizer, images, bboxes, labels, out, defer_step=True)
            for _ in gen:
                pass
            if self.reducer is not None:
                self.reducer.finish()      # nothing was announced: the whole arena is reduced here
            self.optimizer.step()
            return out
        out, rng = {}, self.tail_range()
        cut = self._phased() and rng is not None and hasattr(self.model, "cut_features")
        if self.reducer is not None:
            self.reducer.begin(explicit=True)
        for ph in det_train_phases(self.model, self.optimizer, images, bboxes, labels, out, loss_settings=self.loss_settings,
                                   cut=cut, defer_step=True, noise_ahead=self.noise_ahead):
            if ph == "tail" and self.reducer is not None:
                self.reducer.launch_params(*rng)
        if self.reducer is not None:
            self.reducer.finish()          # whatever no launch_params() announced (the backbone) is reduced here
        self.optimizer.step()
        return out


def tail_range(names):
    idx = [i for i, n in enumerate(names) if n.startswith(TAIL_PREFIXES)]
    if not idx or idx != list(range(idx[0], len(names))):
        return None
    return idx[0], len(names)
