"""What the four Classification programs share, as plain functions: the flag groups, set-up, model preparation, the loaders, ONE train()
for the three trainers (train_step.AfanTrainer, train_step.BaseTrainer, learnable.LearnableTrainer), ONE evaluation loop (validate and
main_inference.robust_validate), resume, the epoch-end files and the epoch loop.  main_perturb.py, main_base.py, main_learnable.py and
main_inference.py keep their parsers, their trainers and what only they print; the loops take any trainer with step() and
flush_guard(), so they run on stubs without a GPU (tests/test_cls_entry.py)."""
import os
import pickle
import random

import numpy as np
import torch
import torch.distributed as dist

from . import cls_data, host, infer, resnet_s


# ----------------------------------------------------------------------------------------- flag groups
def add_base_flags(parser, save_dir, data_help="location of the data corpus (cifar-10-batches-py)"):
    """main_perturb.py:28-33"""
    parser.add_argument("--data", type=str, default="../data", help=data_help)
    parser.add_argument("--print_freq", default=50, type=int, help="print frequency")
    parser.add_argument("--seed", default=None, type=int, help="random seed")
    parser.add_argument("--gpu", type=int, default=0, help="gpu device id")
    parser.add_argument("--resume", action="store_true", help="resume from checkpoint")
    parser.add_argument("--save_dir", help="The directory used to save the trained models", default=save_dir, type=str)


def add_optimizer_flags(parser, batch_help="batch size (global; split across ranks)"):
    """main_perturb.py:36-41"""
    parser.add_argument("--batch_size", type=int, default=128, help=batch_help)
    parser.add_argument("--lr", default=0.1, type=float, help="initial learning rate")
    parser.add_argument("--momentum", default=0.9, type=float, help="momentum")
    parser.add_argument("--weight_decay", default=5e-4, type=float, help="weight decay")
    parser.add_argument("--epochs", default=200, type=int, help="number of total epochs to run")
    parser.add_argument("--decreasing_lr", default="50,150", help="decreasing strategy")


def add_addition_flags(parser, arch=True, dual_bn=False, max_iters=True,
                       synthetic_help="train on N synthetic images instead of CIFAR-10"):
    """The flags the reference does not have."""
    if arch:
        parser.add_argument("--arch", default="resnet56s", choices=sorted(resnet_s.ARCHS))
    parser.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="backbone compute dtype")
    parser.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"],
                        help="internal activation / weight layout (nhwc: the library's MFMA convolutions; nchw: the general fp32-arithmetic kernels)")
    if dual_bn:
        parser.add_argument("--dual_bn", action="store_true", help="auxiliary BatchNorm set for adversarial features (not in the "
                            "reference: extra state_dict keys <bn>.adv.*; evaluation uses the main set)")
    parser.add_argument("--synthetic", type=int, default=0, help=synthetic_help)
    if max_iters:
        parser.add_argument("--max_iters", type=int, default=0, help="stop each epoch after this many iterations (0 = all)")


# ------------------------------------------------------------------------------- set-up, model, loaders
def setup(program, gpu, distributed=False, place=True):
    """-> (device, rank, world, placement, log).  distributed: rank, world and the local device are torch.distributed.run's, one rank per
    MI355X, and the process group is opened when there is more than one.  place: this rank's threads go on one block of cores of its
    GPU's NUMA node (before the GPU is touched); the placement is returned for the program to print.  log prints on rank 0."""
    world = int(os.environ.get("WORLD_SIZE", "1")) if distributed else 1
    rank = int(os.environ.get("RANK", "0")) if distributed else 0
    local = int(os.environ.get("LOCAL_RANK", str(gpu))) if distributed else int(gpu)
    placement = host.place_rank(local) if place else None
    if not torch.cuda.is_available():
        raise RuntimeError(f"{program} needs an MI355X: this build has no CPU path (oracle/ is test infrastructure)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)

    def log(*a):
        if rank == 0:
            print(*a, flush=True)

    return dev, rank, world, placement, log


def close(world):
    if world > 1:
        dist.destroy_process_group()


def shown_placement(placement):
    return {k: v for k, v in placement.items() if k != "restore"}


def setup_seed(seed):
    """main_perturb.py:310-315 (cudnn.deterministic selects deterministic MIOpen algorithms on ROCm)."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True


def check_arch(args):
    if args.arch == "resnet50" and not args.synthetic:
        raise SystemExit("--arch resnet50 is the ImageNet-shape synthetic configuration: pass --synthetic N")


def prepare_model(model, args, dev):
    model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model.set_channels_last(args.layout == "nhwc").to(dev)
    return model


def log_general_convs(model, log):
    """After the trainer is built: the line says what the iteration will run."""
    vendor = resnet_s.general_convs(model)
    log("convolutions outside the library's kernels: {}{}".format(
        len(vendor), " (general f32-MFMA kernels; --dtype bf16 --layout nhwc is the tuned bf16 MFMA path)" if vendor else ""))


def synthetic_shape(args):
    """(side, classes) of --synthetic images: ImageNet's for --arch resnet50, CIFAR-10's otherwise."""
    return (224, 1000) if getattr(args, "arch", None) == "resnet50" else (32, 10)


def build_loaders(args, dev, rank=0, world=1, shared_seed=True):
    """-> (train, validation, test) loaders, resident on the device.  shared_seed: rank 0's draw (seeded or not) is every rank's
    shuffling seed; main_learnable.py (single GPU, like the reference) makes no such draw."""
    if args.synthetic:
        side, classes = synthetic_shape(args)
        train_loader = cls_data.SyntheticLoader(args.synthetic, args.batch_size, dev, rank, world, side=side, classes=classes)
        val_loader = test_loader = cls_data.SyntheticLoader(max(args.synthetic // 10, args.batch_size), args.batch_size, dev,
                                                            side=side, classes=classes)
        return train_loader, val_loader, test_loader
    tr, va, te = cls_data._load_cifar10(args.data)
    seed = None
    if shared_seed:
        shared = torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64)
        if world > 1:
            shared = shared.to(dev)
            dist.broadcast(shared, src=0)
        seed = int(shared.item())
    train_loader = cls_data.DeviceLoader(tr[0], tr[1], args.batch_size, dev, True, rank, world, seed=seed)
    val_loader = cls_data.DeviceLoader(va[0], va[1], args.batch_size, dev, False, drop_last=False)
    test_loader = cls_data.DeviceLoader(te[0], te[1], args.batch_size, dev, False, drop_last=False)
    return train_loader, val_loader, test_loader


# ----------------------------------------------------------------------------------------------- loops
class AverageMeter(object):
    """main_perturb.py:271-286"""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def accuracy(output, target):
    return (output.argmax(dim=1) == target).float().sum() * (100.0 / target.shape[0])


def _drain(pending, losses, top1):
    """The read-back: (loss, prec1, n) device scalars of every iteration since the last one, into the meters, in order."""
    for loss_t, prec_t, n in pending:
        losses.update(loss_t.item(), n)
        top1.update(prec_t.item(), n)
    pending.clear()


NORMS = {"cat": lambda parts: torch.mean(torch.cat(parts, dim=0)).cpu(),       # main_perturb.py: one mean over every sample
         "layers": lambda parts: torch.cat(parts, dim=1).mean(dim=1).cpu()}    # main_learnable.py: one mean per perturbed layer


def train(train_loader, trainer, optimizer, epoch, args, log, norms=None):
    """main_perturb.py:153-225, main_base.py:140-180, main_learnable.py:175-277.  Device-side accumulation; one read-back per print_freq
    iterations, in iteration order, so the printed values are those of the per-batch reads.  norms: None (no perturbation: no norm
    lines, returns (accuracy, loss)) or a key of NORMS (`l2 mean` / `linf mean` lines, returns (accuracy, loss, l2, linf))."""
    losses, top1 = AverageMeter(), AverageMeter()
    trainer.model.train()
    wp_steps = len(train_loader)
    norm_l2, norm_linf, pending = [], [], []

    def flush():
        # (the host reads results here anyway: every step issued so far is verified against a given-up grid barrier of the in-launch
        # BatchNorm, and run again on the two-launch forms if one did — grid_guard.GuardedTrainer.flush_guard)
        if trainer.flush_guard():
            log("in-launch BatchNorm: a grid barrier gave up; the affected steps were run again on the two-launch forms "
                "(their logged loss / accuracy values are invalid)")
        _drain(pending, losses, top1)

    for i, (inp, target) in enumerate(train_loader):
        if args.max_iters and i >= args.max_iters:
            break
        if epoch == 0:      # train_step.warmup_lr (main_perturb.py:288-293), which divides by zero on a one-batch epoch
            lr = min(i * args.lr / (wp_steps - 1), args.lr) if wp_steps > 1 else args.lr
            for g in optimizer.param_groups:
                g["lr"] = lr
        r = trainer.step(inp, target)
        if norms:
            norm_l2.append(r["l2"])
            norm_linf.append(r["linf"])
        pending.append((r["loss"], r["prec1"], inp.size(0)))
        if i % args.print_freq == 0:
            flush()
            log("Epoch: [{0}][{1}/{2}]\t"
                "Loss {loss.val:.4f} ({loss.avg:.4f})\t"
                "Accuracy {top1.val:.3f} ({top1.avg:.3f})\t".format(epoch, i, len(train_loader), loss=losses, top1=top1))
    flush()
    if norms:
        norm_mean_l2, norm_mean_linf = NORMS[norms](norm_l2), NORMS[norms](norm_linf)
        log("l2 mean = {}".format(norm_mean_l2))
        log("linf mean = {}".format(norm_mean_linf))
    log("train_accuracy {top1.avg:.3f}".format(top1=top1))
    if norms:
        return top1.avg, losses.avg, norm_mean_l2.numpy(), norm_mean_linf.numpy()
    return top1.avg, losses.avg


def evaluate(loader, per_batch, tag, closing, args, log):
    """main_perturb.py:227-263 around per_batch(inp, target) -> (loss, prec1) on the device: read back at --print_freq batches and at
    the end, in batch order, so the printed values are those of the per-batch reads.  `<tag>: [i/n]` lines, then `<closing> <avg>`."""
    losses, top1 = AverageMeter(), AverageMeter()
    pending = []
    for i, (inp, target) in enumerate(loader):
        loss, prec = per_batch(inp, target)
        pending.append((loss, prec, inp.size(0)))
        if i % args.print_freq == 0:
            _drain(pending, losses, top1)
            log(tag + ": [{0}/{1}]\t"
                "Loss {loss.val:.4f} ({loss.avg:.4f})\t"
                "Accuracy {top1.val:.3f} ({top1.avg:.3f})".format(i, len(loader), loss=losses, top1=top1))
    _drain(pending, losses, top1)
    log(closing + " {top1.avg:.3f}".format(top1=top1))
    return top1.avg, losses.avg


def validate(val_loader, model, criterion, args, log):
    """The eval forward is infer.Evaluator's (bf16 channels-last: one fused launch per convolution, replayed as a hipGraph per batch
    shape)."""
    model.eval()
    ev = infer.evaluator_for(model, criterion)
    ev.refresh()
    return evaluate(val_loader, ev.evaluate, "Test", "valid_accuracy", args, log)


# ------------------------------------------------------------------------- resume, epoch end, epoch loop
def resume(save_dir, dev, model, trainer, optimizers, scheduler):
    """-> (best_prec1, start_epoch) of save_dir/checkpoint.pt, its state loaded.  optimizers: {checkpoint key: optimizer}."""
    ck = torch.load(os.path.join(save_dir, "checkpoint.pt"), map_location=dev)
    model.load_state_dict(ck["state_dict"])
    trainer.arena.refresh_shadow()
    for key, opt in optimizers.items():
        opt.load_state_dict(ck[key])
    scheduler.load_state_dict(ck["scheduler"])
    return ck["best_prec1"], ck["epoch"]


def write_epoch(save_dir, epoch, model, best_prec1, is_best, optimizers, scheduler, result, norm_result=None, plot=True):
    """The files of one finished epoch: checkpoint.pt, best_model.pt on an improvement, net_train.png (plot), result.pkl and, where
    there are norms, result_norm.pkl."""
    state = {"epoch": epoch + 1, "state_dict": model.state_dict(), "best_prec1": best_prec1,
             **{key: opt.state_dict() for key, opt in optimizers.items()}, "scheduler": scheduler.state_dict()}
    if is_best:
        torch.save(state, os.path.join(save_dir, "best_model.pt"))
    torch.save(state, os.path.join(save_dir, "checkpoint.pt"))
    if plot:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            plt.plot(result["train"], label="train_acc"), plt.plot(result["ta"], label="TA"), plt.plot(result["test_ta"], label="test_TA")
            plt.legend()
            plt.savefig(os.path.join(save_dir, "net_train.png"))
            plt.close()
        except ImportError:
            pass
    pickle.dump(result, open(os.path.join(save_dir, "result.pkl"), "wb"))
    if norm_result is not None:
        pickle.dump(norm_result, open(os.path.join(save_dir, "result_norm.pkl"), "wb"))


def log_lr(log, lr):
    log(lr)


def run_epochs(args, dev, rank, log, model, criterion, trainer, optimizers, scheduler, loaders, validate, norms=None, plot=True,
               header=log_lr):
    """main_perturb.py:97-150.  optimizers: {checkpoint key: optimizer}, "optimizer" first; header(log, lr): the lines before each
    epoch, the learning rate by default; validate: looked up by the caller, so a program can stand in its own."""
    train_loader, val_loader, test_loader = loaders
    optimizer = optimizers["optimizer"]
    best_prec1, start_epoch = 0, 0
    if args.resume:
        log("resume from checkpoint")
        best_prec1, start_epoch = resume(args.save_dir, dev, model, trainer, optimizers, scheduler)
    result = {"train": [], "test_ta": [], "ta": []}
    norm_result = {"l2": {}, "linf": {}} if norms else None
    os.makedirs(args.save_dir, exist_ok=True)
    for epoch in range(start_epoch, args.epochs):
        header(log, optimizer.state_dict()["param_groups"][0]["lr"])
        acc, _, *norm = train(train_loader, trainer, optimizer, epoch, args, log, norms)
        if norms:
            norm_result["l2"][epoch + 1], norm_result["linf"][epoch + 1] = norm
        tacc, _ = validate(val_loader, model, criterion, args, log)
        test_tacc, _ = validate(test_loader, model, criterion, args, log)
        scheduler.step()
        result["train"].append(acc), result["ta"].append(tacc), result["test_ta"].append(test_tacc)
        is_best = tacc > best_prec1
        best_prec1 = max(tacc, best_prec1)
        if rank == 0:
            write_epoch(args.save_dir, epoch, model, best_prec1, is_best, optimizers, scheduler, result, norm_result, plot)
    return best_prec1
