"""CDR — critical-parameter gradient masking for noisy-label training.

Reference: CDR/main.py:179-215 (`train_one_step`), :218-253 (`train`).
After backward, over all 2-D and 4-D parameters (conv and linear weights):

    metric = |g * w| ;  thr = k-th largest metric, k = int(nonzero_ratio * N)
    g <- g * (|g * w| >= thr) * clip

The reference concatenates the 25.6M-element metric and runs a full
``torch.topk`` every step.  Here (GPU) the threshold comes from a 4-pass 8-bit
radix select over the float bit patterns (``cdr_threshold``) and the mask is
applied in place (``cdr_mask``), both as multi-tensor kernels: nothing is
concatenated or sorted.  CPU uses the reference math.
"""
from __future__ import annotations

from typing import Iterable

import numpy as np
import torch

from .. import _ext

CHUNK = 4096


def _selected(params: Iterable[torch.Tensor]):
    return [p for p in params if p.grad is not None and p.dim() in (2, 4)]


_TABLES = {}


def _table(ps, device):
    """Device (param, grad) pointer table + chunk list, cached per pointer set.  Built with
    ``Fn.table_to_device`` (values in a fill kernel's arguments, no host->device copy), so a step
    captured into a HIP graph (``--graph``) replays it correctly."""
    from ..ops import functional as Fn

    entries, chunks = [], []
    for i, p in enumerate(ps):
        if not (p.is_contiguous() and p.grad.is_contiguous() and p.dtype == torch.float32):
            raise RuntimeError("CDR kernels need contiguous fp32 params/grads")
        entries.append((p.data_ptr(), p.grad.data_ptr(), 0, 0, 0, p.numel()))
    key = (str(device), tuple(entries))
    hit = _TABLES.get(key)
    if hit is None:
        for i, p in enumerate(ps):
            chunks.extend((i, c) for c in range((p.numel() + CHUNK - 1) // CHUNK))
        if len(_TABLES) > 8:
            _TABLES.clear()
        hit = _TABLES[key] = (Fn.table_to_device(entries, torch.int64, device).view(-1, 6),
                              Fn.table_to_device(chunks, torch.int32, device).view(-1, 2))
    return hit


@torch.no_grad()
def cdr_mask_gradients(params: Iterable[torch.Tensor], nonzero_ratio: float, clip: float) -> torch.Tensor:
    """Mask gradients in place; returns the threshold (0-dim tensor on the params' device)."""
    ps = _selected(params)
    if not ps:
        return torch.tensor(0.0)
    n = sum(p.numel() for p in ps)
    nz = int(nonzero_ratio * n)
    dev = ps[0].device
    if nz <= 0:
        for p in ps:
            p.grad.zero_()
        return torch.tensor(float("inf"), device=dev)
    if ps[0].is_cuda:
        K = _ext.hip_ops()
        from ..ops import functional as Fn

        tab, ch = _table(ps, dev)
        # fresh every step (the select passes rewrite it): a fill kernel, so a graph replay resets it
        state = Fn.table_to_device([0, 0, nz, 0], torch.int32, dev)
        thr = K.cdr_threshold(tab, ch, state)
        K.cdr_mask(tab, ch, state, float(clip))
        return thr.reshape(())
    metric = torch.cat([(p.grad * p).abs().view(-1) for p in ps])
    thr = torch.topk(metric, nz)[0][-1]
    for p in ps:
        mask = ((p * p.grad).abs() >= thr).to(p.grad.dtype) * clip
        p.grad.mul_(mask)
    return thr


def clip_schedule(noise_rate: float, num_gradual: int, epoch: int) -> float:
    """CDR/main.py:222-227.  The reference computes a gradual schedule and then
    overrides it with the constant ``1 - noise_rate`` (kept for parity)."""
    sched = np.linspace(1 - noise_rate, 1, num=num_gradual)[::-1]
    _ = sched[epoch] if epoch < num_gradual else None
    return 1.0 - noise_rate


def run(args):
    """CDR/main.py:286-383: ResNet-50 + MLP head + LogSoftmax, SGD(momentum 0.9),
    MultiStepLR([10, 20]) stepped BEFORE each epoch (reference order), CE on the
    log-probabilities, critical-parameter masking after every backward."""
    from ..config import refuse_mix

    refuse_mix(args, "cdr")
    from ..algos.baseline import build_classifier
    from ..engine.loop import ClassificationLoop
    from ..engine.logger import rotate_results_file
    from ..engine.runtime import build_data, setup
    from ..ops import functional as Fn
    from ..optim import MultiStepLR, build_ema, build_optimizer
    from ..parallel.ddp import wrap_ddp
    import os

    rt = setup(args)
    rotate_results_file(os.path.join(args.out_dir, "results_cdr.txt"))
    train_data, val_data, _, _ = build_data(args, rt)
    model = build_classifier(args, log_softmax=True).to(rt.device)
    # one process per GPU: gradients are all-reduced by DDP before the mask, so every rank
    # selects the same critical parameters from the global-batch gradient
    net = wrap_ddp(model, rt.local_rank, syncbn=args.syncbn and (rt.world > 1 or args.force_ddp), bucket_cap_mb=args.bucket_cap_mb,
                   first_bucket_mb=args.first_bucket_mb, force=args.force_ddp)
    opt = build_optimizer("sgd", model.parameters(), args.lr, args.momentum, 0.0)
    sched = MultiStepLR(opt, milestones=args.milestones, gamma=args.gamma)
    C = args.num_classes
    state = {"epoch": 0}

    def fwd_train(batch):
        return Fn.cross_entropy(net(batch[0]), batch[1], C, return_rank=True)

    def fwd_eval(batch):
        return Fn.cross_entropy_rows(model(batch[0]), batch[1], C)

    def post_backward():
        clip = clip_schedule(args.noise_rate, args.num_gradual, state["epoch"])
        cdr_mask_gradients(model.parameters(), nonzero_ratio=clip, clip=clip)

    class _Loop(ClassificationLoop):
        def train_epoch(self, epoch):
            state["epoch"] = epoch
            return super().train_epoch(epoch)

    models = {"model": model}
    loop = _Loop(args, rt, models, opt, sched, train_data, val_data, fwd_train, fwd_eval,
                 post_backward=post_backward, scheduler_before_epoch=True, train_modules=[net],
                 ema=build_ema(args, models, opt))
    best = loop.run()
    hist = loop.logger.history.get("val/top1", [])
    if rt.is_main and hist:  # the reference crashes on an empty list here (CDR/main.py:381)
        loop.logger.line(f"best val top1 {100 * max(hist):.3f} at epoch {int(np.argmax(hist)) + 1}")
    return best
