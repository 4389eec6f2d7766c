"""LR schedules used by the reference workloads.

* StepLR(step_size=10, gamma=0.1) per epoch (BASELINE/main.py:154,312; ARCFACE/arc_main.py:255)
  and MultiStepLR(milestones) (CDR/main.py:340, NESTED/train.py:423) are torch's own
  (re-exported here).
* :class:`LinearWarmup` — per-iteration linear ramp (BASELINE/main.py:170-197
  ramps 1e-6 -> lr; NESTED/train.py:292-295 ramps lr*n/warmUpIter).
"""
from __future__ import annotations

from torch.optim.lr_scheduler import MultiStepLR, StepLR  # noqa: F401


class LinearWarmup:
    """Set lr = start + (target - start) * n / iters for n = 1..iters (per-iteration)."""

    def __init__(self, optimizers, iters: int, target_lr: float, start_lr: float = 0.0):
        self.optimizers = optimizers if isinstance(optimizers, (list, tuple)) else [optimizers]
        self.iters, self.target, self.start = int(iters), float(target_lr), float(start_lr)
        self.n = 0

    def lr_at(self, n: int) -> float:
        if self.iters <= 0:
            return self.target
        f = min(1.0, n / float(self.iters))
        return self.start + (self.target - self.start) * f

    def step(self) -> float:
        self.n += 1
        lr = self.lr_at(self.n)
        for opt in self.optimizers:
            for g in opt.param_groups:
                g["lr"] = lr
        return lr

    @property
    def done(self) -> bool:
        return self.n >= self.iters

    def state_dict(self):
        return {"n": self.n, "iters": self.iters, "target": self.target, "start": self.start}

    def load_state_dict(self, sd):
        self.n, self.iters, self.target, self.start = sd["n"], sd["iters"], sd["target"], sd["start"]


class PolyDecay:
    """Per-iteration polynomial decay after the warm-up (the LARS large-batch recipe):

        lr_at(step) = target * (1 - (step - warm) / (total - warm)) ** power      for step >= warm

    with ``step`` the 0-based global iteration and ``total`` = epochs x steps per epoch.  Up to the
    end of the warm-up (``step <= warm``, the ramp is :class:`LinearWarmup`'s) it returns the target;
    past ``total`` it stays at 0.  A pure function of the step: resuming needs no state."""

    def __init__(self, optimizers, total: int, target_lr: float, warm: int = 0, power: float = 2.0):
        self.optimizers = optimizers if isinstance(optimizers, (list, tuple)) else [optimizers]
        self.total, self.warm = int(total), max(0, int(warm))
        self.target, self.power = float(target_lr), float(power)

    def lr_at(self, step: int) -> float:
        span = self.total - self.warm
        if step <= self.warm or span <= 0:
            return self.target
        f = min(1.0, (step - self.warm) / float(span))
        return self.target * (1.0 - f) ** self.power

    def set(self, step: int) -> float:
        lr = self.lr_at(step)
        for opt in self.optimizers:
            for g in opt.param_groups:
                g["lr"] = lr
        return lr
