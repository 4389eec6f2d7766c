"""The noise-robust losses (csrc/loss_robust.hip) as their textbook formulas, differentiated by
autograd; shared by test_loss_robust_cpu.py and test_loss_robust_gpu.py.

Evaluated in fp64 it is the reference; evaluated in fp32 (``dtype``) on the same inputs it is the
yardstick: the error an fp32 evaluation of the same formula makes, from which the GPU test derives
its bound.  ``x`` holds the values the kernel reads (already rounded to bf16 where it reads bf16).
"""
import math

import torch

from tests import head_ref as R

A = -math.log(1e-4)
LO, HI = 1e-4, 1 - 1e-4


def robust(x, labels, C, plan, g, dtype=torch.float64, table=None, idx=None):
    """plan: ("gce", q) | ("sce", alpha, beta) | ("elr", lam, mom) -> dict: loss [B], grad [B, C] of
    g * sum(loss), lse [B], rank [B], valid [B], table (elr: the updated copy, else None).  A row whose
    label is outside [0, C) has loss 0, a zero gradient row and leaves its table row alone."""
    x = x.detach().cpu().to(dtype)[:, :C].clone().requires_grad_(True)
    lab, valid, safe = R.label_info(labels, C)
    lse = torch.logsumexp(x, 1)
    xa = x.gather(1, safe[:, None]).squeeze(1)
    ce = lse - xa
    p = torch.exp(x - lse[:, None])
    pa = torch.exp(-ce)
    hp = [R.f32(v) for v in plan[1:]]  # the kernel receives them as float
    if plan[0] == "gce":
        loss = (1 - pa ** hp[0]) / hp[0]
    elif plan[0] == "sce":
        loss = hp[0] * ce + hp[1] * A * (1 - pa)
    else:
        lam, mom = hp
        table = table.detach().cpu().to(dtype).clone()
        rows = idx.cpu().long()
        pc = p.clamp(LO, HI)
        t = mom * table[rows] + (1 - mom) * (pc / pc.sum(1, keepdim=True)).detach()
        table[rows[valid]] = t[valid]
        loss = ce + lam * torch.log(1 - (pc * t).sum(1))
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    (float(g) * loss.sum()).backward()
    xd = x.detach()
    return {"loss": loss.detach(), "grad": x.grad, "lse": lse.detach(), "valid": valid,
            "rank": (xd > xd.gather(1, safe[:, None])).sum(1), "table": table if plan[0] == "elr" else None}
