"""Mixup and CutMix plans: which image of a batch is mixed into which, and how.

The images are mixed on the device by the input kernels while they normalise them
(``dcp::to_nhwc_mix`` / ``to_nhwc_s2d_mix``, csrc/misc.hip) and the loss reads the label pair in its
own kernel (``dcp::xent_mix_fwd`` / ``xent_mix_bwd``, csrc/loss.hip).  The host only draws the plan
of a batch of N images of H x W -- four small arrays:

=========  ==============  ==========================================================================
partner    int32 [N]       index, inside the same batch, of the image mixed into row n
blend      fp32 [N]        weight of the row's own image outside the box; 1 = no blending
box        int32 [N, 4]    y0, x0, y1, x1 in output pixels, half open: inside it the partner's pixel
                           is pasted; y0 == y1 = no box
wlab       fp32 [N]        weight of the row's own label in the loss
=========  ==============  ==========================================================================

The identity plan (``partner = arange``, ``blend = 1``, empty boxes, ``wlab = 1``) is what an
unmixed step carries, so the batch tuple has the same shapes every step and one captured HIP graph
serves all of them.

Semantics (written from the definitions of the two papers, Zhang et al. 2018 and Yun et al. 2019):
``lam ~ Beta(alpha, alpha)``, ``partner[n] = N - 1 - n`` (the batch flipped; the middle row of an
odd batch pairs with itself).  Mixup: ``blend = wlab = lam``, no box.  CutMix: ``r = sqrt(1 - lam)``,
a box of ``int(H r) x int(W r)`` pixels around a centre drawn uniformly over the image, clipped to
the image; ``blend = 1`` and ``wlab = 1 - area / (H W)`` of the CLIPPED box.  With both alphas
positive CutMix is chosen with probability ``switch_prob``, else Mixup; the whole draw applies with
probability ``prob``.  ``mode="batch"`` draws once per batch, ``"elem"`` once per row.

Every draw is a pure function of (seed, epoch, step within the epoch, rank): numpy's Philox
generator keyed by (seed, rank) with (step, epoch) in its counter, so a resumed run redraws the
plans of the uninterrupted one.  Each rank mixes inside its own local batch.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

MODES = ("batch", "elem")


class MixPlan(NamedTuple):
    """numpy arrays on the host (:meth:`MixSampler.draw`) or tensors on the device."""
    partner: object
    blend: object
    box: object
    wlab: object


def identity_plan(n: int) -> MixPlan:
    return MixPlan(np.arange(n, dtype=np.int32), np.ones(n, dtype=np.float32), np.zeros((n, 4), dtype=np.int32),
                   np.ones(n, dtype=np.float32))


def cutmix_box(lam: float, uy: float, ux: float, H: int, W: int):
    """The clipped CutMix box of a ``lam`` and a centre at the fractions (uy, ux) of the image."""
    r = math.sqrt(max(0.0, 1.0 - float(lam)))
    ch, cw = int(H * r), int(W * r)
    cy, cx = min(int(uy * H), H - 1), min(int(ux * W), W - 1)
    y0, x0 = cy - ch // 2, cx - cw // 2
    y1, x1 = y0 + ch, x0 + cw
    y0, y1 = min(max(y0, 0), H), min(max(y1, 0), H)
    x0, x1 = min(max(x0, 0), W), min(max(x1, 0), W)
    return y0, x0, y1, x1


class MixSampler:
    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch", seed: int = 0, rank: int = 0):
        if mode not in MODES:
            raise ValueError(f"mix mode {mode!r}: one of {MODES}")
        if mixup_alpha < 0 or cutmix_alpha < 0 or not (mixup_alpha > 0 or cutmix_alpha > 0):
            raise ValueError("MixSampler needs a positive --mixup-alpha or --cutmix-alpha (and neither negative)")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError("mix probabilities lie in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def _rng(self, epoch: int, step: int):
        mask = (1 << 64) - 1
        return np.random.Generator(np.random.Philox(key=[self.seed & mask, self.rank & mask],
                                                    counter=[0, 0, int(step) & mask, int(epoch) & mask]))

    def draw(self, n: int, H: int, W: int, step: int, epoch: int = None) -> MixPlan:
        """The host plan of batch ``step`` of ``epoch`` (default: the epoch of :meth:`set_epoch`)."""
        rng = self._rng(self.epoch if epoch is None else epoch, step)
        k = n if self.mode == "elem" else 1
        # a fixed number of variates per draw, whatever the branch taken: the stream's layout
        # does not depend on the values
        u_apply, u_switch = rng.random(k), rng.random(k)
        lam_mix = rng.beta(self.mixup_alpha, self.mixup_alpha, k) if self.mixup_alpha > 0 else np.ones(k)
        lam_cut = rng.beta(self.cutmix_alpha, self.cutmix_alpha, k) if self.cutmix_alpha > 0 else np.ones(k)
        uy, ux = rng.random(k), rng.random(k)
        plan = identity_plan(n)
        for row in range(n):
            i = row if self.mode == "elem" else 0
            if not u_apply[i] < self.prob:
                continue
            cut = self.cutmix_alpha > 0 and (self.mixup_alpha <= 0 or u_switch[i] < self.switch_prob)
            plan.partner[row] = n - 1 - row
            if cut:
                y0, x0, y1, x1 = cutmix_box(lam_cut[i], uy[i], ux[i], H, W)
                area = (y1 - y0) * (x1 - x0)
                if area > 0:
                    plan.box[row] = (y0, x0, y1, x1)
                plan.wlab[row] = np.float32(1.0 - area / float(H * W))
            else:
                plan.blend[row] = plan.wlab[row] = np.float32(lam_mix[i])
        return plan

    def device_plan(self, n: int, H: int, W: int, step: int, device, epoch: int = None) -> MixPlan:
        """:meth:`draw` on ``device``: the four arrays packed into one pinned host buffer and copied
        with ``non_blocking=True`` on the current stream (the loaders call this on their side
        stream); no synchronisation.  The pinned block comes from torch's caching host allocator,
        which hands it out again only after that copy has completed."""
        return plan_to_device(self.draw(n, H, W, step, epoch), device)


def plan_to_device(plan: MixPlan, device) -> MixPlan:
    device = torch.device(device)
    n = int(plan.partner.shape[0])
    host = torch.empty(7 * n, dtype=torch.int32, pin_memory=device.type == "cuda")
    buf = host.numpy()
    buf[:n] = plan.partner
    buf[n:2 * n] = np.ascontiguousarray(plan.blend, dtype=np.float32).view(np.int32)
    buf[2 * n:3 * n] = np.ascontiguousarray(plan.wlab, dtype=np.float32).view(np.int32)
    buf[3 * n:] = np.ascontiguousarray(plan.box, dtype=np.int32).reshape(-1)
    dev = host.to(device, non_blocking=True) if device.type == "cuda" else host
    return MixPlan(dev[:n], dev[n:2 * n].view(torch.float32), dev[3 * n:].view(n, 4),
                   dev[2 * n:3 * n].view(torch.float32))
