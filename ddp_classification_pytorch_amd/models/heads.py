"""Classifier heads of the reference workloads.

* :class:`MLPHead` — 2048 -> 512 -> ReLU -> C (+ optional LogSoftmax); the
  torchvision-ResNet ``fc`` replacement of BASELINE/main.py:137-142 and
  CDR/main.py:332-337 (which appends LogSoftmax), and the ARCFACE embedding
  head 2048 -> 512 -> ReLU -> 256 -> LogSoftmax (ARCFACE/arc_main.py:226-231).
* :class:`ArcMarginProduct` — additive angular margin head
  (ARCFACE/arc_main.py:130-176), computed by the fused HIP ArcFace path.
* :class:`NetClassifier` — bias-free ``feature @ W`` with W stored
  [feat_dim, nb_cls] (NESTED/model/model.py:64-76).
* :class:`ClassifierModel` — backbone (num_classes=0) + head, one module so a
  single DDP wrapper covers both (the reference wraps backbone and ARC head
  in two DDP instances, ARCFACE/arc_main.py:238-243).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ..ops import functional as Fn
from .layers import Linear


class MLPHead(nn.Module):
    def __init__(self, in_features=2048, hidden=512, out_features=1000, log_softmax=False):
        super().__init__()
        self.fc1 = Linear(in_features, hidden)
        self.fc2 = Linear(hidden, out_features)
        self.log_softmax = log_softmax
        self.out_features = out_features

    def forward(self, f):
        h = self.fc1(f, relu=True)
        y = self.fc2(h)
        if self.log_softmax:
            y = Fn.log_softmax(y, self.out_features)
        return y


class ArcMarginProduct(nn.Module):
    """cos(theta + m) margin on the target class, scaled by s; weight [out, in] (xavier init).

    ``sub_centers`` = K > 1 is Sub-center ArcFace (Deng et al., ECCV 2020): weight [out, K, in]
    (xavier init over the [out * K, in] rows), a sample scored against the nearest of a class's K
    centres.  ``forward`` then keeps the winning centre of each row's label class in the
    non-persistent buffer ``last_sub_idx`` (int32 [B]).

    ``sample_rate`` < 1 is Partial FC (An et al., CVPR 2022): in training mode ``forward`` scores a
    row against the batch's labels and a random share of the other classes
    (:func:`Fn.arcface_partial_loss`) and keeps the sampled classes in the non-persistent buffer
    ``last_sample_idx`` (int32 [Cs]); evaluation runs the full head.  Not with sub-centres."""

    def __init__(self, in_features=256, out_features=2173, s=30.0, m=0.50, easy_margin=True, sub_centers=1,
                 sample_rate=1.0):
        super().__init__()
        self.sample_rate = float(sample_rate)
        if not 0.0 < self.sample_rate <= 1.0:
            raise ValueError(f"ArcMarginProduct covers 0 < sample_rate <= 1, got {sample_rate}")
        if self.sample_rate < 1.0 and int(sub_centers) > 1:
            raise ValueError("Partial FC (sample_rate < 1) covers sub_centers = 1 only: the sampled head has no "
                             f"sub-centre kernel, got sub_centers = {sub_centers}")
        self.in_features, self.out_features = in_features, out_features
        self.s, self.m, self.easy_margin = s, m, easy_margin
        self.sub_centers = int(sub_centers)
        if self.sub_centers == 1:
            self.weight = nn.Parameter(torch.empty(out_features, in_features))
            nn.init.xavier_uniform_(self.weight)
            if self.sample_rate < 1.0:
                self.register_buffer("last_sample_idx", torch.zeros(0, dtype=torch.int32), persistent=False)
        else:
            Fn.arcface_sub_check(self.sub_centers, in_features)
            w = torch.empty(out_features * self.sub_centers, in_features)
            nn.init.xavier_uniform_(w)
            self.weight = nn.Parameter(w.view(out_features, self.sub_centers, in_features))
            self.register_buffer("last_sub_idx", torch.zeros(0, dtype=torch.int32), persistent=False)
        self.cos_m, self.sin_m = math.cos(m), math.sin(m)
        self.th, self.mm = math.cos(math.pi - m), math.sin(math.pi - m) * m

    def forward(self, x, label, return_logits=False):
        """-> (mean CE loss over margin logits, label rank, margin logits or empty)."""
        if self.sample_rate < 1.0 and self.training:
            if return_logits:
                raise ValueError("Partial FC (sample_rate < 1) writes no logits in training mode: return_logits "
                                 "needs the full head (eval mode, or sample_rate = 1)")
            loss, rank, self.last_sample_idx = Fn.arcface_partial_loss(x, self.weight, label, self.s, self.m,
                                                                       self.easy_margin, self.sample_rate)
            return loss, rank, torch.empty(0, device=x.device)
        if self.sub_centers == 1:
            return Fn.arcface_loss(x, self.weight, label, self.s, self.m, self.easy_margin, return_logits)
        loss, rank, logits, self.last_sub_idx = Fn.arcface_loss(x, self.weight, label, self.s, self.m,
                                                                self.easy_margin, return_logits, return_sub_idx=True)
        return loss, rank, logits

    @torch.no_grad()
    def margin_logits(self, x, label):
        """The reference's output tensor (ARCFACE/arc_main.py:157-176) in plain torch math (with
        sub-centres: the max over a class's K cosines first)."""
        cos = torch.nn.functional.linear(torch.nn.functional.normalize(x.float()),
                                         torch.nn.functional.normalize(self.weight.float().flatten(0, -2)))
        if self.sub_centers > 1:
            cos = cos.view(-1, self.out_features, self.sub_centers).amax(2)
        sine = torch.sqrt((1.0 - cos.pow(2)).clamp(0, 1))
        phi = cos * self.cos_m - sine * self.sin_m
        phi = torch.where(cos > 0, phi, cos) if self.easy_margin else torch.where(cos > self.th, phi, cos - self.mm)
        one_hot = torch.zeros_like(cos).scatter_(1, label.view(-1, 1).long(), 1)
        return (one_hot * phi + (1.0 - one_hot) * cos) * self.s


class NewFC(nn.Module):
    """ARCFACE/arc_main.py:106-113 ``NewFC``: a plain Linear returning the features (unused in the
    reference's training path; provided for API parity) -- on the MFMA GEMM."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.fc = Linear(in_features, out_features)

    def forward(self, features):
        return self.fc(features)


class ArcFaceNet(nn.Module):
    """ARCFACE/arc_main.py:115-129 ``ArcFaceNet`` (dead code in the reference, kept for API parity):
    log(exp(s cos(theta_y + m)) / (sum_j exp(s cos theta_j) - exp(s cos theta_y) + exp(s cos(theta_y + m))))
    for EVERY column y (the reference's un-labelled formulation), with theta = acos(cos / 10) -- the
    reference divides the cosine by 10 before acos ("prevents underflow"); kept as written.  The
    cosine GEMM runs on the MFMA kernel; the transcendental tail is plain torch (no training path
    uses this head)."""

    def __init__(self, cls_num=10, feature_dim=2):
        super().__init__()
        self.w = nn.Parameter(torch.randn(feature_dim, cls_num))

    def forward(self, features, m=1.0, s=10.0):
        f = torch.nn.functional.normalize(features.float(), dim=1)
        w = torch.nn.functional.normalize(self.w.float(), dim=0)
        cos = Fn.linear(f.to(features.dtype), w.t().contiguous()).float()
        theta = torch.acos(cos / 10)
        num = torch.exp(s * torch.cos(theta + m))
        e = torch.exp(s * torch.cos(theta))
        den = e.sum(dim=1, keepdim=True) - e + num
        return torch.log(num / den)


class NetClassifier(nn.Module):
    def __init__(self, feat_dim, nb_cls):
        super().__init__()
        w = torch.empty(nb_cls, feat_dim)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))  # nn.Linear init, stored transposed like the reference
        self.weight = nn.Parameter(w.t().contiguous())

    def forward(self, feature):
        return Fn.linear(feature, self.weight.t())


class ClassifierModel(nn.Module):
    """backbone.forward_features -> head.  ``head`` may be any module mapping [B, F] -> logits/features."""

    def __init__(self, backbone, head):
        super().__init__()
        self.backbone, self.head = backbone, head

    def forward(self, x):
        return self.head(self.backbone.forward_features(x))
