"""ARCFACE workload (ARCFACE/arc_main.py).

ResNet-50 backbone -> 2048->512->ReLU->256->LogSoftmax "embedding"
(ARCFACE/arc_main.py:223-231, kept for parity: the margin head then
L2-normalises those log-probabilities) -> ArcMarginProduct(256 -> C, s=30,
m=0.5, easy margin) -> CE, trained jointly under DDP with Adam (default) or
SGD(momentum 0.9, wd 5e-4).  The reference wraps backbone and ARC head in two
DDP instances (two reducers); here backbone+head+margin are one module under
one DDP wrapper (one bucketed all-reduce stream, same math).

Eval: the reference applies the margin with the TRUE labels at validation
(ARCFACE/arc_main.py:368); that is the default (``--arc-eval-with-labels``),
``--arc-eval-plain-cosine`` ranks plain cosines instead.  ``--arc-eval-knn K`` adds the
label-free retrieval evaluation (engine/loop.py ``evaluate_knn``): Recall@1 / @3 / @K of every
validation embedding against the other validation embeddings.  ``--arc-eval-knn-vote K`` (K <= 256,
``--arc-knn-temperature``) classifies every validation embedding by the weighted vote of its K nearest
other validation embeddings (``evaluate_knn_vote``).

``--arc-sample-rate R`` < 1 trains with Partial FC (``Fn.arcface_partial_loss``): each step scores a
row against the batch's labels and a share R of the other classes, drawn on the device; each rank
samples against its own labels and the dense weight gradient is all-reduced as ever.  Evaluation
keeps the full head.

``--arc-supcon-weight W`` > 0 adds W times the in-batch supervised contrastive loss
(``Fn.supcon_loss``, ``--arc-supcon-temperature``) of the embedding the head receives to the step's
loss.  It is taken over each rank's local batch: no cross-rank negatives, the scope Mixup has.
"""
from __future__ import annotations

import torch.nn as nn

from ..engine.loop import ClassificationLoop
from ..config import check_knn, refuse_mix
from ..engine.runtime import build_data, setup
from ..models import build_model
from ..models.heads import ArcMarginProduct, MLPHead
from ..ops import functional as Fn
from ..optim import StepLR, build_ema, build_optimizer, optimizer_flags
from ..parallel.ddp import attach_optimizer, wrap_ddp


class ArcFaceModel(nn.Module):
    def __init__(self, backbone, embed_head, arc, supcon_weight=0.0, supcon_temperature=0.07):
        super().__init__()
        self.backbone, self.embed, self.arc = backbone, embed_head, arc
        self.supcon_weight, self.supcon_temperature = float(supcon_weight), float(supcon_temperature)

    def features(self, x):
        return self.embed(self.backbone.forward_features(x))

    def forward(self, x, labels):
        f = self.features(x)
        loss, rank, _ = self.arc(f, labels)
        if self.supcon_weight > 0:  # (0: no new kernel runs, every bit as before)
            loss = loss + self.supcon_weight * Fn.supcon_loss(f.contiguous(), labels.long(), self.supcon_temperature)
        return loss, rank


def build_arcface(args):
    backbone = build_model(args.model, num_classes=0)
    if args.pretrained:
        from ..models.pretrained import load_pretrained

        load_pretrained(backbone, args.pretrained)
    embed = MLPHead(backbone.feat_dim, args.hidden, args.embed_dim, log_softmax=True)
    arc = ArcMarginProduct(args.embed_dim, args.num_classes, s=args.arc_s, m=args.arc_m, easy_margin=args.easy_margin,
                           sub_centers=args.arc_sub_centers, sample_rate=getattr(args, "arc_sample_rate", 1.0))
    return ArcFaceModel(backbone, embed, arc, getattr(args, "arc_supcon_weight", 0.0),
                        getattr(args, "arc_supcon_temperature", 0.07))


def run(args):
    refuse_mix(args, "arcface")
    check_knn(args)
    rt = setup(args)
    train_data, val_data, _, _ = build_data(args, rt)
    model = build_arcface(args).to(rt.device)
    net = wrap_ddp(model, rt.local_rank, syncbn=args.syncbn and (rt.world > 1 or args.force_ddp), bucket_cap_mb=args.bucket_cap_mb,
                   first_bucket_mb=args.first_bucket_mb, force=args.force_ddp)
    name = args.optimizer.lower()
    wd = args.weight_decay if name in ("sgd", "lars", "lamb") else 0.0  # ARCFACE/arc_main.py:249-253
    opt = build_optimizer(name, model.parameters(), args.lr, args.momentum, wd, **optimizer_flags(args))
    attach_optimizer(net, opt)
    sched = StepLR(opt, step_size=args.step_size, gamma=args.gamma)

    def fwd_train(batch):
        return net(batch[0], batch[1])

    def fwd_eval(batch):
        x, y = batch[0], batch[1]
        f = model.features(x)
        return Fn.arcface_rows(f, model.arc.weight, y, model.arc.s, model.arc.m, model.arc.easy_margin,
                               with_margin=args.arc_eval_with_labels)

    models = {"model": model}
    # --model-ema: over every model of the dict (backbone, embedding head and the ArcFace class centres)
    loop = ClassificationLoop(args, rt, models, opt, sched, train_data, val_data, fwd_train, fwd_eval,
                              train_modules=[net], ema=build_ema(args, models, opt),
                              embed_eval=lambda batch: model.features(batch[0]))
    return loop.run()
