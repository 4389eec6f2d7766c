from .fused import FusedAdam, FusedLARS, FusedSGD
from .schedulers import LinearWarmup, MultiStepLR, PolyDecay, StepLR


def build_optimizer(name: str, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                    nesterov: bool = False, betas=(0.9, 0.999), lars_eta: float = 1e-3, lars_eps: float = 1e-8,
                    lars_keep_1d: bool = False):
    name = name.lower()
    if name == "sgd":
        return FusedSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
    if name in ("adam", "adamw"):
        return FusedAdam(params, lr=lr, betas=betas, weight_decay=weight_decay, decoupled=name == "adamw")
    if name == "lars":
        # the usual large-batch recipe: BN scales / shifts and biases (ndim <= 1) take plain momentum
        # SGD without weight decay; every weight tensor gets the layer-wise rate and the decay
        params = list(params)
        if lars_keep_1d:
            groups = [dict(params=params)]
        else:
            groups = [dict(params=[p for p in params if p.ndim >= 2]),
                      dict(params=[p for p in params if p.ndim <= 1], adapt=False, weight_decay=0.0)]
            groups = [g for g in groups if g["params"]]
        return FusedLARS(groups, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                         eta=lars_eta, eps=lars_eps)
    raise ValueError(f"unknown optimizer {name}")


__all__ = ["FusedSGD", "FusedAdam", "FusedLARS", "LinearWarmup", "MultiStepLR", "PolyDecay", "StepLR",
           "build_optimizer"]
