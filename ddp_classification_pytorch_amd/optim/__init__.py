from .ema import WeightEMA
from .fused import FusedAdam, FusedLAMB, FusedLARS, FusedSGD
from .schedulers import LinearWarmup, MultiStepLR, PolyDecay, StepLR


def _split_1d(params, keep_1d):
    """The usual large-batch recipe: BN scales / shifts and biases (ndim <= 1) step without the
    layer-wise rate and without weight decay; every weight tensor gets both."""
    params = list(params)
    if keep_1d:
        return [dict(params=params)]
    groups = [dict(params=[p for p in params if p.ndim >= 2]),
              dict(params=[p for p in params if p.ndim <= 1], adapt=False, weight_decay=0.0)]
    return [g for g in groups if g["params"]]


def build_optimizer(name: str, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                    nesterov: bool = False, betas=(0.9, 0.999), lars_eta: float = 1e-3, lars_eps: float = 1e-8,
                    lars_keep_1d: bool = False, lamb_eps: float = 1e-6, lamb_bias_correction: bool = True,
                    lamb_keep_1d: bool = False, device_lr: bool = False, max_grad_norm: float = 0.0,
                    skip_nonfinite: bool = False, lars_trust_clip: bool = False, lamb_phi_min: float = 0.0,
                    lamb_phi_max: float = float("inf")):
    """``device_lr``: FusedSGD / FusedAdam read the learning rate from the device (FusedLARS and
    FusedLAMB always do).  ``max_grad_norm`` / ``skip_nonfinite``: global gradient-norm clipping and
    the non-finite skip of every optimizer (optim/fused.py ``_GradClip``)."""
    clip = dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    name = name.lower()
    if name == "sgd":
        return FusedSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                        device_lr=device_lr, **clip)
    if name in ("adam", "adamw"):
        return FusedAdam(params, lr=lr, betas=betas, weight_decay=weight_decay, decoupled=name == "adamw",
                         device_lr=device_lr, **clip)
    if name == "lars":
        return FusedLARS(_split_1d(params, lars_keep_1d), lr=lr, momentum=momentum, weight_decay=weight_decay,
                         nesterov=nesterov, eta=lars_eta, eps=lars_eps, trust_clip=lars_trust_clip, **clip)
    if name == "lamb":
        return FusedLAMB(_split_1d(params, lamb_keep_1d), lr=lr, betas=betas, weight_decay=weight_decay,
                         eps=lamb_eps, bias_correction=lamb_bias_correction, phi_min=lamb_phi_min,
                         phi_max=lamb_phi_max, **clip)
    raise ValueError(f"unknown optimizer {name}")


def optimizer_flags(args):
    """build_optimizer's keyword arguments from the command line (config.py)."""
    return dict(lars_eta=getattr(args, "lars_eta", 1e-3), lars_eps=getattr(args, "lars_eps", 1e-8),
                lars_keep_1d=getattr(args, "lars_keep_1d", False), lamb_eps=getattr(args, "lamb_eps", 1e-6),
                lamb_bias_correction=getattr(args, "lamb_bias_correction", True),
                lamb_keep_1d=getattr(args, "lamb_keep_1d", False), device_lr=getattr(args, "device_lr", False),
                max_grad_norm=getattr(args, "clip_grad_norm", 0.0), skip_nonfinite=getattr(args, "skip_nonfinite", False),
                lars_trust_clip=getattr(args, "lars_trust_clip", False),
                lamb_phi_min=getattr(args, "lamb_phi_min", 0.0), lamb_phi_max=getattr(args, "lamb_phi_max", float("inf")))


def build_ema(args, models, optimizer=None):
    """``--model-ema``: the :class:`WeightEMA` over every model of the loop's ``models`` dict (the optimizer's
    non-finite skip is honoured); None without the flag."""
    if not getattr(args, "model_ema", False):
        return None
    return WeightEMA(models, decay=getattr(args, "model_ema_decay", 0.9998),
                     warmup=getattr(args, "model_ema_warmup", False), optimizer=optimizer)


__all__ = ["FusedSGD", "FusedAdam", "FusedLARS", "FusedLAMB", "LinearWarmup", "MultiStepLR", "PolyDecay", "StepLR",
           "WeightEMA", "build_ema", "build_optimizer", "optimizer_flags"]
