"""Exponential moving average (EMA) of the model weights on the gfx950 ``mt_ema`` / ``mt_swap`` kernels.

For every tracked fp32 tensor ``w`` with its average ``e`` one update is, per element, in fp32

    t  = w - e                 (one rounding)
    e' = fma(omd, t, e)        (one rounding)

the ``lerp`` form of ``torch.lerp`` and timm's ``ModelEmaV3``: ``e == w`` is a fixed point bit for bit.
``omd`` ("one minus decay") is one fp32 device scalar per :class:`WeightEMA`, read by the kernel.  With
``n`` the number of updates already made,

    d_n   = decay                                 (warmup=False)
    d_n   = min(decay, (1 + n) / (10 + n))        (warmup=True: the TensorFlow rule)
    omd_n = fl32(1 - d_n)                         (fp64 on the host, rounded once)

:meth:`WeightEMA.push_decay` writes ``omd_n`` to the device when its fp32 value changed (the
``_DeviceLR.push_lr`` pattern of optim/fused.py), so one captured HIP graph follows the warm-up:
``push_decay()``, replay.  ``n`` advances in :meth:`update` and, for replays, in
:meth:`on_graph_replay` (hand the object to ``HostCounters(..., [optimizer, ema])``).

Tracked: every fp32 tensor of ``state_dict()`` of every model given (parameters and the BN running
statistics), under the key ``"<models key>.<state_dict name>"``.  Integer buffers
(``num_batches_tracked``) are not averaged: :meth:`state_dict` carries their live value.  The average
starts as a copy of the weights.

Given an optimizer with a clipping control block (``--clip-grad-norm`` / ``--skip-nonfinite``), the
kernel reads it: a step the optimizer skipped writes no average -- also not the BN statistics that a
non-finite forward pass has just poisoned in the live model.  ``n`` still advances on such a step (the
host cannot know about the skip without a sync; the same caveat as Adam's step count).

:meth:`applied` exchanges weights and averages in place (``mt_swap``: pure copies) for an evaluation
on the averaged weights and exchanges them back: no address changes, so a captured graph, the
optimizer's tables and the gradient-bucket views stay valid, and two exchanges restore every bit.

CPU: the same math with torch ops (ops/_ref.py; tests and gloo plumbing).
"""
from __future__ import annotations

import contextlib

import torch

from .. import _ext
from ..ops import _ref
from ..ops import functional as Fn
from .fused import _capturing, _TableCache


def _unwrap(m):
    from ..engine.checkpoint import _unwrap as unwrap

    return unwrap(m)


class WeightEMA:
    def __init__(self, models, decay: float = 0.9998, warmup: bool = False, optimizer=None):
        if isinstance(models, torch.nn.Module):
            models = {"model": models}
        self._models = {k: _unwrap(m) for k, m in models.items()}
        live, ints = [], []
        for mk, m in self._models.items():
            for name, t in m.state_dict().items():
                key = f"{mk}.{name}"
                if t.is_floating_point():
                    live.append((key, t))
                else:
                    ints.append(key)
        self._int_keys = ints
        self._init(live, None, decay, warmup, optimizer)

    @classmethod
    def from_pairs(cls, pairs, decay: float = 0.9998, warmup: bool = False, optimizer=None, names=None):
        """The low-level constructor: explicit ``(live, average)`` fp32 tensor pairs (views at any
        float offset are fine), tracked as they are -- the averages are NOT re-initialised."""
        self = cls.__new__(cls)
        pairs = list(pairs)
        names = list(names) if names is not None else [str(i) for i in range(len(pairs))]
        if len(names) != len(pairs):
            raise ValueError("WeightEMA.from_pairs: one name per pair")
        self._models, self._int_keys = {}, []
        self._init([(k, w) for k, (w, _) in zip(names, pairs)], [e for _, e in pairs], decay, warmup, optimizer)
        return self

    def _init(self, live, averages, decay, warmup, optimizer):
        if not 0.0 <= decay <= 1.0:
            raise ValueError("WeightEMA: decay must be in [0, 1]")
        self.decay, self.warmup = float(decay), bool(warmup)
        self.optimizer = optimizer if hasattr(optimizer, "_clip_ctl") else None
        self.n = 0                  # updates made so far (host counter, checkpointed)
        self.pushes = 0             # writes of the device scalar so far (diagnostic)
        self._omd = None            # float32[1] on the tensors' device
        self._pushed = None         # the fp32 value last written to it
        self._cache = _TableCache()
        self._tabs = None           # (table, chunks): built once, the tracked tensors never move
        self._swapped = False
        self._keys, self._live, self._avg = [], [], []
        for i, (key, w) in enumerate(live):
            w = w.detach()
            e = averages[i] if averages is not None else None
            for t, what in ((w, "tensor"), (e, "average")):
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                    raise RuntimeError(f"WeightEMA: {what} {key!r} must be contiguous fp32 (got {t.dtype}, "
                                       f"contiguous={t.is_contiguous()})")
            if e is None:
                e = w.clone(memory_format=torch.contiguous_format)
            elif e.shape != w.shape or e.device != w.device:
                raise RuntimeError(f"WeightEMA: average {key!r} must match its tensor's shape and device")
            self._keys.append(key)
            self._live.append(w)
            self._avg.append(e)
        if len(set(self._keys)) != len(self._keys):
            raise ValueError("WeightEMA: duplicate keys")
        devs = {t.device for t in self._live}
        if len(devs) > 1:
            raise RuntimeError(f"WeightEMA: every tracked tensor must live on one device (got {sorted(map(str, devs))})")
        self.device = devs.pop() if devs else torch.device("cpu")
        self._index = {k: i for i, k in enumerate(self._keys)}

    # ---------------------------------------------------------------- the decay schedule
    @property
    def num_updates(self) -> int:
        return self.n

    def decay_at(self, n: int) -> float:
        return min(self.decay, (1.0 + n) / (10.0 + n)) if self.warmup else self.decay

    def omd_at(self, n: int) -> float:
        """fl32(1 - d_n): formed in fp64, rounded once."""
        return float(torch.tensor(1.0 - self.decay_at(n), dtype=torch.float64).to(torch.float32))

    def push_decay(self):
        """Write ``omd_n`` into the device scalar on the current stream when its fp32 value changed
        since the last write (the first call creates the scalar: not during a capture)."""
        omd = self.omd_at(self.n)
        if self._omd is None:
            if _capturing():
                raise RuntimeError("WeightEMA: the device decay scalar must be created by push_decay() or an eager "
                                   "update() before capture")
            self._omd = torch.full((1,), omd, dtype=torch.float32, device=self.device)
        elif omd != self._pushed:
            self._omd.fill_(omd)
        else:
            return
        self._pushed = omd
        self.pushes += 1

    # ---------------------------------------------------------------- the update
    def _tables(self):
        if self._tabs is None:
            entries = [(w.data_ptr(), 0, e.data_ptr(), 0, 0, w.numel()) for w, e in zip(self._live, self._avg)]
            self._tabs = self._cache.get(entries, self.device)
        return self._tabs

    def _pairs(self):
        return list(zip(self._live, self._avg))

    @torch.no_grad()
    def update(self):
        """One EMA update of every tracked tensor from the live weights (call it after
        ``optimizer.step()``).  Outside a capture it pushes the decay itself; a captured update reads
        whatever :meth:`push_decay` wrote before the replay."""
        if self._swapped:
            raise RuntimeError("WeightEMA.update() inside applied(): the live model holds the averages")
        if not _capturing():
            self.push_decay()
        elif self._omd is None:
            raise RuntimeError("WeightEMA: the device decay scalar must be created by push_decay() or an eager "
                               "update() before capture")
        if self._live:
            if self.device.type == "cuda":
                table, chunks = self._tables()
                ctl = self.optimizer._clip_ctl() if self.optimizer is not None else None
                _ext.hip_ops().mt_ema(table, chunks, self._omd, ctl)
            else:
                _ref.mt_ema(self._pairs(), self._omd, skip=bool(self.optimizer is not None and self.optimizer._cpu_skip()))
        self.n += 1

    def on_graph_replay(self):
        """A captured step was replayed: its ``mt_ema`` launch made one more update."""
        self.n += 1

    # ---------------------------------------------------------------- evaluation on the average
    @torch.no_grad()
    def swap(self):
        """Exchange every tracked tensor with its average in place and invalidate the bf16 weight cache."""
        if _capturing():
            raise RuntimeError("WeightEMA: the exchange of weights and averages must not be captured into a HIP graph")
        if self._live:
            if self.device.type == "cuda":
                table, chunks = self._tables()
                _ext.hip_ops().mt_swap(table, chunks)
            else:
                _ref.mt_swap(self._pairs())
        self._swapped = not self._swapped
        Fn.bump_weight_generation()

    @contextlib.contextmanager
    def applied(self):
        """``with ema.applied():`` the live model computes on the averaged weights (and BN statistics);
        on exit -- also on an exception -- every bit of the live weights is back."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ---------------------------------------------------------------- access / persistence
    def keys(self):
        return list(self._keys)

    def average_of(self, name: str) -> torch.Tensor:
        """The average of the tensor tracked under ``name`` (the buffer itself, not a copy)."""
        if self._swapped:
            return self._live[self._index[name]]
        return self._avg[self._index[name]]

    def _live_ints(self):
        out = {}
        if self._int_keys:
            want = set(self._int_keys)
            for mk, m in self._models.items():
                for name, t in m.state_dict().items():  # folds the BN modules' pending batch counts
                    if f"{mk}.{name}" in want:
                        out[f"{mk}.{name}"] = t.detach().clone()
        return out

    def state_dict(self):
        """``averages``: a copy of every average by key, plus the live value of each integer buffer
        (``num_batches_tracked``), in ``state_dict()`` order per model: ``model_state_dict(key)`` of it
        loads into a fresh model.  ``n``, ``decay``, ``warmup``: the schedule."""
        ints = self._live_ints()
        order = []
        for mk, m in self._models.items():
            order.extend(f"{mk}.{name}" for name in m.state_dict().keys())
        order = order or self._keys
        av = {}
        for k in order:
            av[k] = self.average_of(k).detach().clone() if k in self._index else ints[k]
        return {"averages": av, "n": int(self.n), "decay": self.decay, "warmup": self.warmup}

    def model_state_dict(self, model_key: str = "model"):
        """The averaged ``state_dict`` of one model: its keys stripped of the ``"<model_key>."`` prefix."""
        pre = model_key + "."
        return {k[len(pre):]: v for k, v in self.state_dict()["averages"].items() if k.startswith(pre)}

    @torch.no_grad()
    def load_state_dict(self, state):
        """Into the existing buffers (``copy_``, never rebinding: captured pointers survive a resume).
        The schedule comes back too: ``n``, and ``decay`` / ``warmup`` as the checkpoint has them -- like
        an optimizer's learning rate, they override what the object was built with."""
        if self._swapped:
            raise RuntimeError("WeightEMA.load_state_dict() inside applied()")
        av = state["averages"]
        missing = [k for k in self._keys if k not in av]
        extra = [k for k in av if k not in self._index and k not in set(self._int_keys)]
        if missing or extra:
            raise KeyError(f"WeightEMA.load_state_dict: missing {missing[:5]}, unexpected {extra[:5]}")
        for k, e in zip(self._keys, self._avg):
            if av[k].shape != e.shape:
                raise RuntimeError(f"WeightEMA.load_state_dict: {k!r} has shape {tuple(av[k].shape)}, "
                                   f"expected {tuple(e.shape)}")
            e.copy_(av[k])
        self.n = int(state["n"])
        self.decay, self.warmup = float(state["decay"]), bool(state["warmup"])
        self._pushed = None  # the (loaded) schedule is written at the next push
