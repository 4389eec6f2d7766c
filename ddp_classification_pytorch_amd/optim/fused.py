"""Fused multi-tensor SGD / Adam on the gfx950 ``mt_sgd`` / ``mt_adam`` kernels.

Drop-in ``torch.optim.Optimizer`` subclasses (param groups, state_dict,
LR schedulers all work).  Semantics follow torch.optim.SGD / Adam exactly
(momentum buffer initialised to the first gradient; Adam bias correction;
L2 weight decay added to the gradient, or decoupled for AdamW), which the
reference uses at BASELINE/main.py:153 (SGD mom 0.9), ARCFACE/arc_main.py:249-253
(Adam / SGD wd 5e-4), NESTED/train.py:386-392 and PLC/utils.py:237 (nesterov).

GPU: one kernel launch per parameter group updates every tensor; the device
table of (param, grad, state) pointers is rebuilt only when a pointer changes.
CPU: the same math with torch ops (tests / gloo plumbing).

HIP-graph replay (engine/graph.py): a replayed step re-runs the captured kernels with
their captured arguments.  Adam's bias corrections therefore come from a device step
counter that the captured step itself increments (``mt_adam(step_dev=...)``), and
:meth:`FusedAdam.on_graph_replay` advances the host ``state["step"]`` mirrors so
``state_dict`` / resume see the true count.  SGD has no step-dependent argument; the
learning rate of a captured step is the one at capture (the grapher recaptures when it
changes) unless the optimizer was built with ``device_lr=True``: the kernels then read the
rate from a device scalar that :meth:`push_lr` keeps current, and one capture follows a
per-iteration schedule.

:class:`FusedLARS` (layer-wise adaptive rate scaling for large global batches) adds a per-tensor
trust ratio in front of the SGD update (``mt_lars``), :class:`FusedLAMB` one in front of Adam's
(``mt_lamb``); both always read their learning rate from the device.

All four take ``max_grad_norm`` / ``skip_nonfinite``: global gradient-norm clipping and the non-finite
skip, computed on the device and read by the update kernels (:class:`_GradClip`).
"""
from __future__ import annotations

import math

import torch

from .. import _ext
from ..ops import functional as Fn

CHUNK = 4096


class _TableCache:
    """Device tables of one launch: the (param, grad, state..., numel) entries, rebuilt when a
    pointer changes (every eager step when grads are set to None), and the (entry, chunk) work
    list, which depends only on the tensor sizes and is built once (a per-step Python loop over
    ResNet-50's 6,240 chunks cost milliseconds of host time per eager step)."""

    def __init__(self):
        self.key = None
        self.sizes = None
        self.table = None
        self.chunks = None

    def get(self, entries, device):
        key = tuple((e[0], e[1], e[2], e[3], e[5]) for e in entries)
        if key != self.key:
            sizes = tuple(e[5] for e in entries)
            if sizes != self.sizes:
                counts = torch.tensor([(n + CHUNK - 1) // CHUNK for n in sizes], dtype=torch.int64)
                ent = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int64), counts)
                first = torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)
                ch = torch.stack([ent, torch.arange(ent.numel(), dtype=torch.int64) - first], 1)
                self.chunks = Fn.table_to_device(ch.to(torch.int32), torch.int32, device).view(-1, 2)
                self.sizes = sizes
            # graph-capture safe uploads (grads of a captured step live in the graph pool: the
            # table is rebuilt once during capture and replayed from the fill kernel's arguments)
            self.table = Fn.table_to_device([list(e) for e in entries], torch.int64, device).view(-1, 6)
            self.key = key
        return self.table, self.chunks


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _DeviceLR:
    """The device learning rate of the fused optimizers.  With ``self.device_lr`` each group owns a
    ``float32[1]`` device tensor that the update kernel reads.  ``group["lr"]`` stays the host truth
    (schedulers, checkpoints, logging); :meth:`push_lr` writes it to the device when it changed.  A
    HIP-graph replay therefore follows a per-iteration schedule without recapture: change
    ``group["lr"]``, call ``push_lr()``, replay.  The training loop decides on the per-instance
    ``device_lr`` attribute (always true on FusedLARS / FusedLAMB, opt-in on FusedSGD / FusedAdam)."""

    device_lr = False

    def _init_device_lr(self, device_lr):
        self.device_lr = bool(device_lr)
        self._lr_dev = {}        # group index -> [float32[1] device tensor, host value last written]

    def push_lr(self):
        """Write each group's ``lr`` into its device scalar on the current stream if the host value
        changed since the last write; a no-op otherwise (and before the first GPU step, which creates
        the scalars from the learning rates of that moment, and without ``device_lr``)."""
        for gi, ent in self._lr_dev.items():
            lr = float(self.param_groups[gi]["lr"])
            if ent[1] != lr:
                ent[0].fill_(lr)
                ent[1] = lr

    def _lr_tensor(self, gi, group, device):
        ent = self._lr_dev.get(gi)
        if ent is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: the device learning rate must be created by an eager "
                                   "step before capture")
            lr = float(group["lr"])
            ent = self._lr_dev[gi] = [torch.full((1,), lr, dtype=torch.float32, device=device), lr]
        return ent[0]

    def _forget_pushed_lr(self):
        for ent in self._lr_dev.values():
            ent[1] = None  # the (loaded) learning rates are written at the next push


class _ClipState:
    """Device state of one optimizer's clipping: the control block (float32[8]: coefficient, skip flag,
    norm, skipped count, epoch; see ``ClipCtl`` in csrc/launchers.h), the partials (one slot per
    4096-element chunk of every parameter) and each slot's ``grad_scale``."""

    def __init__(self):
        self.sig = None          # numels per group: the slot layout depends on nothing else
        self.ctl = None
        self.partials = self.slot_gs = None
        self.slot0 = {}          # id(param) -> its first slot
        self.gs = None           # the groups' grad_scale last written to slot_gs
        self.spans = []          # (first slot, slot count) per group
        self.tables = {}
        self.fast = {}           # launch key -> (pointer fingerprint, table, chunks, slots)


class _GradClip:
    """Global gradient-norm clipping and the non-finite skip of the fused optimizers.

        norm = fl32(sqrt(sum over every parameter with a gradient of (grad_scale * g)^2))   (fp64 sum)
        coef = max_grad_norm / (norm + 1e-6)  in fp32, replaced by 1 when it exceeds 1
        the step = the plain step with grad_scale' = fl32(grad_scale * coef), and nothing else

    which is ``torch.nn.utils.clip_grad_norm_`` in front of the step.  The norm is global over all
    groups of ONE optimizer: a workload that builds two optimizers clips each on its own.  With
    ``skip_nonfinite`` a step whose norm is inf or NaN changes no parameter, momentum buffer, moment
    or trust ratio (``max_grad_norm=0`` then computes the norm for the flag only, coefficient 1).
    Adam's and LAMB's bias-correction step count still advances on a skipped step, on the device and
    on the host -- the host cannot know about the skip without a sync -- unlike a GradScaler-skipped
    ``torch.optim.Adam`` step, which leaves the count alone.  A skipped FIRST step of a momentum
    buffer leaves it zero and the next step treats it as an ordinary one (identical with dampening 0).

    GPU: ``mt_gnorm2`` writes one fp32 sum of g^2 per chunk into that parameter's fixed slots (ordered
    by group and position in the group, so the merge order and the bits of the norm do not depend on
    the entry point or launch order), ``gnorm_finish`` merges them in fp64 into the control block
    that every update kernel reads.  Nothing is read on the host: a captured step clips, does not
    clip, or skips from replay to replay purely from the data.  The control block is created by an
    eager step before capture, like the device learning rate.

    The bucket engine calls :meth:`norm_params` per bucket behind its all-reduce and
    :meth:`step_after_norms` once at the end of backward (``needs_global_norm`` selects that route).
    """

    needs_global_norm = False

    def _init_clip(self, max_grad_norm, skip_nonfinite):
        if not max_grad_norm >= 0:
            raise ValueError("max_grad_norm must be >= 0 (0: no clipping)")
        self.max_grad_norm = float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.needs_global_norm = self.max_grad_norm > 0 or self.skip_nonfinite
        self._clip = _ClipState()
        self._cpu_sums = {}      # CPU: id(param) -> fp64 sum of g^2 of this step
        self._cpu_clip = None    # CPU: (coef, skip, norm, skipped count) of the last step

    # ---------------------------------------------------------------- accessors (no sync)
    def _clip_field(self, i, as_int=False):
        if self._cpu_clip is not None:
            return self._cpu_clip[i]
        ctl = self._clip.ctl
        if ctl is None:
            return None
        return (ctl.view(torch.int32) if as_int else ctl)[i]

    def grad_norm(self):
        """The global gradient norm of the last step as a device scalar view; None before it."""
        return self._clip_field(2)

    def clip_coef(self):
        """The coefficient the last step applied (1: not clipped; NaN: a NaN norm without skipping)."""
        return self._clip_field(0)

    def skipped_steps(self):
        """The running count of skipped steps (int32 device scalar view; diagnostic, not checkpointed)."""
        return self._clip_field(3, as_int=True)

    # ---------------------------------------------------------------- device state
    def _clip_state(self, device):
        st = self._clip
        sig = tuple(tuple(p.numel() for p in g["params"]) for g in self.param_groups)
        if st.sig != sig:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: the clipping control block must be created by an eager "
                                   "step before capture")
            if st.ctl is None:
                st.ctl = torch.zeros(8, dtype=torch.float32, device=device)
                st.ctl[0] = 1.0
                st.ctl.view(torch.int32)[4] = 1  # epoch 1: the zeroed partials belong to no step
            acc, st.slot0, st.spans = 0, {}, []
            for g in self.param_groups:
                first = acc
                for p in g["params"]:
                    st.slot0[id(p)] = acc
                    acc += (p.numel() + CHUNK - 1) // CHUNK
                st.spans.append((first, acc - first))
            st.partials = torch.zeros(max(acc, 1), 2, dtype=torch.float32, device=device)
            st.sig, st.gs = sig, None
            st.tables.clear()
            st.fast.clear()
        gs = tuple(float(g["grad_scale"]) for g in self.param_groups)
        if st.gs != gs:
            per_slot = torch.cat([torch.full((max(n, 0),), v, dtype=torch.float32) for (_, n), v in zip(st.spans, gs)]
                                 + [torch.zeros(1, dtype=torch.float32)])[:st.partials.shape[0]]
            # through the fill kernel's arguments (graph-capture safe): the float bits as int32
            st.slot_gs = Fn.table_to_device(per_slot.view(torch.int32), torch.int32, device).view(torch.float32)
            st.gs = gs
        return st

    def _clip_ctl(self):
        # the norm pass of this step created it (no parameter with a gradient: nothing launches either)
        return self._clip.ctl if self.needs_global_norm else None

    def _own_with_grad(self, params=None):
        if params is None:
            return [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        gid = FusedSGD._group_index(self)
        return [p for p in params if id(p) in gid and p.grad is not None]

    @torch.no_grad()
    def norm_params(self, params):
        """The norm pass for ``params`` (one bucket, behind its all-reduce): their chunks' sums of g^2
        into their slots.  Any partition of the parameters, in any order, gives the same norm bits."""
        params = self._own_with_grad(params)
        if not params:
            return
        if not params[0].is_cuda:
            for p in params:
                g = p.grad.detach().to(torch.float64)
                self._cpu_sums[id(p)] = (g * g).sum()
            return
        name = type(self).__name__
        dev = params[0].device
        st = self._clip_state(dev)
        key = (len(params), params[0].data_ptr())
        fp = tuple((id(p), p.grad.data_ptr()) for p in params)
        hit = st.fast.get(key)
        if hit is None or hit[0] != fp:
            entries = []
            for p in params:
                if not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                    raise RuntimeError(f"{name} needs contiguous fp32 grads")
                entries.append((p.data_ptr(), p.grad.data_ptr(), 0, 0, 0, p.numel()))
            table, chunks = st.tables.setdefault(key, _TableCache()).get(entries, dev)
            slots = Fn.table_to_device([st.slot0[id(p)] for p in params], torch.int32, dev)
            hit = st.fast[key] = (fp, table, chunks, slots)
        _ext.hip_ops().mt_gnorm2(hit[1], hit[2], hit[3], st.partials, st.ctl)

    def _finish_norm(self):
        """Merge this step's partials into the norm, the coefficient and the skip flag."""
        ps = [p for g in self.param_groups for p in g["params"]]
        if not ps:
            return
        if ps[0].is_cuda:
            st = self._clip_state(ps[0].device)
            _ext.hip_ops().gnorm_finish(st.partials, st.slot_gs, self.max_grad_norm, self.skip_nonfinite, st.ctl)
            return
        total = torch.zeros((), dtype=torch.float64)
        for g in self.param_groups:  # the fixed order: by group, by position in the group
            gs = float(torch.tensor(g["grad_scale"], dtype=torch.float32))
            for p in g["params"]:
                s = self._cpu_sums.get(id(p))
                if s is not None:
                    total = total + gs * gs * s
        self._cpu_sums = {}
        norm = total.sqrt().to(torch.float32)
        coef = torch.ones((), dtype=torch.float32)
        if self.max_grad_norm > 0:
            coef = torch.tensor(self.max_grad_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
            if coef > 1:
                coef = torch.ones((), dtype=torch.float32)
        skip = bool(self.skip_nonfinite and not torch.isfinite(norm))
        count = (int(self._cpu_clip[3]) if self._cpu_clip is not None else 0) + int(skip)
        self._cpu_clip = (coef, skip, norm, torch.tensor(count, dtype=torch.int32))

    def _cpu_gs(self, group):
        """CPU path: the group's effective grad_scale, fl32(grad_scale * coef) under clipping."""
        gs = group["grad_scale"]
        if not self.needs_global_norm or self._cpu_clip is None:
            return gs
        return float(torch.tensor(gs, dtype=torch.float32) * self._cpu_clip[0])

    def _cpu_skip(self):
        return self.needs_global_norm and self._cpu_clip is not None and self._cpu_clip[1]

    def _norm_all(self):
        if self.needs_global_norm:
            self.norm_params(None)
            self._finish_norm()

    def _no_bucket_steps(self):
        if self.needs_global_norm:
            raise RuntimeError(f"{type(self).__name__}: a global gradient norm needs every gradient before any "
                               "update; use norm_params() per bucket and step_after_norms() instead of step_params()")


class FusedSGD(_GradClip, _DeviceLR, torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 grad_scale=1.0, device_lr=False, max_grad_norm=0.0, skip_nonfinite=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, grad_scale=grad_scale)
        super().__init__(params, defaults)
        self._tables = {}
        self._fast = {}          # launch key -> (pointer fingerprint, table, chunks): see _update
        self._gid = None         # id(param) -> group index (step_params), rebuilt when groups change
        self._reducer_stepped = False
        self._init_device_lr(device_lr)
        self._init_clip(max_grad_norm, skip_nonfinite)

    def mark_stepped_by_reducer(self):
        """The bucket engine (parallel/reducer.py) already applied this step per bucket: the next
        ``step()`` is a no-op (the training loop's call after backward)."""
        self._reducer_stepped = True
        Fn.bump_weight_generation()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._fast.clear()  # new momentum buffers: the cached tables point at the old ones
        self._forget_pushed_lr()

    def _group_index(self):
        sig = tuple(len(g["params"]) for g in self.param_groups)
        if self._gid is None or self._gid[0] != sig:
            self._gid = (sig, {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]})
        return self._gid[1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._reducer_stepped:
            self._reducer_stepped = False
            return loss
        if self.device_lr and not _capturing():
            self.push_lr()
        self._norm_all()
        self._step_subset(None)
        Fn.bump_weight_generation()
        return loss

    @torch.no_grad()
    def step_after_norms(self):
        """The bucket engine's end of backward under clipping: every bucket's :meth:`norm_params` has
        run; merge the norm, then update every parameter that has a gradient."""
        if self.device_lr and not _capturing():
            self.push_lr()
        self._finish_norm()
        self._step_subset(None)

    @torch.no_grad()
    def step_params(self, params):
        """Update only ``params`` (one bucket, right behind its all-reduce); every group's
        hyper-parameters apply to its own members.  The caller bumps the weight generation.
        Host cost is O(len(params)): the bucket's members are grouped by a cached param -> group
        map instead of scanning every group (the bucket engine calls this once per bucket)."""
        self._no_bucket_steps()
        if self.device_lr and not _capturing():
            self.push_lr()
        gid = self._group_index()
        by_group = {}
        for p in params:
            gi = gid.get(id(p))
            if gi is not None and p.grad is not None:
                by_group.setdefault(gi, []).append(p)
        for gi in sorted(by_group):
            self._step_group(gi, self.param_groups[gi], by_group[gi])

    def _step_subset(self, ids):
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None and (ids is None or id(p) in ids)]
            if params:
                self._step_group(gi, group, params)

    def _step_group(self, gi, group, params):
        mom = group["momentum"]
        # torch.optim.SGD initialises each momentum buffer to that parameter's first
        # gradient: parameters seen for the first time step with first=True in their own
        # launch, so a late-arriving gradient never resets the others' momentum
        fresh = set()
        for p in params:
            st = self.state[p]
            if mom != 0 and "momentum_buffer" not in st:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                fresh.add(p)
        for first, sub in ((True, [p for p in params if p in fresh]), (False, [p for p in params if p not in fresh])):
            if sub:
                self._update(gi, group, sub, first)

    def _update(self, gi, group, params, first):
        mom = group["momentum"]
        if params[0].is_cuda:
            # steady state: the parameters, their gradients (bucket views under the bucket engine)
            # and momentum buffers keep their addresses, so a pointer fingerprint of (param, grad)
            # stands in for rebuilding and comparing the whole table -- ~5x less host time per
            # step for ResNet-50 (momentum buffers only move on load_state_dict, which clears it)
            key = (gi, first, len(params), params[0].data_ptr())
            fp = tuple((p.data_ptr(), p.grad.data_ptr()) for p in params)
            hit = self._fast.get(key) if not first else None
            if hit is not None and hit[0] == fp:
                self._launch(gi, group, hit[1], hit[2], first)
                return
            entries = []
            for p in params:
                if not (p.is_contiguous() and p.grad.is_contiguous()):
                    raise RuntimeError("FusedSGD needs contiguous params and grads")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                    raise RuntimeError("FusedSGD expects fp32 master params and grads")
                buf = self.state[p].get("momentum_buffer")
                entries.append((p.data_ptr(), p.grad.data_ptr(), buf.data_ptr() if buf is not None else 0, 0, 0,
                                p.numel()))
            key = (gi, first, len(params), params[0].data_ptr())  # one table per bucket subset
            table, chunks = self._tables.setdefault(key, _TableCache()).get(entries, params[0].device)
            if not first:
                self._fast[key] = (fp, table, chunks)
            self._launch(gi, group, table, chunks, first)
            return
        if self._cpu_skip():
            return
        for p in params:
            g = p.grad * self._cpu_gs(group)
            if group["weight_decay"]:
                g = g + group["weight_decay"] * p
            if mom:
                buf = self.state[p]["momentum_buffer"]
                if first:
                    buf.copy_(g)
                else:
                    buf.mul_(mom).add_(g, alpha=1 - group["dampening"])
                g = g + mom * buf if group["nesterov"] else buf
            p.add_(g, alpha=-group["lr"])

    def _launch(self, gi, group, table, chunks, first):
        if self.device_lr or self.needs_global_norm:
            # mt_lars without a trust table is the mt_sgd step, bit for bit, with the rate read from the device
            # and / or the clipping control block applied
            _ext.hip_ops().mt_lars(table, chunks, None, None, None, group["lr"], group["momentum"], group["dampening"],
                                   group["weight_decay"], group["nesterov"], first, group["grad_scale"], 0.0, 0.0,
                                   self._lr_tensor(gi, group, table.device) if self.device_lr else None,
                                   self._clip_ctl())
            return
        _ext.hip_ops().mt_sgd(table, chunks, group["lr"], group["momentum"], group["dampening"], group["weight_decay"],
                              group["nesterov"], first, group["grad_scale"])


class FusedAdam(_GradClip, _DeviceLR, torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                 grad_scale=1.0, device_lr=False, max_grad_norm=0.0, skip_nonfinite=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled,
                        grad_scale=grad_scale)
        super().__init__(params, defaults)
        self._init_runtime(device_lr, max_grad_norm, skip_nonfinite)

    def _init_runtime(self, device_lr, max_grad_norm=0.0, skip_nonfinite=False):
        self._tables = {}
        self._dsteps = {}        # launch key -> [device int32 step, host mirror, params]
        self._captured = None    # launch keys of the step being / last captured into a HIP graph
        self._reducer_stepped = False
        self._bucket_capture_open = False
        self._gid = None
        self._init_device_lr(device_lr)
        self._init_clip(max_grad_norm, skip_nonfinite)

    def mark_stepped_by_reducer(self):
        self._reducer_stepped = True
        self._bucket_capture_open = False
        Fn.bump_weight_generation()

    def on_graph_replay(self):
        """A captured step was replayed: its kernels advanced the device step counters; advance the
        host mirrors and every stepped parameter's ``state["step"]`` to match."""
        for key in self._captured or ():
            ds = self._dsteps.get(key)
            if ds is None:
                continue
            ds[1] += 1
            for p in ds[2]:
                self.state[p]["step"] += 1

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._dsteps.clear()  # re-seeded from the loaded host step counts at the next step
        self._forget_pushed_lr()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._reducer_stepped:
            self._reducer_stepped = False
            return loss
        capturing = _capturing()
        if capturing:
            self._captured = []
        elif self.device_lr:
            self.push_lr()
        self._norm_all()
        self._step_subset(None)
        Fn.bump_weight_generation()
        return loss

    @torch.no_grad()
    def step_after_norms(self):
        """See FusedSGD.step_after_norms."""
        if _capturing():
            self._captured = []  # this capture's launch keys
        elif self.device_lr:
            self.push_lr()
        self._finish_norm()
        self._step_subset(None)

    @torch.no_grad()
    def step_params(self, params):
        """Update only ``params`` (one bucket of the bucket engine); see FusedSGD.step_params."""
        self._no_bucket_steps()
        capturing = _capturing()
        if capturing and not self._bucket_capture_open:
            self._captured = []  # the first bucket of a captured backward: this capture's launch keys
            self._bucket_capture_open = True
        if self.device_lr and not capturing:
            self.push_lr()
        gid = FusedSGD._group_index(self)
        by_group = {}
        for p in params:
            gi = gid.get(id(p))
            if gi is not None and p.grad is not None:
                by_group.setdefault(gi, []).append(p)
        for gi in sorted(by_group):
            self._step_group(gi, self.param_groups[gi], by_group[gi])

    def _step_subset(self, ids):
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None and (ids is None or id(p) in ids)]
            if params:
                self._step_group(gi, group, params)

    def _step_group(self, gi, group, params):
        for p in params:
            st = self.state[p]
            if "step" not in st:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["step"] += 1
        # bias correction is per parameter (torch.optim.Adam): one launch per distinct step count
        by_step = {}
        for p in params:
            by_step.setdefault(self.state[p]["step"], []).append(p)
        for step, sub in sorted(by_step.items()):
            self._update(gi, group, sub, step)

    def _device_step(self, key, step, params):
        """The launch's device step counter, advanced to ``step`` on the current stream."""
        ds = self._dsteps.get(key)
        if ds is None or ds[1] != step - 1:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: step counters must be seeded by an eager step before "
                                   "capture")
            ds = self._dsteps[key] = [torch.full((1,), step - 1, dtype=torch.int32, device=params[0].device),
                                      step - 1, params]
        ds[0].add_(1)  # captured with the step: every replay advances the device count
        ds[1], ds[2] = step, params
        if self._captured is not None and torch.cuda.is_current_stream_capturing():
            self._captured.append(key)
        return ds[0]

    def _update(self, gi, group, params, step):
        b1, b2 = group["betas"]
        if params[0].is_cuda:
            entries = []
            for p in params:
                st = self.state[p]
                entries.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(),
                                st["exp_avg_sq"].data_ptr(), 0, p.numel()))
            dev = params[0].device
            key = (gi, len(params), params[0].data_ptr())
            table, chunks = self._tables.setdefault(key, _TableCache()).get(entries, dev)
            _ext.hip_ops().mt_adam(table, chunks, group["lr"], b1, b2, group["eps"], group["weight_decay"], step,
                                   group["decoupled"], group["grad_scale"], self._device_step(key, step, params),
                                   self._lr_tensor(gi, group, dev) if self.device_lr else None, self._clip_ctl())
            return
        if self._cpu_skip():
            return
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        for p in params:
            st = self.state[p]
            g = p.grad * self._cpu_gs(group)
            if group["weight_decay"]:
                if group["decoupled"]:
                    p.mul_(1 - group["lr"] * group["weight_decay"])
                else:
                    g = g + group["weight_decay"] * p
            st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = st["exp_avg_sq"].sqrt() / math.sqrt(bc2) + group["eps"]
            p.addcdiv_(st["exp_avg"], denom, value=-group["lr"] / bc1)


class _LarsTables(_TableCache):
    """A LARS launch's tables plus its scratch: the per-tensor (first chunk, chunk count) spans, the
    per-chunk (sum w^2, sum g^2) partials and the per-tensor trust ratios.  Like the chunk list they
    depend only on the tensor sizes.  One per launch key: the compute stream's ``step()`` and the
    comm stream's per-bucket ``step_params()`` never share scratch."""

    def __init__(self):
        super().__init__()
        self.span_sizes = None
        self.spans = self.partials = self.trust = None

    def get(self, entries, device):
        super().get(entries, device)
        if self.sizes != self.span_sizes:
            counts = [(n + CHUNK - 1) // CHUNK for n in self.sizes]
            firsts, acc = [], 0
            for c in counts:
                firsts.append(acc)
                acc += c
            self.spans = Fn.table_to_device([[f, c] for f, c in zip(firsts, counts)], torch.int32, device).view(-1, 2)
            self.partials = torch.zeros(acc, 2, dtype=torch.float32, device=device)
            self.trust = torch.ones(len(counts), dtype=torch.float32, device=device)
            self.span_sizes = self.sizes
        return self


class FusedLARS(FusedSGD):
    """Layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017) in front of FusedSGD's update:

        g~    = grad_scale * g
        trust = eta * |w| / (|g~| + wd * |w| + eps)    if adapt and |w| > 0 and |g~| > 0, else 1
        d     = trust * (g~ + wd * w)
        buf   = d  (a parameter's first gradient)  |  momentum * buf + (1 - dampening) * d
        w    -= lr * (d + momentum * buf  if nesterov else  buf)

    GPU: per (group, first / not-first) subset the ``mt_lars`` op launches the per-chunk sums of
    squares, the per-tensor trust ratios (chunk partials merged in fp64 in a fixed order; no float
    atomics, so a step is bit-reproducible) and the update.  The trust ratio never leaves the device.

    Device learning rate: each group owns a ``float32[1]`` device tensor that the update kernel reads.
    ``group["lr"]`` stays the host truth (schedulers, checkpoints, logging); :meth:`push_lr` writes
    it to the device when it changed.  A HIP-graph replay therefore follows a per-iteration schedule
    without recapture: change ``group["lr"]``, call ``push_lr()``, replay.

    ``trust_clip=True`` is LARC's clip mode: an adaptive ratio becomes ``min(trust / lr, 1)`` (``lr`` read
    from the device; 1 when ``lr <= 0``), so the layer's rate ``lr * trust`` is ``min(eta |w| / ..., lr)``.
    ``max_grad_norm`` / ``skip_nonfinite``: see :class:`_GradClip`.
    """

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 grad_scale=1.0, eta=1e-3, eps=1e-8, adapt=True, max_grad_norm=0.0, skip_nonfinite=False,
                 trust_clip=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, grad_scale=grad_scale, eta=eta, eps=eps, adapt=adapt)
        torch.optim.Optimizer.__init__(self, params, defaults)
        self._tables = {}
        self._fast = {}          # launch key -> (pointer fingerprint, _LarsTables)
        self._gid = None
        self._reducer_stepped = False
        self._init_device_lr(True)   # push_lr / _lr_tensor: see _DeviceLR
        self._init_clip(max_grad_norm, skip_nonfinite)
        self.trust_clip = bool(trust_clip)
        self._trust = {}         # id(param) -> (trust tensor, index) of its last step
        self._ones = {}          # device -> float32[1] of 1.0 (trust_of for non-adaptive groups)
        self._via = "step"       # which entry point is stepping: part of the launch key

    def trust_of(self, p):
        """The trust ratio of ``p``'s last step as a device scalar view (no sync); 1 for a parameter
        of a non-adaptive group, None before its first step."""
        return self._trust.get(id(p))

    @torch.no_grad()
    def step(self, closure=None):
        self._via = "step"
        return super().step(closure)

    @torch.no_grad()
    def step_params(self, params):
        self._via = "bucket"
        super().step_params(params)

    @torch.no_grad()
    def step_after_norms(self):
        self._via = "bucket"
        super().step_after_norms()

    def _update(self, gi, group, params, first):
        mom, wd, gs = group["momentum"], group["weight_decay"], group["grad_scale"]
        adapt = bool(group["adapt"])
        if params[0].is_cuda:
            dev = params[0].device
            lr_dev = self._lr_tensor(gi, group, dev)
            key = (self._via, gi, first, len(params), params[0].data_ptr())
            fp = (adapt,) + tuple((p.data_ptr(), p.grad.data_ptr()) for p in params)
            hit = self._fast.get(key) if not first else None
            if hit is not None and hit[0] == fp:
                tabs = hit[1]
            else:
                entries = []
                for p in params:
                    if not (p.is_contiguous() and p.grad.is_contiguous()):
                        raise RuntimeError("FusedLARS needs contiguous params and grads")
                    if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                        raise RuntimeError("FusedLARS expects fp32 master params and grads")
                    buf = self.state[p].get("momentum_buffer")
                    entries.append((p.data_ptr(), p.grad.data_ptr(), buf.data_ptr() if buf is not None else 0, 0, 0,
                                    p.numel()))
                tabs = self._tables.setdefault(key, _LarsTables()).get(entries, dev)
                if not first:
                    self._fast[key] = (fp, tabs)
                if adapt:
                    for i, p in enumerate(params):
                        self._trust[id(p)] = tabs.trust[i]
                else:
                    one = self._ones.get(dev)
                    if one is None:
                        one = self._ones[dev] = torch.ones((), dtype=torch.float32, device=dev)
                    for p in params:
                        self._trust[id(p)] = one
            _ext.hip_ops().mt_lars(tabs.table, tabs.chunks, tabs.spans if adapt else None,
                                   tabs.partials if adapt else None, tabs.trust if adapt else None, group["lr"], mom,
                                   group["dampening"], wd, group["nesterov"], first, gs, group["eta"], group["eps"],
                                   lr_dev, self._clip_ctl(), self.trust_clip)
            return
        # CPU: the same formulas in fp32 (norms merged in fp64, as the trust kernel does)
        if self._cpu_skip():
            return
        gs = self._cpu_gs(group)
        for p in params:
            g = p.grad * gs
            trust = torch.ones((), dtype=torch.float32)
            if adapt:
                wn = (p.detach() * p.detach()).sum(dtype=torch.float64).sqrt().float()
                gn = ((p.grad * p.grad).sum(dtype=torch.float64).sqrt() * abs(gs)).float()
                if wn > 0 and gn > 0:
                    trust = group["eta"] * wn / (wd * wn + gn + group["eps"])
                    if self.trust_clip:
                        lr32 = torch.tensor(group["lr"], dtype=torch.float32)
                        trust = torch.clamp(trust / lr32, max=1.0) if lr32 > 0 else torch.ones((), dtype=torch.float32)
            self._trust[id(p)] = trust
            if wd:
                g = g + wd * p
            g = trust * g
            if mom:
                buf = self.state[p]["momentum_buffer"]
                if first:
                    buf.copy_(g)
                else:
                    buf.mul_(mom).add_(g, alpha=1 - group["dampening"])
                g = g + mom * buf if group["nesterov"] else buf
            p.add_(g, alpha=-group["lr"])


class FusedLAMB(FusedAdam):
    """LAMB (You et al. 2020): Adam's moments with a layer-wise trust ratio in front of the update.
    Per tensor, ``t`` being that parameter's step count as in FusedAdam:

        g~ = grad_scale * g
        m  = b1 m + (1 - b1) g~            v = b2 v + (1 - b2) g~^2
        r  = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)     bc_i = 1 - b_i^t, or 1 with bias_correction=False
        u  = r + wd * w
        trust = |w| / |u|   if adapt and |w| > 0 and |u| > 0, else 1
        w -= lr * trust * u

    GPU: an adaptive launch of the ``mt_lamb`` op is three kernels (moments + per-chunk sums of w^2 and
    u^2, per-tensor trust ratios merged in fp64 in a fixed order, the update on the recomputed u); a
    non-adaptive group takes one.  No float atomics: a step is bit-reproducible.  The learning rate is
    always read from the device (see :class:`_DeviceLR`), the bias corrections from FusedAdam's device
    step counter: one captured HIP graph follows both.

    ``phi_min`` / ``phi_max`` are the paper's phi: ``trust = clamp(|w|, phi_min, phi_max) / |u|`` (the
    defaults 0 and +inf leave ``|w| / |u|``).  ``max_grad_norm`` / ``skip_nonfinite``: see :class:`_GradClip`.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, grad_scale=1.0,
                 bias_correction=True, adapt=True, max_grad_norm=0.0, skip_nonfinite=False, phi_min=0.0,
                 phi_max=math.inf):
        if not 0 <= phi_min <= phi_max:
            raise ValueError("FusedLAMB needs 0 <= phi_min <= phi_max")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale,
                        bias_correction=bias_correction, adapt=adapt)
        torch.optim.Optimizer.__init__(self, params, defaults)
        self._init_runtime(True, max_grad_norm, skip_nonfinite)
        self.phi_min, self.phi_max = float(phi_min), float(phi_max)
        self._trust = {}         # id(param) -> trust ratio (device scalar view) of its last step
        self._trust_src = {}     # launch key -> what self._trust was last filled from
        self._ones = {}          # device -> float32 scalar 1.0 (trust_of for non-adaptive groups)
        self._via = "step"       # which entry point is stepping: part of the launch key

    trust_of = FusedLARS.trust_of

    @torch.no_grad()
    def step(self, closure=None):
        self._via = "step"
        return super().step(closure)

    @torch.no_grad()
    def step_params(self, params):
        self._via = "bucket"
        super().step_params(params)

    @torch.no_grad()
    def step_after_norms(self):
        self._via = "bucket"
        super().step_after_norms()

    def _update(self, gi, group, params, step):
        b1, b2 = group["betas"]
        wd, gs, eps = group["weight_decay"], group["grad_scale"], group["eps"]
        adapt, bias = bool(group["adapt"]), bool(group["bias_correction"])
        if params[0].is_cuda:
            dev = params[0].device
            entries = []
            for p in params:
                if not (p.is_contiguous() and p.grad.is_contiguous()):
                    raise RuntimeError("FusedLAMB needs contiguous params and grads")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                    raise RuntimeError("FusedLAMB expects fp32 master params and grads")
                st = self.state[p]
                entries.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(),
                                st["exp_avg_sq"].data_ptr(), 0, p.numel()))
            # step() on the compute stream and step_params() on the comm stream never share scratch
            key = (self._via, gi, len(params), params[0].data_ptr())
            tabs = self._tables.setdefault(key, _LarsTables()).get(entries, dev)
            src = (tabs.trust, adapt, tuple(id(p) for p in params))
            old = self._trust_src.get(key)
            if old is None or old[0] is not src[0] or old[1:] != src[1:]:
                self._trust_src[key] = src
                if adapt:
                    for i, p in enumerate(params):
                        self._trust[id(p)] = tabs.trust[i]
                else:
                    one = self._ones.get(dev)
                    if one is None:
                        one = self._ones[dev] = torch.ones((), dtype=torch.float32, device=dev)
                    for p in params:
                        self._trust[id(p)] = one
            _ext.hip_ops().mt_lamb(tabs.table, tabs.chunks, tabs.spans if adapt else None,
                                   tabs.partials if adapt else None, tabs.trust if adapt else None, group["lr"], b1, b2,
                                   eps, wd, step, bias, gs, self._device_step(key, step, params),
                                   self._lr_tensor(gi, group, dev), self._clip_ctl(), self.phi_min,
                                   None if math.isinf(self.phi_max) else self.phi_max)
            return
        # CPU: the same formulas in fp32 (norms merged in fp64, as the trust kernel does)
        if self._cpu_skip():
            return
        gs = self._cpu_gs(group)
        bc1, bc2 = (1 - b1 ** step, 1 - b2 ** step) if bias else (1.0, 1.0)
        for p in params:
            st = self.state[p]
            g = p.grad * gs
            st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
            u = (st["exp_avg"] / bc1) / (st["exp_avg_sq"].sqrt() / math.sqrt(bc2) + eps)
            if wd:
                u = u + wd * p
            trust = torch.ones((), dtype=torch.float32)
            if adapt:
                wn = (p.detach() * p.detach()).sum(dtype=torch.float64).sqrt().float()
                un = (u * u).sum(dtype=torch.float64).sqrt().float()
                if wn > 0 and un > 0:
                    trust = torch.clamp(wn, min=self.phi_min, max=self.phi_max) / un
            self._trust[id(p)] = trust
            p.add_(u, alpha=-float(torch.tensor(group["lr"], dtype=torch.float32) * trust))
