"""Step time of the fused optimizers over ResNet-50's parameter tensors (25.6M elements): FusedLARS
against FusedSGD, FusedLAMB against FusedAdam.

    python tools/optim_step_bench.py [--steps 200] [--rounds 5] [--arms sgd,lars,adam,lamb] [--clip] [--ema] [--out FILE]

Every optimizer steps its own copy of the same parameters and gradients (weight decay 1e-4; momentum
0.9 for SGD / LARS), eagerly and as a replayed HIP graph of one step.  Timing: HIP events around
blocks of ``--steps`` steps after a warm-up, the arms alternating block by block; the figure per arm
is the median over ``--rounds`` blocks, with the spread printed.

Byte accounting per element: the SGD step reads p, g, buf and writes p, buf (20 B); LARS reads p and g
once more for the norms (28 B); Adam reads p, g, m, v and writes p, m, v (28 B); LAMB's moments pass
reads p, g, m, v and writes m, v, its update reads p, m, v and writes p (40 B).  The script prints
the measured ratios and, beside them, each arm's bytes / time; it makes no statement on where a
second read is served from.

``--clip`` adds a clipped arm per optimizer (``max_grad_norm=1``, ``skip_nonfinite``; the gradients'
norm is 5, so every step clips): the norm pass reads g once more (+4 B per element) and one
workgroup merges the 6,240 chunk sums.  It also times the norm pass and the finish kernel alone.

``--ema`` adds two arms over the tensors a WeightEMA tracks in a ResNet-50 built here (parameters and BN
running statistics): ``ema`` (mt_ema: reads w and e, writes e, 12 B per element) and ``swap`` (mt_swap:
reads and writes both, 16 B), next to ``sgd`` in the same alternating blocks.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ddp_classification_pytorch_amd import _ext  # noqa: E402
from ddp_classification_pytorch_amd.models import build_model  # noqa: E402
from ddp_classification_pytorch_amd.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, WeightEMA  # noqa: E402

# one adaptive group over every tensor for LARS / LAMB: the full traffic (build_optimizer's default
# split leaves the 1-D tensors, 0.2 % of the elements, non-adaptive)
ARMS = {
    "sgd": (FusedSGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-4), 20),
    "lars": (FusedLARS, dict(lr=0.1, momentum=0.9, weight_decay=1e-4, eta=1e-3), 28),
    "adam": (FusedAdam, dict(lr=1e-3, weight_decay=1e-4), 28),
    "lamb": (FusedLAMB, dict(lr=1e-3, weight_decay=1e-4), 40),
}
RATIOS = (("lars", "sgd"), ("lamb", "adam"), ("adam", "sgd"))
CLIP = dict(max_grad_norm=1.0, skip_nonfinite=True)
for _k in list(ARMS):
    ARMS[_k + "+clip"] = (ARMS[_k][0], dict(ARMS[_k][1], **CLIP), ARMS[_k][2] + 4)
CLIP_RATIOS = tuple((k + "+clip", k) for k in ("sgd", "adam", "lars", "lamb"))
ARMS["ema"] = (None, {}, 12)
ARMS["swap"] = (None, {}, 16)
EMA_RATIOS = (("ema", "sgd"), ("swap", "sgd"))


def _arm(cls, shapes, dev, seed, **kw):
    gen = torch.Generator().manual_seed(seed)
    ps = [(0.05 * torch.randn(s, generator=gen)).to(dev).requires_grad_(True) for s in shapes]
    for p in ps:
        p.grad = (1e-3 * torch.randn(p.shape, generator=gen)).to(dev)
    return ps, cls(ps, **kw)


def _time_block(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps  # us per step


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default="sgd,lars,adam,lamb")
    ap.add_argument("--modes", default="eager,graph")
    ap.add_argument("--clip", action="store_true", help="add a clipped arm per optimizer, the norm pass and the "
                                                        "finish kernel alone")
    ap.add_argument("--ema", action="store_true", help="add the weight-EMA update and exchange kernels over "
                                                       "ResNet-50's tracked tensors, next to sgd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_bench needs the GPU: a step time is not measured on the CPU")
    _ext.hip_ops()
    dev = torch.device("cuda", 0)
    names = [k for k in a.arms.split(",") if k and k not in ("ema", "swap")]
    if a.ema and "sgd" not in names:
        names.insert(0, "sgd")
    if a.clip:
        names += [k + "+clip" for k in names if "+" not in k]
    shapes = [tuple(p.shape) for p in build_model("resnet50", num_classes=1000).parameters()]
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    lines = [f"# optim_step_bench: {len(shapes)} tensors, {n} elements (ResNet-50), wd 1e-4, "
             f"{a.rounds} alternating blocks of {a.steps} steps, median [min .. max] us per step",
             f"# device: {torch.cuda.get_device_name(0)}"]
    opts = {k: _arm(ARMS[k][0], shapes, dev, 1, **ARMS[k][1])[1] for k in names}
    arms = {k: o.step for k, o in opts.items()}
    counts = {k: n for k in names}
    if a.ema:
        ema = WeightEMA(build_model("resnet50", num_classes=1000).to(dev), decay=0.9998)
        table, chunks = ema._tables()
        arms["ema"] = ema.update
        arms["swap"] = lambda: _ext.hip_ops().mt_swap(table, chunks)  # the kernel alone: no generation bump
        counts["ema"] = counts["swap"] = sum(ema.average_of(k).numel() for k in ema.keys())
        names += ["ema", "swap"]
        lines.append(f"# ema / swap: {len(ema.keys())} tracked tensors, {counts['ema']} elements, {chunks.shape[0]} "
                     "chunks (parameters and BN running statistics)")
    for f in arms.values():  # first launches, tables, the device learning rate and step counters
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    modes = {"eager": arms}
    if "graph" in a.modes:
        graphs = {}
        side = torch.cuda.Stream()
        for name, f in arms.items():
            g = torch.cuda.CUDAGraph()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                f()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                f()
            graphs[name] = g.replay
        modes["graph"] = graphs
    bytes_per = {k: ARMS[k][2] * counts[k] for k in names}
    res = {}
    for mode in [m for m in a.modes.split(",") if m in modes]:
        fns = modes[mode]
        for f in fns.values():
            _time_block(f, a.steps)  # warm-up of this mode
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():  # the arms alternate
                t[k].append(_time_block(f, a.steps))
        for k in fns:
            med = statistics.median(t[k])
            res[(mode, k)] = med
            lines.append(f"{mode:5s} {k:4s} {med:8.1f} us  [{min(t[k]):.1f} .. {max(t[k]):.1f}]   "
                         f"{bytes_per[k] / 1e6:.0f} MB accounted -> {bytes_per[k] / med / 1e6:.2f} TB/s")
        for num, den in RATIOS + CLIP_RATIOS + EMA_RATIOS:
            if num in fns and den in fns:
                ratio = res[(mode, num)] / res[(mode, den)]
                lines.append(f"{mode:5s} {num.upper()} / {den.upper()} step-time ratio {ratio:.3f}  (traffic model "
                             f"{ARMS[num][2] / ARMS[den][2]:.2f}; extra {res[(mode, num)] - res[(mode, den)]:.1f} us "
                             "per step)")
    clipped = [k for k in names if k.endswith("+clip")]
    if clipped:
        o = opts[clipped[0]]
        parts = {"norm pass (mt_gnorm2)": (lambda: o.norm_params(None), 4 * n), "finish (gnorm_finish)": (o._finish_norm, 0)}
        for label, (f, nbytes) in parts.items():
            _time_block(f, a.steps)
            t = [_time_block(f, a.steps) for _ in range(a.rounds)]
            med = statistics.median(t)
            rate = f"   {nbytes / 1e6:.0f} MB -> {nbytes / med / 1e6:.2f} TB/s" if nbytes else ""
            lines.append(f"eager {label:24s} {med:8.1f} us  [{min(t):.1f} .. {max(t):.1f}]{rate}")
        o.step()  # a whole step again: the finish-only blocks above merged no partials of their own epoch
        lines.append(f"# clipped arms: grad norm {float(o.grad_norm()):.4f}, coefficient {float(o.clip_coef()):.4f}, "
                     f"skipped {int(o.skipped_steps())}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
