"""Step time of FusedLARS against FusedSGD over ResNet-50's parameter tensors (25.6M elements).

    python tools/optim_step_bench.py [--steps 200] [--rounds 5] [--out FILE]

Both optimizers step their own copies of the same parameters and gradients (momentum 0.9, weight
decay 1e-4), eagerly and as a replayed HIP graph of one step.  Timing: HIP events around blocks of
``--steps`` steps after a warm-up, the two arms alternating block by block; the figure per arm is
the median over ``--rounds`` blocks, with the spread printed.

Byte accounting: the SGD step reads p, g, buf and writes p, buf (20 B / element); LARS reads p and g
once more for the norms (28 B / element): 1.4x the traffic, plus the norm and trust launches.  The
script prints the measured ratio and, beside it, each arm's bytes / time; it makes no statement on
where the second read of p and g is served from.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ddp_classification_pytorch_amd import _ext  # noqa: E402
from ddp_classification_pytorch_amd.models import build_model  # noqa: E402
from ddp_classification_pytorch_amd.optim import FusedLARS, FusedSGD  # noqa: E402


def _arm(cls, shapes, dev, seed, **kw):
    gen = torch.Generator().manual_seed(seed)
    ps = [(0.05 * torch.randn(s, generator=gen)).to(dev).requires_grad_(True) for s in shapes]
    for p in ps:
        p.grad = (1e-3 * torch.randn(p.shape, generator=gen)).to(dev)
    opt = cls(ps, lr=0.1, momentum=0.9, weight_decay=1e-4, **kw)
    return ps, opt


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_bench needs the GPU: a step time is not measured on the CPU")
    _ext.hip_ops()
    dev = torch.device("cuda", 0)
    shapes = [tuple(p.shape) for p in build_model("resnet50", num_classes=1000).parameters()]
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    lines = [f"# optim_step_bench: {len(shapes)} tensors, {n} elements (ResNet-50), momentum 0.9, wd 1e-4, "
             f"{a.rounds} alternating blocks of {a.steps} steps, median [min .. max] us per step",
             f"# device: {torch.cuda.get_device_name(0)}"]
    _, sgd = _arm(FusedSGD, shapes, dev, 1)
    # one adaptive group over every tensor: the full 28 B / element (build_optimizer's default split
    # leaves the 1-D tensors, 0.2 % of the elements, non-adaptive)
    _, lars = _arm(FusedLARS, shapes, dev, 1, eta=1e-3)
    arms = {"sgd": sgd.step, "lars": lars.step}
    for f in arms.values():  # first=True launches, tables, the device learning rate
        for _ in range(3):
            f()
    torch.cuda.synchronize()
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
    bytes_per = {"sgd": 20 * n, "lars": 28 * n}
    res = {}
    for mode, fns in (("eager", arms), ("graph", graphs)):
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
        ratio = res[(mode, "lars")] / res[(mode, "sgd")]
        lines.append(f"{mode:5s} LARS / SGD step-time ratio {ratio:.3f}  (traffic model 1.40; extra "
                     f"{res[(mode, 'lars')] - res[(mode, 'sgd')]:.1f} us per step)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
