#!/usr/bin/env python3
"""Times the fused supervised contrastive loss (csrc/supcon.hip) against the plain-torch [B, B] route
on the GPU, in one process, interleaved.

Arms, forward + backward from fp32 rows [B, D] with 100 classes, tau = 0.07: ``Fn.supcon_loss`` (the
fused kernels) and ``_ref.supcon_loss`` on the device (normalise, the [B, B] similarity matrix, its masks,
logsumexp and autograd).  Shapes: D = 256 at B = 1024 / 4096 / 8192, D = 512 at B = 4096.  Every arm is
warmed up, then timed ``--repeats`` times round-robin with the other (HIP events around ``--iters``
calls); the median per arm is reported, with the peak memory a call allocates above its inputs.
Needs a GPU: there is no CPU fallback.

    python tools/supcon_bench.py [--repeats 9] [--iters 10] [--out supcon.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddp_classification_pytorch_amd import _ext  # noqa: E402
from ddp_classification_pytorch_amd.ops import _ref  # noqa: E402
from ddp_classification_pytorch_amd.ops import functional as Fn  # noqa: E402

TAU = 0.07


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench(B, D, repeats, iters, lines):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(B + D)
    x = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    y = torch.randint(0, 100, (B,), generator=g).to(dev)

    def arm(loss_fn):
        def run():
            x.grad = None
            loss_fn(x, y, TAU).backward()
        return run

    arms = {"fused": arm(Fn.supcon_loss), "torch": arm(_ref.supcon_loss)}
    mem = {}
    for name, fn in arms.items():
        for _ in range(3):
            fn()
        mem[name] = peak_extra(fn)
    times = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    base = statistics.median(times["torch"])
    for name, v in times.items():
        med = statistics.median(v)
        lines.append(f"supcon fwd+bwd fp32 B {B:5d} D {D:3d} {name:5s} {med:9.1f} us (min {min(v):.1f} max {max(v):.1f}) "
                     f"{med / base:6.3f}x torch  peak extra memory {mem[name] / 2 ** 20:8.1f} MiB")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("supcon_bench: no GPU (timings are taken on the device only)")
    _ext.hip_ops()
    lines = []
    for B, D in ((1024, 256), (4096, 256), (8192, 256), (4096, 512)):
        bench(B, D, a.repeats, a.iters, lines)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
