#!/usr/bin/env python3
"""Times the noise-robust loss kernels (csrc/loss_robust.hip) against the cross-entropy pair in one
process, interleaved.

Arms, forward + backward at B = 4096, C = 1000 and 2173, bf16 logits and gradient: ``xent_fwd`` +
``xent_bwd`` (the baseline), and ``xent_robust_fwd`` + ``xent_robust_bwd`` under gce, sce and elr.
Byte model per row (ld = C rounded up to 8): gce / sce read the row in the forward, read it and write
the gradient in the backward, 2 C + 2 C + 2 ld bytes; elr adds the target row's read and write in the
forward and its read in the backward, + 12 C.  The cross-entropy pair is charged the same 2 C + 2 C +
2 ld (its re-reads hit cache), so the TB/s columns compare like with like.

Every arm is warmed up, then timed ``--repeats`` times round-robin with the others (HIP events around
``--iters`` launches); the median per arm is reported.  Needs a GPU: there is no CPU fallback.

    python tools/robust_loss_bench.py [--repeats 9] [--iters 20] [--out robust.txt]
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


def time_round_robin(arms, repeats, iters):
    """arms: {name: fn} -> {name: (median, min, max) microseconds per call}"""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def bench(K, B, C, repeats, iters, lines):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    ld = (C + 7) // 8 * 8
    x = (torch.randn(B, ld, generator=g) * 2).bfloat16().to(dev)
    labels = torch.randint(0, C, (B,), generator=g).to(dev)
    idx = torch.randperm(B, generator=g).to(dev)
    table = torch.zeros(B, C, device=dev)
    go = torch.ones(1, device=dev)

    def plain():
        K.xent_fwd(x, labels, C, 0.0)
        return K.xent_bwd(x, labels, C, go, 1.0 / B, 0.0, True)

    def robust(mode, a0, a1, t=None, i=None):
        def run():
            _, _, rec = K.xent_robust_fwd(x, labels, C, mode, a0, a1, t, i)
            return K.xent_robust_bwd(x, labels, C, rec, mode, a0, t, i, go, 1.0 / B, True)
        return run

    arms = {"xent": plain, "gce": robust(0, 0.7, 0.0), "sce": robust(1, 1.0, 1.0),
            "elr": robust(2, 3.0, 0.7, table, idx)}
    res = time_round_robin(arms, repeats, iters)
    base = res["xent"][0]
    row = B * (2 * C + 2 * C + 2 * ld)
    nbytes = {"xent": row, "gce": row, "sce": row, "elr": row + B * 12 * C}
    for k, (med, lo, hi) in res.items():
        lines.append(f"loss fwd+bwd bf16 B {B} C {C:5d} {k:5s} {med:9.1f} us (min {lo:.1f} max {hi:.1f}) "
                     f"{nbytes[k] / med / 1e6:6.3f} TB/s  {med / base:5.3f}x xent (byte model "
                     f"{nbytes[k] / row:.2f}x)")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("robust_loss_bench: no GPU (timings are taken on the device only)")
    K = _ext.hip_ops()
    lines = []
    for C in (1000, 2173):
        bench(K, 4096, C, a.repeats, a.iters, lines)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
