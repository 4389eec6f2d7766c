#!/usr/bin/env python3
"""Times the Mixup / CutMix kernels against their unmixed forms in one process, interleaved.

* Input kernel: ``to_nhwc_s2d_mix`` under a Mixup, a CutMix and the identity plan against
  ``to_nhwc_s2d`` (uint8 NHWC, 224 x 224, 2x2 space-to-depth) at batch 256 and 4096.
  Byte model per source pixel: 3 B read per image touched + 8 B written (4 bf16 channel slots), so
  Mixup (both images everywhere) is (6 + 8) / (3 + 8) = 1.27x the unmixed kernel, the identity plan
  (no partner read) 1.0x and CutMix (one image per pixel) 1.0x.
* Loss kernels: ``xent_mix_fwd`` + ``xent_mix_bwd`` against ``xent_fwd`` + ``xent_bwd`` at B = 4096,
  C = 1000 and 2173, bf16.  Byte model: 1.0x (two more scalars per row); the forward reads the row
  once (the second pass hits cache), the backward reads it and writes the gradient: 6 B per logit.

Every arm is warmed up, then timed ``--repeats`` times round-robin with the other arms of its group
(HIP events around ``--iters`` launches); the median per arm is reported with its TB/s under the
byte model.  Needs a GPU: there is no CPU fallback.

    python tools/mix_bench.py [--repeats 9] [--iters 20] [--out mix.txt]
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
from ddp_classification_pytorch_amd.data.mix import MixPlan, identity_plan, plan_to_device  # noqa: E402


def time_round_robin(arms, repeats, iters):
    """arms: {name: fn} -> {name: median microseconds per call}"""
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


def input_plans(n, size):
    import numpy as np

    flip = np.arange(n, dtype=np.int32)[::-1].copy()
    ident = identity_plan(n)
    mixup = MixPlan(flip, np.full(n, 0.3, np.float32), ident.box, np.full(n, 0.3, np.float32))
    q = size // 4  # a centred half-by-half box: a quarter of the image
    box = np.tile(np.array([q, q, size - q, size - q], np.int32), (n, 1))
    cutmix = MixPlan(flip, ident.blend, box, np.full(n, 0.75, np.float32))
    return {"identity": ident, "cutmix": cutmix, "mixup": mixup}


def bench_input(K, n, size, repeats, iters, lines):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g).to(dev)
    mean = torch.tensor((0.485, 0.456, 0.406), device=dev)
    std = torch.tensor((0.229, 0.224, 0.225), device=dev)
    plans = {k: plan_to_device(p, dev) for k, p in input_plans(n, size).items()}
    arms = {"unmixed": lambda: K.to_nhwc_s2d(imgs, False, 1 / 255.0, mean, std, 2)}
    for k, p in plans.items():
        arms[k] = (lambda p=p: K.to_nhwc_s2d_mix(imgs, False, 1 / 255.0, mean, std, p.partner, p.blend, p.box, 2))
    # the identity plan is the unmixed kernel bit for bit at the size that is timed
    assert torch.equal(arms["identity"](), arms["unmixed"]())
    pix = n * size * size
    model = {"unmixed": 11, "identity": 11, "cutmix": 11, "mixup": 14}  # bytes per source pixel
    res = time_round_robin(arms, repeats, iters)
    base = res["unmixed"][0]
    for k, (med, lo, hi) in res.items():
        lines.append(f"input s2d=2 u8-nhwc {size}x{size} batch {n:5d} {k:9s} {med:9.1f} us (min {lo:.1f} max {hi:.1f}) "
                     f"{pix * model[k] / med / 1e6:6.3f} TB/s  {med / base:5.3f}x unmixed (byte model "
                     f"{model[k] / 11:.2f}x)")


def bench_loss(K, B, C, repeats, iters, lines):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    ld = (C + 7) // 8 * 8
    x = (torch.randn(B, ld, generator=g) * 2).bfloat16().to(dev)
    labels = torch.randint(0, C, (B,), generator=g).to(dev)
    partner = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=dev)
    wlab = torch.rand(B, generator=g).to(dev)
    go = torch.ones(1, device=dev)

    def plain():
        K.xent_fwd(x, labels, C, 0.1)
        return K.xent_bwd(x, labels, C, go, 1.0 / B, 0.1, True)

    def mixed():
        K.xent_mix_fwd(x, labels, partner, wlab, C, 0.1)
        return K.xent_mix_bwd(x, labels, partner, wlab, C, go, 1.0 / B, 0.1, True)

    res = time_round_robin({"xent": plain, "xent_mix": mixed}, repeats, iters)
    base = res["xent"][0]
    nbytes = B * (2 * C + 2 * C + 2 * ld)  # forward read, backward read + write
    for k, (med, lo, hi) in res.items():
        lines.append(f"loss fwd+bwd bf16 B {B} C {C:5d} {k:9s} {med:9.1f} us (min {lo:.1f} max {hi:.1f}) "
                     f"{nbytes / med / 1e6:6.3f} TB/s  {med / base:5.3f}x xent (byte model 1.00x)")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: no GPU (timings are taken on the device only)")
    K = _ext.hip_ops()
    lines = []
    for n in a.batches:
        bench_input(K, n, a.size, a.repeats, a.iters, lines)
    for C in (1000, 2173):
        bench_loss(K, 4096, C, a.repeats, a.iters, lines)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
