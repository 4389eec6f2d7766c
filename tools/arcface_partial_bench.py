#!/usr/bin/env python3
"""Partial FC head step (sampler + operands + forward + dX + dW + scatter; csrc/arcface_pfc.hip) against
the full fused head (csrc/arcface.hip) at the same shapes, and the sampler alone.

    python tools/arcface_partial_bench.py [--batch 1024] [--classes 100000,1000000] [--dims 256,512]
                                          [--rates 1.0,0.3,0.1] [--iters 10] [--blocks 5] [--eager]

Every arm is a HIP-graph replay of one step (as main.py / bench.py run the head; ``--eager`` times
eager calls, host launch cost included).  The arms run in alternating blocks of ``--iters`` calls,
timed by device events; a cell is the median block's time per call.  "MB" is the peak memory during
one eager step beyond what stays allocated between steps (features, weight, their gradients).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddp_classification_pytorch_amd import _ext  # noqa: E402
from ddp_classification_pytorch_amd.ops import _ref  # noqa: E402
from ddp_classification_pytorch_amd.ops import functional as Fn  # noqa: E402


def make_step(x, W, lab, rate):
    """rate None: the full fused head; else the sampled op at that rate."""
    def step():
        x.grad = W.grad = None
        if rate is None:
            loss = Fn.arcface_loss(x, W, lab, 30.0, 0.5, True)[0]
        else:
            loss = Fn.arcface_partial_loss(x, W, lab, 30.0, 0.5, True, sample_rate=rate)[0]
        loss.backward()
    return step


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def peak_mb(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def time_blocks(runs, iters, blocks):
    """runs: {name: callable}; alternating blocks -> {name: median us per call}."""
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(blocks):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return {k: statistics.median(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--classes", default="100000,1000000")
    ap.add_argument("--dims", default="256,512")
    ap.add_argument("--rates", default="1.0,0.3,0.1")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--eager", action="store_true")
    a = ap.parse_args()
    k = _ext.hip_ops()
    dev = torch.device("cuda", 0)
    rates = [float(r) for r in a.rates.split(",")]
    B = a.batch
    print(f"B = {B}, {'eager calls' if a.eager else 'HIP-graph replays'}, median of {a.blocks} alternating blocks of "
          f"{a.iters} calls; us per head step")
    print(f"{'C':>8s} {'D':>4s} | {'full us':>9s} {'MB':>7s} | " +
          " | ".join(f"{'r=' + str(r):>6s} {'Cs':>7s} {'us':>9s} {'x full':>6s} {'MB':>7s}" for r in rates) +
          f" | {'sampler us':>10s}")
    for D in (int(d) for d in a.dims.split(",")):
        for C in (int(c) for c in a.classes.split(",")):
            torch.manual_seed(0)
            x = torch.randn(B, D, device=dev).requires_grad_(True)
            W = (torch.randn(C, D, device=dev) * 0.05).requires_grad_(True)
            lab = torch.randint(0, C, (B,), device=dev)
            steps = {None: make_step(x, W, lab, None), **{r: make_step(x, W, lab, r) for r in rates}}
            mem = {r: peak_mb(fn) for r, fn in steps.items()}
            seed, ctr = Fn.pfc_state(dev)
            Cs_min = _ref.pfc_num_sampled(B, C, min(rates))
            steps["sampler"] = lambda: k.pfc_sample(lab, C, Cs_min, seed, ctr)
            runs = steps if a.eager else {r: graphed(fn) for r, fn in steps.items()}
            us = time_blocks(runs, a.iters, a.blocks)
            x.grad = W.grad = None
            cells = " | ".join(f"{'':6s} {_ref.pfc_num_sampled(B, C, r):7d} {us[r]:9.1f} {us[None] / us[r]:6.2f} {mem[r]:7.1f}"
                               for r in rates)
            print(f"{C:8d} {D:4d} | {us[None]:9.1f} {mem[None]:7.1f} | {cells} | {us['sampler']:10.1f}", flush=True)
            del x, W, lab, steps, runs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
