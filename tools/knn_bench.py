"""Fused cosine top-k retrieval (Fn.cosine_topk, csrc/knn.hip) against the unfused route: the bf16 cosine
matrix [Nq, Ng] through the MFMA linear kernel (l2norm_rows + linear_fwd, as Fn.arcface_rows builds it)
followed by torch.topk.

    python tools/knn_bench.py [--shapes 10000x256,50000x256,50000x512] [--ks 1,8] [--rounds 5] [--wide] [--out FILE]

A k above 8 (or any k under ``--wide``) adds the wide route Fn.cosine_topk_wide (csrc/knn_wide.hip) and
Fn.knn_classify (the wide top-k followed by the weighted label vote over 100 random classes); the
k <= 8 kernel is timed only where it applies.

A shape NxD is Nq = Ng = N rows of width D, the validation set against itself (no exclusion: the unfused
route has none).  Timing: HIP events around blocks of calls after a warm-up, the two arms alternating
block by block; per arm the median over ``--rounds`` blocks with the spread, and the peak extra device
memory of one call.  Beside the times the MFMA work of the shape, 2 Nq Ng Dp FLOP, and that work over
the fused time.  The two routes order ties differently and the unfused one rounds the cosines to bf16,
so only the fused route's first neighbours are checked (against the unfused values, to bf16 precision)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ddp_classification_pytorch_amd import _ext  # noqa: E402
from ddp_classification_pytorch_amd.ops import functional as Fn  # noqa: E402


def _time_block(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps  # ms per call


def _peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    del out
    return extra


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="10000x256,50000x256,50000x512")
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wide", action="store_true", help="time Fn.cosine_topk_wide at k <= 8 too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs the GPU: a call time is not measured on the CPU")
    ops = _ext.hip_ops()
    dev = torch.device("cuda", 0)
    lines = [f"# knn_bench: Nq = Ng = N, {a.rounds} alternating blocks per arm, median [min .. max] ms per call",
             f"# device: {torch.cuda.get_device_name(0)}",
             "# fused: Fn.cosine_topk; unfused: l2norm_rows + linear_fwd (bf16 [Nq, Ng]) + torch.topk",
             "# wide: Fn.cosine_topk_wide; classify: Fn.knn_classify (top-k + weighted vote)"]
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.split("x"))
        x = torch.randn(N, D, device=dev, generator=torch.Generator(dev).manual_seed(N + D))
        y = torch.randint(0, 100, (N,), device=dev)
        Dp, Np = Fn.arcface_fused_dp(D), Fn.round_up(N, 64)
        flop = 2.0 * Np * Np * Dp
        steps = max(2, min(50, int(2e9 / (N * N))))  # ~ a quarter second and more of work per block
        # the unfused route in query chunks whose cosine matrix stays below 2^29 elements (1 GB of bf16):
        # the linear kernel has never been run at a larger output
        chunk = max(64, min(N, (1 << 29) // Np // 64 * 64))
        if chunk < N:
            lines.append(f"# N {N}: unfused in query chunks of {chunk} rows ({chunk * Np * 2 / 2**20:.0f} MB of bf16 "
                         f"cosines each; the whole [N, N] matrix would be {N * Np * 2 / 2**20:.0f} MB)")
        for k in (int(v) for v in a.ks.split(",")):
            def fused():
                return Fn.cosine_topk(x, x, k)

            def unfused():
                xn, _ = ops.l2norm_rows(x, Fn.round_up(D, 8), 1e-12)
                gn, _ = ops.l2norm_rows(x, Fn.round_up(D, 8), 1e-12, Np)
                parts = [torch.topk(ops.linear_fwd(xn[r:r + chunk], gn, None, 0)[:, :N], k, dim=1)
                         for r in range(0, N, chunk)]
                return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

            arms = {"fused": fused} if k <= Fn.KNN_MAX_K else {}
            if k > Fn.KNN_MAX_K or a.wide:
                arms["wide"] = lambda: Fn.cosine_topk_wide(x, x, k)  # noqa: B023 - called inside this iteration
                arms["classify"] = lambda: Fn.knn_classify(x, x, y, k)  # noqa: B023
            arms["unfused"] = unfused
            first = next(iter(arms))
            fv, uv = arms[first]()[0], unfused()[0].float()
            worst = (fv[:, 0] - uv[:, 0]).abs().max().item()  # self-matches: cosine 1 on both routes
            mem = {n: _peak_extra(f) for n, f in arms.items()}
            for f in arms.values():
                _time_block(f, steps)
            t = {n: [] for n in arms}
            for _ in range(a.rounds):
                for n, f in arms.items():  # the arms alternate
                    t[n].append(_time_block(f, steps))
            med = {n: statistics.median(v) for n, v in t.items()}
            lines.append(f"N {N:6d} D {D:3d} k {k}: MFMA work {flop / 1e12:.3f} TFLOP, {steps} calls per block, "
                         f"|{first} - unfused| first value {worst:.1e}")
            for n in arms:
                rate = f"   {flop / med[n] / 1e9:7.1f} TFLOP/s of MFMA work" if n != "unfused" else ""
                lines.append(f"    {n:8s} {med[n]:9.3f} ms  [{min(t[n]):.3f} .. {max(t[n]):.3f}]   "
                             f"extra memory {mem[n] / 2**20:8.1f} MB{rate}")
            for n in arms:
                if n != "unfused":
                    lines.append(f"    unfused / {n} time {med['unfused'] / med[n]:.2f}x, memory "
                                 f"{mem['unfused'] / max(mem[n], 1):.1f}x")
        del x
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
