#!/usr/bin/env python3
"""Times ``dcp::rand_augment`` (csrc/randaug.hip) and the shard loader with and without it.

* Kernel: microseconds per batch of 256 and of 4096 uint8 images of 224 x 224 under four plans --
  identity, pointwise only (Brightness then Solarize), the default ``2,9`` draw of the sampler, and the
  worst case (Sharpness then Rotate, both out of place) -- next to ``to_nhwc`` on the same batch, arms
  interleaved.  Byte model per pixel: 3 B read + 3 B written, plus 6 B for every out-of-place op that is
  followed by another op (a 224 x 224 image fills the LDS, so the intermediate goes through global
  memory); the sampled plan's model is averaged over its rows.  The plans are packed on the device
  beforehand, so the figures are the kernel's.
* Loader: img/s of a ``ShardLoader`` (nested train preset, 224 x 224, batch 256) over a synthetic shard
  with and without ``RandAugSampler(2, 9)``, alternating, and of 16 worker processes computing the same
  bytes with ``apply_pil``.

Needs a GPU: there is no CPU fallback.

    python tools/randaug_bench.py [--repeats 7] [--iters 10] [--out randaug.txt]
"""
import argparse
import multiprocessing as mp
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddp_classification_pytorch_amd import _ext  # noqa: E402
from ddp_classification_pytorch_amd.data import randaug as ra  # noqa: E402
from tools.mix_bench import time_round_robin  # noqa: E402


def model_bytes_per_pixel(plan):
    """3 + 3, plus 6 for each out-of-place op with a non-identity op after it, averaged over the rows."""
    extra = 0
    for row in plan.op:
        live = [o for o in row.tolist() if o != ra.IDENTITY]
        extra += sum(6 for i, o in enumerate(live[:-1]) if o in ra.GEOMETRIC or o == ra.SHARPNESS)
    return 6 + extra / plan.op.shape[0]


def bench_kernel(K, n, size, repeats, iters, lines):
    dev = torch.device("cuda", 0)
    imgs = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    mean = torch.tensor((0.485, 0.456, 0.406), device=dev)
    std = torch.tensor((0.229, 0.224, 0.225), device=dev)
    neg = np.arange(2 * n).reshape(n, 2) % 2 == 1
    plans = {"identity": ra.identity_plan(n, 2),
             "pointwise": ra.make_plan(np.tile([ra.BRIGHTNESS, ra.SOLARIZE], (n, 1)), 9, neg, size, size),
             "sampled 2,9": ra.RandAugSampler(2, 9, seed=0).plan(n, size, size, step=0),
             "sharp+rotate": ra.make_plan(np.tile([ra.SHARPNESS, ra.ROTATE], (n, 1)), 9, neg, size, size)}
    packed = {k: ra.plan_to_device(p, dev) for k, p in plans.items()}
    arms = {"to_nhwc": lambda: K.to_nhwc(imgs, False, 8, 1 / 255.0, mean, std)}
    for k, p in packed.items():
        arms[k] = (lambda p=p: K.rand_augment(imgs, p))
    assert torch.equal(arms["identity"](), imgs)
    res = time_round_robin(arms, repeats, iters)
    pix = n * size * size
    model = {k: model_bytes_per_pixel(p) for k, p in plans.items()}
    model["to_nhwc"] = 3 + 16
    base = res["to_nhwc"][0]
    for k, (med, lo, hi) in res.items():
        lines.append(f"kernel u8-nhwc {size}x{size} batch {n:5d} {k:13s} {med:9.1f} us (min {lo:.1f} max {hi:.1f}) "
                     f"{model[k]:5.2f} B/px model -> {pix * model[k] / med / 1e6:6.3f} TB/s  {med / base:6.3f}x to_nhwc")


_PIL_IMAGES = {}


def _pil_init(n, size):
    torch.set_num_threads(1)  # one core per worker, as DataLoader workers run
    _PIL_IMAGES["x"] = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, size, size, 3), dtype=np.uint8))


def _pil_worker(step):
    imgs = _PIL_IMAGES["x"]
    n, size = imgs.shape[0], imgs.shape[1]
    ra.apply_pil_batch(imgs, ra.RandAugSampler(2, 9, seed=0).plan(n, size, size, step=step))
    return n


def bench_pil(workers, size, lines):
    with mp.get_context("spawn").Pool(workers, initializer=_pil_init, initargs=(64, size)) as pool:
        pool.map(_pil_worker, range(workers), chunksize=1)  # start-up and imports
        t0 = time.perf_counter()
        done = sum(pool.map(_pil_worker, range(workers, 9 * workers), chunksize=1))
        dt = time.perf_counter() - t0
    lines.append(f"PIL {workers} workers apply_pil 2,9 on {size}x{size} images in memory (no decode, no crop): "
                 f"{done / dt:9.0f} img/s")


def bench_loader(size, batch, count, repeats, lines):
    from ddp_classification_pytorch_amd.data.shards import ShardLoader, aug_preset, write_shard

    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (320, 320, 3), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.dcps")
        write_shard(path, ((np.roll(base, i, axis=1)[:256 + i % 48, :256 + i % 64], i % 100) for i in range(count)))
        aug, out = aug_preset("nested", train=True, size=size)
        rates = {"plain": [], "randaugment 2,9": []}
        for rep in range(repeats + 1):
            for name in rates:
                sampler = ra.RandAugSampler(2, 9, seed=1) if name != "plain" else None
                ld = ShardLoader(path, batch_size=batch, aug=aug, out_size=out, device="cuda", threads=16, prefetch=3,
                                 s2d=True, drop_last=True, randaug=sampler)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = sum(b[0].shape[0] for b in ld)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ld.close()
                if rep:  # the first pass of each arm warms the page cache and the kernels
                    rates[name].append(n / dt)
        for name, v in rates.items():
            lines.append(f"loader alone {size}x{size} batch {batch} {count} images 16 host threads {name:16s} "
                         f"{statistics.median(v):9.0f} img/s (min {min(v):.0f} max {max(v):.0f})")
        lines.append(f"loader with / without RandAugment: {statistics.median(rates['randaugment 2,9']) / statistics.median(rates['plain']):.3f}x")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--loader-images", type=int, default=4096)
    ap.add_argument("--pil-workers", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench: no GPU (timings are taken on the device only)")
    K = _ext.hip_ops()
    lines = []
    for n in a.batches:
        bench_kernel(K, n, a.size, a.repeats, a.iters, lines)
    if a.pil_workers:
        bench_pil(a.pil_workers, a.size, lines)
    if a.loader_images:
        bench_loader(a.size, 256, a.loader_images, 3, lines)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
