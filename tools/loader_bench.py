"""Native shard loader throughput on one GPU: synthetic shard of variable-size uint8 records
(ImageNet-like 256-short-side images), RandomResizedCrop(224)+flip, batches of normalised bf16
NHWC (s2d stem layout) delivered to cuda:0.  Prints one JSON line.

    python tools/loader_bench.py --images 2048 --batch 256 --threads 8 --epochs 2

``--preset cdr|cifar|plc`` times the affine route (data/shards.py) of those workloads' training
augmentation instead; ``cifar`` packs 32x32 records and uses the CIFAR stem layout (no s2d).
``--pil-workers N`` times the path those presets had before (and keep under DCP_SHARD_AFFINE=0):
N PIL DataLoader worker processes over the same shard feeding the device prefetcher.
``--resample pil`` times the PIL-exact mode of the native loader (antialiased fixed-point resize,
nearest rotation: the bytes the PIL workers deliver) instead of the default ``fast`` one.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddp_classification_pytorch_amd.data import (DevicePrefetcher, ShardSampler, build_loader,  # noqa: E402
                                                build_transform)
from ddp_classification_pytorch_amd.data.shards import ShardDataset, ShardLoader, aug_preset, write_shard  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--prefetch", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--preset", default="nested", choices=["nested", "cdr", "cifar", "plc"])
    ap.add_argument("--pil-workers", type=int, default=0, help="time the PIL DataLoader path with N workers instead")
    ap.add_argument("--resample", default="fast", choices=["fast", "pil"], help="native loader resampling mode")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    path = os.path.join(a.dir, f"loader_bench_{os.getpid()}.dcps")

    def gen():
        for i in range(a.images):
            if a.preset == "cifar":
                yield rng.integers(0, 256, (32, 32, 3), dtype=np.uint8), i % 100
                continue
            w = int(rng.integers(256, 400))
            yield rng.integers(0, 256, (256, w, 3), dtype=np.uint8), i % 1000

    t0 = time.time()
    write_shard(path, gen())
    pack_s = time.time() - t0
    try:
        aug, size = aug_preset(a.preset, train=True, size=224, resample=a.resample)
        sampler = ShardSampler(list(range(a.images)), num_replicas=1, rank=0, shuffle=True)
        if a.pil_workers:
            ds = ShardDataset(path, build_transform(a.preset, True, size))
            ld = DevicePrefetcher(build_loader(ds, a.batch, sampler, workers=a.pil_workers, drop_last=True), "cuda",
                                  s2d=a.preset != "cifar")
            ld.set_epoch, ld.close = sampler.set_epoch, lambda: None
        else:
            ld = ShardLoader(path, a.batch, sampler=sampler, aug=aug, out_size=size, device="cuda",
                             threads=a.threads, prefetch=a.prefetch, s2d=a.preset != "cifar", drop_last=True,
                             resample=a.resample)
        ld.set_epoch(0)
        for _ in ld:  # warm-up epoch (page cache, allocator)
            pass
        torch.cuda.synchronize()
        n, t0 = 0, time.time()
        for ep in range(1, a.epochs + 1):
            ld.set_epoch(ep)
            for batch in ld:
                n += batch[1].numel()
        torch.cuda.synchronize()
        dt = time.time() - t0
        ld.close()
    finally:
        os.remove(path)
    what = {"nested": "RRC224+flip, bf16 NHWC s2d", "cdr": "RRC256+rot15+flip+crop224, bf16 NHWC s2d",
            "cifar": "pad4 crop32+flip, bf16 NHWC", "plc": "stretch256+flip+crop224, bf16 NHWC s2d"}[a.preset]
    path_name = (f"PIL DataLoader x{a.pil_workers} over the shard" if a.pil_workers
                 else "shard loader" + (" (pil-exact resampling)" if a.resample == "pil" else ""))
    print(json.dumps({"metric": f"{path_name} images/s to cuda:0 ({what})",
                      "value": round(n / dt, 1), "images": a.images, "batch": a.batch, "threads": a.threads,
                      "prefetch": a.prefetch, "resample": "PIL" if a.pil_workers else a.resample,
                      "pack_s": round(pack_s, 2)}), flush=True)


if __name__ == "__main__":
    main()
