"""kNN label-noise audit of one labelled set of embeddings: every sample is classified by the weighted vote
of its k nearest OTHER samples (leave-one-out, cosine; Fn.knn_classify: the fused top-k kernels and
knn_vote_kernel on the GPU, the reference math on the CPU).  A sample whose neighbours outvote its own label
-- the share ``agree`` of the neighbours' weight that carries its label is below ``--threshold`` -- is suspect.

    python tools/knn_audit.py --features F.npy --labels L.npy --k 50 [--temperature 0.07] [--threshold 0.5]
                              [--majority] [--chunk 16384] [--device cuda|cpu] --out audit.npz

``F.npy`` is [N, D] (D <= 512), ``L.npy`` [N] integers.  The output holds pred [N] int64, conf [N], agree [N]
fp32 and suspect [N] bool.  Dropping or relabelling the suspects is left to the caller."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ddp_classification_pytorch_amd.ops import functional as Fn  # noqa: E402


def audit(feats, labels, k, temperature=0.07, threshold=0.5, weighted=True, chunk=16384):
    """feats [N, D], labels [N] on one device -> (pred, conf, agree, suspect); queries go in chunks of
    ``chunk`` rows against the whole set (the gallery operand is prepared per chunk, a small share)."""
    N = feats.shape[0]
    outs = []
    for r in range(0, N, chunk):
        own = torch.arange(r, min(N, r + chunk), dtype=torch.int32, device=feats.device)
        outs.append(Fn.knn_classify(feats[r:r + chunk], feats, labels, k, q_labels=labels[r:r + chunk],
                                    temperature=temperature, weighted=weighted, exclude=own))
    pred, conf, agree = (torch.cat([o[i] for o in outs]) for i in range(3))
    return pred, conf, agree, agree < threshold


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--features", required=True)
    ap.add_argument("--labels", required=True)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--majority", action="store_true", help="unweighted majority vote")
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    feats = torch.from_numpy(np.load(a.features).astype(np.float32)).to(a.device)
    labels = torch.from_numpy(np.load(a.labels).astype(np.int64)).reshape(-1).to(a.device)
    if feats.dim() != 2 or labels.numel() != feats.shape[0]:
        raise SystemExit(f"features {tuple(feats.shape)} and labels {tuple(labels.shape)}: [N, D] and [N]")
    if not 1 <= a.k <= min(Fn.KNN_WIDE_MAX_K, feats.shape[0] - 1):
        raise SystemExit(f"--k covers 1 .. min({Fn.KNN_WIDE_MAX_K}, N - 1), got {a.k} for N = {feats.shape[0]}")
    pred, conf, agree, suspect = audit(feats, labels, a.k, a.temperature, a.threshold, not a.majority, a.chunk)
    np.savez(a.out, pred=pred.cpu().numpy(), conf=conf.cpu().numpy(), agree=agree.cpu().numpy(),
             suspect=suspect.cpu().numpy())
    print(f"knn_audit: N {feats.shape[0]} k {a.k} T {a.temperature:g}: kNN top1 "
          f"{100 * (pred == labels).float().mean().item():.2f} %, mean agree {agree.mean().item():.4f}, "
          f"{int(suspect.sum())} suspects (agree < {a.threshold:g})")


if __name__ == "__main__":
    main()
