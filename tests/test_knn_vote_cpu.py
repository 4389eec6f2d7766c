"""kNN label vote off the GPU: the reference path of Fn.knn_vote against a brute-force loop, the ARCFACE
workload with --arc-eval-knn-vote end to end, the refusal elsewhere, and the audit tool."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import main as entry
from ddp_classification_pytorch_amd.ops import functional as Fn


@pytest.mark.parametrize("weighted", [True, False])
def test_reference_path_against_brute_force(weighted):
    gen = torch.Generator().manual_seed(0)
    q, g = torch.randn(30, 16, generator=gen), torch.randn(60, 16, generator=gen)
    gl, ql = torch.randint(0, 4, (60,), generator=gen), torch.randint(0, 4, (30,), generator=gen)
    val, idx = Fn.cosine_topk_wide(q, g[:9], 12)  # three (-inf, -1) tail entries per row
    assert idx[:, 9:].eq(-1).all()
    val2, idx2 = Fn.cosine_topk_wide(q, g, 12, exclude=torch.arange(30))
    val, idx = torch.cat([val, val2]), torch.cat([idx, idx2])
    val, idx = torch.cat([val, val[:1]]), torch.cat([idx, torch.full_like(idx[:1], -1)])  # a row without neighbours
    ql = torch.cat([ql, ql, ql[:1]])
    pred, conf, agree = Fn.knn_vote(val, idx, gl, ql, temperature=0.5, weighted=weighted)
    for r in range(val.shape[0]):
        votes, W = {}, 0.0
        for j in range(12):
            if idx[r, j] >= 0:
                w = math.exp((float(val[r, j]) - float(val[r, 0])) / 0.5) if weighted else 1.0
                c = int(gl[idx[r, j]])
                votes[c], W = votes.get(c, 0.0) + w, W + w
        if not votes:
            assert (pred[r].item(), conf[r].item(), agree[r].item()) == (-1, 0.0, 0.0)
            continue
        best = max(votes.values())
        if weighted:  # fp32 against Python doubles: 12 terms, exp of |arg| <= 4
            assert votes[int(pred[r])] >= best - 1e-5
        else:
            assert int(pred[r]) == min(c for c, v in votes.items() if v == best)
        assert abs(conf[r].item() - best / W) <= 1e-5
        assert abs(agree[r].item() - votes.get(int(ql[r]), 0.0) / W) <= 1e-5
    assert Fn.knn_vote(val, idx, gl)[2] is None


COMMON = ["--model", "resnet18", "--data", "synthetic", "--dataset", "CIFAR10", "--image-size", "32", "--batchsize",
          "8", "--synthetic-train-size", "16", "--synthetic-val-size", "20", "--workers", "0", "--log-interval", "100",
          "--device", "cpu", "--epochs", "1", "--arc-eval-knn-vote", "5"]


def test_arcface_workload_writes_val_knn_vote(tmp_path):
    entry.main(["--workload", "arcface", "--out-dir", str(tmp_path)] + COMMON)
    recs = [json.loads(line) for line in open(tmp_path / "metrics.jsonl")]
    kv = [r for r in recs if r["kind"] == "val_knn_vote"]
    assert len(kv) == 1 and kv[0]["n"] == 20 and kv[0]["k"] == 5 and kv[0]["T"] == 0.07
    assert 0 <= kv[0]["top1"] <= 1 and 0 <= kv[0]["agree"] <= 1
    assert not [r for r in recs if r["kind"] == "val_knn"]
    assert "VAL-KNNVOTE Epoch 1" in open(tmp_path / "output.txt").read()


def test_other_workloads_refuse_the_flag(tmp_path):
    with pytest.raises(ValueError, match="--arc-eval-knn-vote"):
        entry.main(["--workload", "baseline", "--out-dir", str(tmp_path)] + COMMON)


def test_audit_tool_flags_flipped_labels(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import knn_audit

    gen = torch.Generator().manual_seed(1)
    labels = torch.arange(90) % 3
    feats = torch.eye(3)[labels].repeat(1, 4) + 0.05 * torch.randn(90, 12, generator=gen)  # three tight clusters
    noisy = labels.clone()
    noisy[[4, 50]] = (labels[[4, 50]] + 1) % 3
    np.save(tmp_path / "f.npy", feats.numpy())
    np.save(tmp_path / "l.npy", noisy.numpy())
    knn_audit.main(["--features", str(tmp_path / "f.npy"), "--labels", str(tmp_path / "l.npy"), "--k", "10",
                    "--device", "cpu", "--chunk", "40", "--out", str(tmp_path / "audit.npz")])
    out = np.load(tmp_path / "audit.npz")
    assert np.flatnonzero(out["suspect"]).tolist() == [4, 50]
    assert (out["pred"] == labels.numpy()).all() and out["agree"].dtype == np.float32
