"""Retrieval evaluation off the GPU: the reference path of Fn.cosine_topk against a brute-force loop, the
ARCFACE workload with --arc-eval-knn end to end, the refusal elsewhere, and the 2-rank gathering."""
import json
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import main as entry
from ddp_classification_pytorch_amd.engine.loop import knn_counts
from ddp_classification_pytorch_amd.ops import functional as Fn


def test_reference_path_against_brute_force():
    gen = torch.Generator().manual_seed(0)
    q, g = torch.randint(-2, 3, (40, 24), generator=gen).float(), torch.randint(-2, 3, (50, 24), generator=gen).float()
    ql, gl = torch.randint(0, 4, (40,), generator=gen), torch.randint(0, 4, (50,), generator=gen)
    ex = torch.arange(40, dtype=torch.int32)
    k = 6
    val, idx, hit = Fn.cosine_topk(q, g, k, normalize=False, exclude=ex, q_labels=ql, g_labels=gl)
    for r in range(40):
        cand = sorted((-float(q[r] @ g[c]), c) for c in range(50) if c != r)[:k]  # score desc, index asc
        assert [c for _, c in cand] == idx[r].tolist() and [-s for s, _ in cand] == val[r].tolist()
        hits = [j for j, (_, c) in enumerate(cand) if gl[c] == ql[r]]
        assert hit[r].item() == (hits[0] if hits else k)
    v1, i1 = Fn.cosine_topk(q[:2], g[:1], 3, normalize=False)  # fewer candidates than k
    assert i1[:, 1:].eq(-1).all() and v1[:, 1:].eq(-float("inf")).all() and i1[:, 0].eq(0).all()


COMMON = ["--model", "resnet18", "--data", "synthetic", "--dataset", "CIFAR10", "--image-size", "32", "--batchsize",
          "8", "--synthetic-train-size", "16", "--synthetic-val-size", "20", "--workers", "0", "--log-interval", "100",
          "--device", "cpu", "--epochs", "1", "--arc-eval-knn", "3"]


def test_arcface_workload_writes_val_knn(tmp_path):
    entry.main(["--workload", "arcface", "--out-dir", str(tmp_path)] + COMMON)
    recs = [json.loads(line) for line in open(tmp_path / "metrics.jsonl")]
    kn = [r for r in recs if r["kind"] == "val_knn"]
    assert len(kn) == 1 and kn[0]["n"] == 20 and kn[0]["k"] == 3
    assert 0 <= kn[0]["recall1"] <= kn[0]["recall3"] <= kn[0]["recallK"] <= 1
    assert "VAL-KNN Epoch 1" in open(tmp_path / "output.txt").read()


def test_other_workloads_refuse_the_flag(tmp_path):
    with pytest.raises(ValueError, match="--arc-eval-knn"):
        entry.main(["--workload", "baseline", "--out-dir", str(tmp_path)] + COMMON)


def _data():
    gen = torch.Generator().manual_seed(5)
    return torch.randn(23, 16, generator=gen), torch.randint(0, 3, (23,), generator=gen)


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    f, y = _data()
    acc = knn_counts(f[rank::world], y[rank::world], 4)  # unequal shares: 12 and 11 rows
    dist.all_reduce(acc)
    if rank == 0:
        torch.save(acc, os.path.join(out_dir, "acc.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_count_what_one_process_counts():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, port, d), nprocs=2, join=True)
        got = torch.load(os.path.join(d, "acc.pt"), weights_only=True)
    one = knn_counts(*_data(), 4)
    assert one[3].item() == 23 and 0 < one[1].item() <= one[2].item() <= one[0].item()
    assert torch.equal(got, one)
