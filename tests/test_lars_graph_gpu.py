"""FusedLARS under HIP-graph replay and the bucket engine.

* One captured step follows a learning rate that changes before every replay (the device scalar of
  FusedLARS.push_lr): no recapture, parameters and momentum bit-equal to eager steps.
* A world-1 RCCL group: LARS fused per bucket on the side communication stream, eagerly and
  replayed from a HIP graph, bit-equal to the unwrapped model stepped by step().
* main.py --optimizer lars --lr-decay poly --graph end to end: warm-up and decay through the
  captured step; with SGD the warm-up still runs eagerly as before.
"""
import copy
import json
import os
import socket
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _no_autotune():
    """Fixed kernel configurations (what --no-autotune sets): every step runs the same kernels."""
    from ddp_classification_pytorch_amd import _ext, tuning

    _ext.hip_ops().set_tuning(tuning.slot("autotune"), 0)


def test_step_grapher_follows_device_learning_rate_without_recapture():
    from ddp_classification_pytorch_amd.engine.graph import HostCounters, StepGrapher
    from ddp_classification_pytorch_amd.models import build_model, input_layout
    from ddp_classification_pytorch_amd.ops import functional as Fn
    from ddp_classification_pytorch_amd.optim import build_optimizer

    _no_autotune()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = build_model("resnet18", num_classes=10).to(dev)
    gen = torch.Generator().manual_seed(1)
    batches = [(torch.randint(0, 256, (8, 3, 32, 32), dtype=torch.uint8, generator=gen).to(dev),
                torch.randint(0, 10, (8,), generator=gen).to(dev)) for _ in range(6)]
    lrs = [0.4, 0.8, 1.0, 0.7, 0.3, 0.05]   # two eager warm-up calls, the capture + replay, three more replays
    mean = torch.tensor((0.485, 0.456, 0.406), device=dev)
    std = torch.tensor((0.229, 0.224, 0.225), device=dev)

    def make(model):
        opt = build_optimizer("lars", model.parameters(), lrs[0], 0.9, 1e-4, lars_eta=0.02)
        lay = input_layout(model)

        def step(imgs, labels):
            x = Fn.to_device_nhwc(imgs, mean, std, nchw=True, in_scale=1 / 255.0, **lay)
            loss = Fn.cross_entropy(model(x), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()

        return opt, step

    def set_lr(opt, lr):
        for g in opt.param_groups:
            g["lr"] = lr
        opt.push_lr()

    m_eager, m_graph = base, copy.deepcopy(base)
    oe, eager = make(m_eager)
    for lr, b in zip(lrs, batches):
        set_lr(oe, lr)
        eager(*b)
    og, graphed = make(m_graph)
    grapher = StepGrapher(graphed, warmup=2, counters=HostCounters([m_graph], [og]))
    for lr, b in zip(lrs, batches):
        set_lr(og, lr)
        grapher(*b)
    torch.cuda.synchronize()
    assert grapher.captures == 1 and grapher.calls == 6
    for (n, p1), p2 in zip(m_eager.named_parameters(), m_graph.parameters()):
        assert torch.equal(p1, p2), n
        assert torch.equal(oe.state[p1]["momentum_buffer"], og.state[p2]["momentum_buffer"]), n
    # the learning rate took effect: the same steps at a constant rate end elsewhere
    m_const = copy.deepcopy(base)
    oc, const = make(m_const)
    for b in batches:
        const(*b)
    assert not torch.equal(m_const.fc.weight, m_eager.fc.weight)


def _rccl_lars_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DCP_COMM_STREAM="1")
    sys.path.insert(0, ROOT)
    import datetime

    from ddp_classification_pytorch_amd.engine.graph import GraphedStep
    from ddp_classification_pytorch_amd.models import build_model, input_layout
    from ddp_classification_pytorch_amd.ops import functional as Fn
    from ddp_classification_pytorch_amd.optim import build_optimizer
    from ddp_classification_pytorch_amd.parallel.ddp import attach_optimizer, graph_safe_nccl_env, wrap_ddp

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _no_autotune()
    graph_safe_nccl_env()
    dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=120))
    g = torch.Generator().manual_seed(1)
    imgs = torch.randint(0, 256, (8, 3, 32, 32), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, 10, (8,), generator=g).to(dev)
    out = {}
    for mode in ("plain", "eager", "graph"):
        torch.manual_seed(0)
        model = build_model("resnet18", num_classes=10).to(dev)
        opt = build_optimizer("lars", model.parameters(), 0.5, 0.9, 1e-4, lars_eta=0.02)
        net = model
        if mode != "plain":
            net = wrap_ddp(model, 0, syncbn=False, bucket_cap_mb=2, first_bucket_mb=0.5, force=True, engine="dcp")
            attach_optimizer(net, opt)
        x = Fn.to_device_nhwc(imgs, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), in_scale=1 / 255.0,
                              **input_layout(model))

        def step():
            loss = Fn.cross_entropy(net(x), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()

        if mode == "graph":
            gs = GraphedStep(step, warmup=2, distributed=True)
            gs()
        else:
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        out[mode] = {"params": {n: p.detach().cpu().clone() for n, p in model.named_parameters()},
                     "buckets": len(net.reducer.buckets) if mode != "plain" else 0}
    torch.save(out, os.path.join(out_dir, "lars.pt"))
    dist.destroy_process_group()


def test_rccl_world1_bucket_engine_lars_bit_equal_to_plain_step():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rccl_lars_worker, args=(1, _free_port(), d), nprocs=1, join=True)
        got = torch.load(os.path.join(d, "lars.pt"), weights_only=True)
    assert got["eager"]["buckets"] >= 3 and got["graph"]["buckets"] >= 3
    for n, v in got["plain"]["params"].items():
        assert torch.equal(got["eager"]["params"][n], v), n
        assert torch.equal(got["graph"]["params"][n], v), n


def _run_main(tmp_path, tag, extra, monkeypatch):
    """main.py in this process -> (train_iter records, StepGrapher instances, eager-call count)."""
    import main as entry
    from ddp_classification_pytorch_amd.engine import graph as G

    seen = {"graphers": [], "eager": 0}
    init, eager = G.StepGrapher.__init__, G.StepGrapher.eager

    def spy_init(self, *a, **k):
        init(self, *a, **k)
        seen["graphers"].append(self)

    def spy_eager(self, *t):
        seen["eager"] += 1
        return eager(self, *t)

    monkeypatch.setattr(G.StepGrapher, "__init__", spy_init)
    monkeypatch.setattr(G.StepGrapher, "eager", spy_eager)
    out = tmp_path / tag
    torch.manual_seed(0)
    entry.main(["--workload", "baseline", "--data", "synthetic", "--model", "resnet18", "--num-classes", "10",
                "--epochs", "1", "--max-steps-per-epoch", "8", "--warmup-iters", "4", "--graph",
                "--dataset", "CIFAR10", "--batchsize", "16", "--synthetic-train-size", "128",
                "--synthetic-val-size", "32", "--workers", "0", "--log-interval", "1", "--lr", "0.5",
                "--out-dir", str(out)] + extra)
    with open(out / "metrics.jsonl") as f:
        recs = [json.loads(line) for line in f]
    return [r for r in recs if r["kind"] == "train_iter"], seen["graphers"], seen["eager"]


def test_main_lars_poly_graph_end_to_end(tmp_path, monkeypatch):
    from ddp_classification_pytorch_amd.optim import LinearWarmup, PolyDecay

    it, graphers, eager_calls = _run_main(tmp_path, "lars", ["--optimizer", "lars", "--lr-decay", "poly"], monkeypatch)
    assert len(it) == 8 and all(r["loss"] == r["loss"] and abs(r["loss"]) < float("inf") for r in it)
    warm = LinearWarmup([], 4, 0.5, start_lr=1e-6)
    poly = PolyDecay([], total=8, target_lr=0.5, warm=4)
    want = [warm.lr_at(n) for n in (1, 2, 3, 4)] + [poly.lr_at(s) for s in (4, 5, 6, 7)]
    lrs = [r["lr"] for r in it]
    assert lrs == pytest.approx(want, rel=1e-12), (lrs, want)
    assert lrs[0] < lrs[1] < lrs[2] < lrs[3] == 0.5 == lrs[4] > lrs[5] > lrs[6] > lrs[7] > 0   # ramp, then decay
    # warm-up and decay went through the grapher: its own 2 eager calls, one capture, no recapture
    assert len(graphers) == 1 and graphers[0].captures == 1 and eager_calls == 0


def test_main_sgd_warmup_stays_eager(tmp_path, monkeypatch):
    it, graphers, eager_calls = _run_main(tmp_path, "sgd", ["--optimizer", "sgd"], monkeypatch)
    assert len(it) == 8 and all(abs(r["loss"]) < float("inf") for r in it)
    lrs = [r["lr"] for r in it]
    assert lrs[0] < lrs[1] < lrs[2] < lrs[3] == 0.5 and lrs[4:] == [0.5] * 4
    assert eager_calls == 4 and len(graphers) == 1 and graphers[0].captures == 1
