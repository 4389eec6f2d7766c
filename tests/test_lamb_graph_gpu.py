"""FusedLAMB and the opt-in device learning rate of FusedSGD / FusedAdam under HIP-graph replay and the
bucket engine.

* One captured step follows a learning rate that changes before every replay (push_lr): no recapture,
  parameters and optimizer state bit-equal to eager steps -- for lamb, sgd + device_lr, adam + device_lr.
* A world-1 RCCL group: LAMB fused per bucket on the side communication stream, eagerly and replayed
  from a HIP graph, bit-equal to the unwrapped model stepped by step().
* main.py --optimizer lamb --lr-decay poly --graph end to end: warm-up and decay through one capture.
* main.py --optimizer sgd | adam --device-lr over two epochs: one capture, no eager call, and the same
  parameters as the run that recaptures.
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


# (build_optimizer name, its keyword arguments, the peak learning rate, the optimizer-state tensors)
ARMS = {
    "lamb": ("lamb", dict(weight_decay=1e-2), 0.02, ("exp_avg", "exp_avg_sq")),
    "sgd-device-lr": ("sgd", dict(weight_decay=1e-4, device_lr=True), 0.05, ("momentum_buffer",)),
    "adam-device-lr": ("adam", dict(device_lr=True), 0.002, ("exp_avg", "exp_avg_sq")),
}


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_step_grapher_follows_device_learning_rate_without_recapture(arm):
    from ddp_classification_pytorch_amd.engine.graph import HostCounters, StepGrapher
    from ddp_classification_pytorch_amd.models import build_model, input_layout
    from ddp_classification_pytorch_amd.ops import functional as Fn
    from ddp_classification_pytorch_amd.optim import build_optimizer

    name, okw, peak, state_keys = ARMS[arm]
    _no_autotune()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = build_model("resnet18", num_classes=10).to(dev)
    gen = torch.Generator().manual_seed(1)
    batches = [(torch.randint(0, 256, (8, 3, 32, 32), dtype=torch.uint8, generator=gen).to(dev),
                torch.randint(0, 10, (8,), generator=gen).to(dev)) for _ in range(6)]
    # two eager warm-up calls, the capture + replay, three more replays
    lrs = [peak * f for f in (0.4, 0.8, 1.0, 0.7, 0.3, 0.05)]
    mean = torch.tensor((0.485, 0.456, 0.406), device=dev)
    std = torch.tensor((0.229, 0.224, 0.225), device=dev)

    def make(model):
        opt = build_optimizer(name, model.parameters(), lrs[0], 0.9, **okw)
        assert opt.device_lr is True
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
        assert bool(torch.isfinite(p1).all()), n
        assert torch.equal(p1, p2), n
        for k in state_keys:
            assert torch.equal(oe.state[p1][k], og.state[p2][k]), (n, k)
        if "step" in oe.state[p1]:
            assert oe.state[p1]["step"] == og.state[p2]["step"] == 6, n
    # the learning rate took effect: the same steps at a constant rate end elsewhere
    m_const = copy.deepcopy(base)
    oc, const = make(m_const)
    for b in batches:
        const(*b)
    assert not torch.equal(m_const.fc.weight, m_eager.fc.weight)


def _rccl_lamb_worker(rank, world, port, out_dir):
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
        opt = build_optimizer("lamb", model.parameters(), 0.02, weight_decay=1e-2)
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
                     "steps": sorted({opt.state[p]["step"] for p in model.parameters()}),
                     "buckets": len(net.reducer.buckets) if mode != "plain" else 0}
    torch.save(out, os.path.join(out_dir, "lamb.pt"))
    dist.destroy_process_group()


def test_rccl_world1_bucket_engine_lamb_bit_equal_to_plain_step():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rccl_lamb_worker, args=(1, _free_port(), d), nprocs=1, join=True)
        got = torch.load(os.path.join(d, "lamb.pt"), weights_only=True)
    assert got["eager"]["buckets"] >= 3 and got["graph"]["buckets"] >= 3
    assert got["plain"]["steps"] == got["eager"]["steps"] == got["graph"]["steps"] == [3]
    for n, v in got["plain"]["params"].items():
        assert bool(torch.isfinite(v).all()), n
        assert torch.equal(got["eager"]["params"][n], v), n
        assert torch.equal(got["graph"]["params"][n], v), n


def _run_main(tmp_path, tag, extra, monkeypatch, epochs=1):
    """main.py in this process -> (train_iter records, StepGrapher instances, eager-call count, out dir)."""
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

    with monkeypatch.context() as mpatch:
        mpatch.setattr(G.StepGrapher, "__init__", spy_init)
        mpatch.setattr(G.StepGrapher, "eager", spy_eager)
        out = tmp_path / tag
        torch.manual_seed(0)
        entry.main(["--workload", "baseline", "--data", "synthetic", "--model", "resnet18", "--num-classes", "10",
                    "--epochs", str(epochs), "--max-steps-per-epoch", "8", "--warmup-iters", "4", "--graph",
                    "--dataset", "CIFAR10", "--batchsize", "16", "--synthetic-train-size", "128",
                    "--synthetic-val-size", "32", "--workers", "0", "--log-interval", "1",
                    "--out-dir", str(out)] + extra)
    with open(out / "metrics.jsonl") as f:
        recs = [json.loads(line) for line in f]
    return [r for r in recs if r["kind"] == "train_iter"], seen["graphers"], seen["eager"], out


def test_main_lamb_poly_graph_end_to_end(tmp_path, monkeypatch):
    from ddp_classification_pytorch_amd.optim import LinearWarmup, PolyDecay

    it, graphers, eager_calls, _ = _run_main(tmp_path, "lamb", ["--optimizer", "lamb", "--lr-decay", "poly", "--lr",
                                                               "0.02", "--weight-decay", "0.01"], monkeypatch)
    assert len(it) == 8 and all(r["loss"] == r["loss"] and abs(r["loss"]) < float("inf") for r in it)
    warm = LinearWarmup([], 4, 0.02, start_lr=1e-6)
    poly = PolyDecay([], total=8, target_lr=0.02, warm=4)
    want = [warm.lr_at(n) for n in (1, 2, 3, 4)] + [poly.lr_at(s) for s in (4, 5, 6, 7)]
    lrs = [r["lr"] for r in it]
    assert lrs == pytest.approx(want, rel=1e-12), (lrs, want)
    # warm-up and decay went through the grapher: its own 2 eager calls, one capture, no recapture
    assert len(graphers) == 1 and graphers[0].captures == 1 and eager_calls == 0


@pytest.mark.parametrize("name,lr", [("sgd", "0.05"), ("adam", "0.002")])
def test_main_device_lr_keeps_one_capture_over_two_epochs(tmp_path, monkeypatch, name, lr):
    """--device-lr: warm-up, the epoch boundary and the scheduler's step all replay one capture, and the
    run ends on the parameters of the run without it (which warms up eagerly and recaptures)."""
    args = ["--optimizer", name, "--no-autotune", "--lr", lr]
    it, graphers, eager_calls, out = _run_main(tmp_path, name + "-dev", args + ["--device-lr"], monkeypatch, epochs=2)
    assert len(it) == 16 and all(abs(r["loss"]) < float("inf") for r in it)
    assert len(graphers) == 1 and graphers[0].captures == 1 and eager_calls == 0
    it0, graphers0, eager0, out0 = _run_main(tmp_path, name + "-host", args, monkeypatch, epochs=2)
    assert eager0 == 4 and len(graphers0) == 1 and graphers0[0].captures == 2
    assert [r["lr"] for r in it] == [r["lr"] for r in it0]
    a = torch.load(out / "last.pth", map_location="cpu", weights_only=True)["models"]
    b = torch.load(out0 / "last.pth", map_location="cpu", weights_only=True)["models"]
    n = 0
    for k, sd in a.items():
        for key, v in sd.items():
            assert torch.equal(v, b[k][key]), (k, key)
            n += 1
    assert n > 20
