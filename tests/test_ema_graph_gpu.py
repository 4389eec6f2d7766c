"""The weight EMA inside a captured training step, under evaluation, the bucket engine and main.py.

* One captured step follows a decay warm-up (omd pushed before every call): one capture; parameters,
  momentum buffers, BN statistics, every average and the update count equal six eager steps.
* Logits under ema.applied() equal those of a fresh model loaded with the averaged state_dict; the live
  logits come back; a replay after the block still equals the eager twin.
* A world-1 RCCL group with the per-bucket optimizer on the communication stream, eagerly and replayed:
  the averages equal those of the unwrapped model stepped by step().
* main.py --model-ema --model-ema-warmup with --graph and with --no-graph ends on identical live
  parameters and averages, and logs val_ema every epoch.
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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


def _batches(n, dev):
    gen = torch.Generator().manual_seed(1)
    return [(torch.randint(0, 256, (8, 3, 32, 32), dtype=torch.uint8, generator=gen).to(dev),
             torch.randint(0, 10, (8,), generator=gen).to(dev)) for _ in range(n)]


def _make(model, dev, decay, warmup):
    from ddp_classification_pytorch_amd.models import input_layout
    from ddp_classification_pytorch_amd.ops import functional as Fn
    from ddp_classification_pytorch_amd.optim import WeightEMA, build_optimizer

    opt = build_optimizer("sgd", model.parameters(), 0.05, 0.9, weight_decay=1e-4)
    ema = WeightEMA(model, decay=decay, warmup=warmup, optimizer=opt)
    lay = input_layout(model)
    mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)

    def prep(imgs):
        return Fn.to_device_nhwc(imgs, mean, std, nchw=True, in_scale=1 / 255.0, **lay)

    def step(imgs, labels):
        loss = Fn.cross_entropy(model(prep(imgs)), labels)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        ema.update()
        return loss.detach()

    return opt, ema, step, prep


def _assert_same_run(m1, o1, e1, m2, o2, e2):
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert bool(torch.isfinite(p1).all()), n
        assert torch.equal(p1, p2), n
        assert torch.equal(o1.state[p1]["momentum_buffer"], o2.state[p2]["momentum_buffer"]), n
    s1, s2 = m1.state_dict(), m2.state_dict()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k     # BN running statistics and batch counts included
    assert e1.keys() == e2.keys() and len(e1.keys()) > 60
    for k in e1.keys():
        assert torch.equal(e1.average_of(k), e2.average_of(k)), k
    assert e1.num_updates == e2.num_updates


def test_step_grapher_follows_the_decay_warmup_with_one_capture():
    from ddp_classification_pytorch_amd.engine.graph import HostCounters, StepGrapher
    from ddp_classification_pytorch_amd.models import build_model

    _no_autotune()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = build_model("resnet18", num_classes=10).to(dev)
    batches = _batches(6, dev)
    m_eager, m_graph, m_const = base, copy.deepcopy(base), copy.deepcopy(base)
    oe, ee, eager, _ = _make(m_eager, dev, 0.99, True)
    for b in batches:
        ee.push_decay()
        eager(*b)
    og, eg, graphed, _ = _make(m_graph, dev, 0.99, True)
    grapher = StepGrapher(graphed, warmup=2, counters=HostCounters([m_graph], [og, eg]))
    for b in batches:
        eg.push_decay()
        grapher(*b)
    torch.cuda.synchronize()
    assert grapher.captures == 1 and grapher.calls == 6
    assert ee.num_updates == eg.num_updates == 6 and ee.pushes == eg.pushes == 6
    _assert_same_run(m_eager, oe, ee, m_graph, og, eg)
    # the pushed value took effect: the same steps at a constant decay end on other averages
    oc, ec, const, _ = _make(m_const, dev, 0.99, False)
    for b in batches:
        const(*b)
    assert torch.equal(m_const.fc.weight, m_eager.fc.weight)     # the live model does not care
    assert not torch.equal(ec.average_of("model.fc.weight"), ee.average_of("model.fc.weight"))
    moved = sum(1 for k in ee.keys() if not torch.equal(ee.average_of(k), m_eager.state_dict()[k[len("model."):]]))
    assert moved > 60                                            # averages, not copies of the weights


def test_evaluation_under_applied_and_replay_afterwards():
    from ddp_classification_pytorch_amd.engine.graph import HostCounters, StepGrapher
    from ddp_classification_pytorch_amd.models import build_model

    _no_autotune()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = build_model("resnet18", num_classes=10).to(dev)
    batches = _batches(5, dev)
    m_eager, m_graph = base, copy.deepcopy(base)
    oe, ee, eager, _ = _make(m_eager, dev, 0.9, False)
    og, eg, graphed, prep = _make(m_graph, dev, 0.9, False)
    grapher = StepGrapher(graphed, warmup=2, counters=HostCounters([m_graph], [og, eg]))
    for b in batches[:4]:
        eager(*b)
        grapher(*b)
    x = prep(batches[4][0])

    def logits(m):
        m.eval()
        with torch.no_grad():
            out = m(x).float().clone()
        m.train()
        return out

    live_before = logits(m_graph)
    ptrs = [p.data_ptr() for p in m_graph.parameters()]
    with eg.applied():
        averaged = logits(m_graph)
    live_after = logits(m_graph)
    fresh = build_model("resnet18", num_classes=10)
    fresh.load_state_dict(eg.model_state_dict("model"))
    want = logits(fresh.to(dev))
    assert torch.equal(averaged, want)
    assert not torch.equal(averaged, live_before)
    assert torch.equal(live_after, live_before)
    assert ptrs == [p.data_ptr() for p in m_graph.parameters()]
    # pointers and the bf16 weight cache survived the exchange: one more replay equals one more eager step
    eager(*batches[4])
    grapher(*batches[4])
    torch.cuda.synchronize()
    assert grapher.captures == 1
    _assert_same_run(m_eager, oe, ee, m_graph, og, eg)
    assert ee.num_updates == 5


def _rccl_ema_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DCP_COMM_STREAM="1")
    sys.path.insert(0, ROOT)
    import datetime

    from ddp_classification_pytorch_amd.engine.graph import GraphedStep, HostCounters
    from ddp_classification_pytorch_amd.models import build_model, input_layout
    from ddp_classification_pytorch_amd.ops import functional as Fn
    from ddp_classification_pytorch_amd.optim import WeightEMA, build_optimizer
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
        opt = build_optimizer("sgd", model.parameters(), 0.05, 0.9, weight_decay=1e-4)
        ema = WeightEMA(model, decay=0.9, optimizer=opt)
        net = model
        if mode != "plain":
            net = wrap_ddp(model, 0, syncbn=False, bucket_cap_mb=2, first_bucket_mb=0.5, force=True, engine="dcp")
            attach_optimizer(net, opt)
        x = Fn.to_device_nhwc(imgs, MEAN, STD, in_scale=1 / 255.0, **input_layout(model))

        def step():
            loss = Fn.cross_entropy(net(x), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            ema.update()
            return loss.detach()

        if mode == "graph":
            gs = GraphedStep(step, warmup=2, distributed=True, counters=HostCounters([model], [opt, ema]))
            gs()
            gs()
        else:
            for _ in range(4):
                step()
        torch.cuda.synchronize()
        out[mode] = {"avg": {k: ema.average_of(k).detach().cpu().clone() for k in ema.keys()},
                     "params": {n: p.detach().cpu().clone() for n, p in model.named_parameters()},
                     "n": ema.num_updates, "buckets": len(net.reducer.buckets) if mode != "plain" else 0}
    torch.save(out, os.path.join(out_dir, "ema.pt"))
    dist.destroy_process_group()


def test_rccl_world1_bucket_engine_averages_equal_the_plain_step():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rccl_ema_worker, args=(1, _free_port(), d), nprocs=1, join=True)
        got = torch.load(os.path.join(d, "ema.pt"), weights_only=True)
    assert got["eager"]["buckets"] >= 3 and got["graph"]["buckets"] >= 3
    assert got["plain"]["n"] == got["eager"]["n"] == got["graph"]["n"] == 4
    assert len(got["plain"]["avg"]) > 60
    for n, v in got["plain"]["params"].items():
        assert torch.equal(got["eager"]["params"][n], v) and torch.equal(got["graph"]["params"][n], v), n
    moved = 0
    for k, v in got["plain"]["avg"].items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(got["eager"]["avg"][k], v), k
        assert torch.equal(got["graph"]["avg"][k], v), k
        name = k[len("model."):]
        moved += int(name in got["plain"]["params"] and not torch.equal(v, got["plain"]["params"][name]))
    assert moved > 40


def _run_main(tmp_path, tag, extra):
    import main as entry

    out = tmp_path / tag
    torch.manual_seed(0)
    entry.main(["--workload", "baseline", "--data", "synthetic", "--model", "resnet18", "--dataset", "CIFAR10",
                "--epochs", "2", "--model-ema", "--model-ema-warmup", "--no-autotune", "--max-steps-per-epoch", "6",
                "--batchsize", "16", "--synthetic-train-size", "96", "--synthetic-val-size", "32", "--workers", "0",
                "--log-interval", "1", "--out-dir", str(out)] + extra)
    with open(out / "metrics.jsonl") as f:
        recs = [json.loads(line) for line in f]
    return recs, torch.load(out / "last.pth", map_location="cpu", weights_only=True)


def test_main_graph_and_eager_end_on_identical_weights_and_averages(tmp_path, monkeypatch):
    from ddp_classification_pytorch_amd.engine import graph as G

    graphers = []
    init = G.StepGrapher.__init__

    def spy_init(self, *a, **k):
        init(self, *a, **k)
        graphers.append(self)

    with monkeypatch.context() as mpatch:
        mpatch.setattr(G.StepGrapher, "__init__", spy_init)
        rg, cg = _run_main(tmp_path, "graph", ["--graph"])
        assert len(graphers) == 1 and graphers[0].captures >= 1
        re_, ce = _run_main(tmp_path, "eager", ["--no-graph"])
        assert len(graphers) == 1
    for recs in (rg, re_):
        ve = [r for r in recs if r["kind"] == "val_ema"]
        assert [r["epoch"] for r in ve] == [0, 1] and [r["updates"] for r in ve] == [6, 12]
        assert all(abs(r["loss"]) < float("inf") for r in ve)
    assert cg["ema"]["n"] == ce["ema"]["n"] == 12 and cg["ema"]["warmup"] is True
    n = 0
    for k, v in cg["models"]["model"].items():
        assert torch.equal(v, ce["models"]["model"][k]), k
        n += 1
    assert list(cg["ema"]["averages"]) == list(ce["ema"]["averages"])
    moved = 0
    for k, v in cg["ema"]["averages"].items():
        assert torch.equal(v, ce["ema"]["averages"][k]), k
        live = cg["models"]["model"][k[len("model."):]]
        moved += int(v.dtype == torch.float32 and not torch.equal(v, live))
    assert n > 20 and moved > 20
