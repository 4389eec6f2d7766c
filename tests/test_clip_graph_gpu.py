"""Gradient-norm clipping and the non-finite skip under HIP-graph replay, the bucket engine and main.py.

* One captured ``opt.step()`` of sgd / adam / lars / lamb over static gradient buffers: the replays are
  below the threshold, above it, poisoned with a NaN (skipped) and above it again, purely from the data;
  state bit-equal to an eager optimizer fed the same sequence.
* The control block must exist before a capture.
* A world-1 RCCL group through the bucket engine with clipping on: norm passes per bucket, the updates
  from the end of backward, parameters bit-equal to the same steps without DDP (eager and replayed).
* main.py --clip-grad-norm 1 --skip-nonfinite --device-lr --graph over two epochs: one capture, and the
  train_iter records carry grad_norm / clip_coef / skipped_steps.
"""
import json
import math
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
SIZES = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5, 17, 40 * 4096 + 1]
ARMS = {
    "sgd": ("sgd", dict(weight_decay=1e-3, device_lr=True), ("momentum_buffer",)),
    "adam": ("adam", dict(weight_decay=1e-3), ("exp_avg", "exp_avg_sq")),
    "lars": ("lars", dict(weight_decay=1e-3, lars_eta=0.02, lars_keep_1d=True), ("momentum_buffer",)),   # 1-D tensors adapt too
    "lamb": ("lamb", dict(weight_decay=1e-2, lamb_keep_1d=True), ("exp_avg", "exp_avg_sq")),
}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _no_autotune():
    from ddp_classification_pytorch_amd import _ext, tuning

    _ext.hip_ops().set_tuning(tuning.slot("autotune"), 0)


def _sequence():
    """Gradient sets: the eager warm-up, then replays 1-4 = below, above, a NaN, above (max_grad_norm 1)."""
    gen = torch.Generator().manual_seed(5)
    seq = []
    for scale in (1.0, 2.0 ** -14, 1.0, 1.0, 0.5):
        seq.append([torch.randn(n, generator=gen) * scale for n in SIZES])
    seq[3][5][4096] = float("nan")
    return seq, ("above", "below", "above", "skip", "above")


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_one_captured_step_clips_passes_and_skips_from_the_data(arm):
    from ddp_classification_pytorch_amd.engine.graph import GraphedStep, HostCounters
    from ddp_classification_pytorch_amd.optim import build_optimizer

    name, kw, keys = ARMS[arm]
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(4)
    init = [torch.randn(n, generator=gen) for n in SIZES]
    seq, kinds = _sequence()

    def make():
        ps = [v.to(dev).requires_grad_(True) for v in init]
        for p in ps:
            p.grad = torch.zeros_like(p)          # static gradient buffers
        opt = build_optimizer(name, ps, 0.05, 0.9, max_grad_norm=1.0, skip_nonfinite=True, **kw)
        return ps, opt

    def fill(ps, grads):
        for p, g in zip(ps, grads):
            p.grad.copy_(g)

    def snap(ps, opt):
        return ([p.detach().clone() for p in ps], [[opt.state[p][k].clone() for k in keys] for p in ps],
                [opt.state[p].get("step") for p in ps], float(opt.clip_coef()), int(opt.skipped_steps()))

    ps, opt = make()
    want = []
    for grads in seq:
        fill(ps, grads)
        opt.step()
        want.append(snap(ps, opt))
    for (_, _, _, coef, skipped), kind in zip(want, kinds):   # the sequence does what it says
        assert (coef == 1.0) == (kind == "below") and (coef < 1.0) == (kind == "above"), (kind, coef)
    assert [w[4] for w in want] == [0, 0, 0, 1, 1]
    for a, b in zip(want[2][0], want[3][0]):
        assert torch.equal(a, b)                               # the NaN step changed no parameter

    ps, opt = make()
    fill(ps, seq[0])
    step = GraphedStep(lambda: opt.step(), warmup=1, counters=HostCounters([], [opt]))
    for r in range(1, 5):
        fill(ps, seq[r])
        step()
        torch.cuda.synchronize()
        got = snap(ps, opt)
        for i, n in enumerate(SIZES):
            assert torch.equal(got[0][i], want[r][0][i]), (r, n)
            for k, a, b in zip(keys, got[1][i], want[r][1][i]):
                assert torch.equal(a, b), (r, n, k)
        assert got[2] == want[r][2], r
        assert got[3] == want[r][3] or (math.isnan(got[3]) and math.isnan(want[r][3])), r
        assert got[4] == want[r][4], r
    assert int(opt.skipped_steps()) == 1
    assert all(bool(torch.isfinite(p).all()) for p in ps)


def test_control_block_must_exist_before_capture(monkeypatch):
    from ddp_classification_pytorch_amd.optim import FusedSGD

    dev = torch.device("cuda", 0)
    p = torch.randn(10, device=dev).requires_grad_(True)
    p.grad = torch.randn(10, device=dev)
    opt = FusedSGD([p], lr=0.1, max_grad_norm=1.0)
    with monkeypatch.context() as m:      # what a capture reports, without opening one
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="eager step before capture"):
            opt._clip_state(dev)
    opt.step()
    assert float(opt.grad_norm()) > 0


def _rccl_clip_worker(rank, world, port, out_dir):
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
        opt = build_optimizer("lamb", model.parameters(), 0.02, weight_decay=1e-2, max_grad_norm=0.5,
                              skip_nonfinite=True)
        net = model
        calls = []
        if mode != "plain":
            net = wrap_ddp(model, 0, syncbn=False, bucket_cap_mb=2, first_bucket_mb=0.5, force=True, engine="dcp")
            attach_optimizer(net, opt)
            for name in ("norm_params", "step_after_norms", "step_params"):
                fn = getattr(opt, name)
                setattr(opt, name, lambda *a, _f=fn, _n=name: (calls.append(_n), _f(*a))[1])
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
                     "buckets": len(net.reducer.buckets) if mode != "plain" else 0, "calls": calls,
                     "coef": float(opt.clip_coef()), "norm": float(opt.grad_norm()),
                     "skipped": int(opt.skipped_steps())}
    torch.save(out, os.path.join(out_dir, "clip.pt"))
    dist.destroy_process_group()


def test_rccl_world1_bucket_engine_clips_from_finalize_bit_equal_to_plain_step():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rccl_clip_worker, args=(1, _free_port(), d), nprocs=1, join=True)
        got = torch.load(os.path.join(d, "clip.pt"), weights_only=True)
    nb = got["eager"]["buckets"]
    assert nb >= 3 and got["graph"]["buckets"] >= 3
    # the first backward launches its buckets together at its end; every backward: one norm pass per
    # bucket, then ONE update pass from _finalize; never a per-bucket update
    assert got["eager"]["calls"] == (["norm_params"] * nb + ["step_after_norms"]) * 3
    assert "step_params" not in got["graph"]["calls"] and got["graph"]["calls"].count("step_after_norms") == 3
    assert got["plain"]["steps"] == got["eager"]["steps"] == got["graph"]["steps"] == [3]
    assert 0.0 < got["plain"]["coef"] < 1.0 and got["plain"]["skipped"] == 0
    for mode in ("eager", "graph"):
        assert got[mode]["coef"] == got["plain"]["coef"] and got[mode]["norm"] == got["plain"]["norm"], mode
    for n, v in got["plain"]["params"].items():
        assert bool(torch.isfinite(v).all()), n
        assert torch.equal(got["eager"]["params"][n], v), n
        assert torch.equal(got["graph"]["params"][n], v), n


def test_main_clip_flags_graph_end_to_end(tmp_path, monkeypatch):
    import main as entry
    from ddp_classification_pytorch_amd.engine import graph as G

    graphers, eager_calls = [], [0]
    init, eager = G.StepGrapher.__init__, G.StepGrapher.eager

    def spy_init(self, *a, **k):
        init(self, *a, **k)
        graphers.append(self)

    def spy_eager(self, *t):
        eager_calls[0] += 1
        return eager(self, *t)

    with monkeypatch.context() as mpatch:
        mpatch.setattr(G.StepGrapher, "__init__", spy_init)
        mpatch.setattr(G.StepGrapher, "eager", spy_eager)
        out = tmp_path / "clip"
        torch.manual_seed(0)
        entry.main(["--workload", "baseline", "--data", "synthetic", "--model", "resnet18", "--num-classes", "10",
                    "--epochs", "2", "--max-steps-per-epoch", "8", "--warmup-iters", "4", "--graph",
                    "--dataset", "CIFAR10", "--batchsize", "16", "--synthetic-train-size", "128",
                    "--synthetic-val-size", "32", "--workers", "0", "--log-interval", "1", "--no-autotune",
                    "--lr", "0.05", "--out-dir", str(out),
                    "--clip-grad-norm", "1", "--skip-nonfinite", "--device-lr"])
    with open(out / "metrics.jsonl") as f:
        it = [r for r in map(json.loads, f) if r["kind"] == "train_iter"]
    assert len(it) == 16
    assert len(graphers) == 1 and graphers[0].captures == 1 and eager_calls[0] == 0
    for r in it:
        assert math.isfinite(r["loss"]) and math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0, r
        assert 0.0 < r["clip_coef"] <= 1.0, r
        assert r["skipped_steps"] == 0, r
