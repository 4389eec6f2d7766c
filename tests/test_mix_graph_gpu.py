"""Mixup / CutMix through the training step: one captured HIP graph serves mixed and unmixed steps
(the plan is ordinary batch data), main.py end to end, and the shard loader with a sampler.

* StepGrapher on the CIFAR ResNet-18 at 32 x 32, batch 16, fixed kernel configurations, fed by a
  SyntheticLoader carrying a sampler: 2 eager warm-ups, one capture, replays over a Mixup, a CutMix,
  an identity and a Mixup step; the parameters are torch.equal to a twin that ran the same batches
  eagerly.
* main.py --graph --mixup-alpha 0.2 --cutmix-alpha 1.0 over 8 steps: one capture, finite losses,
  train_iter records; two runs without mix flags and one with --mix-prob 0 (the identity plan
  through the mixed kernels) end on the same parameters bit for bit.
* ShardLoader with a sampler on a tiny packed shard: four tensors per batch, and the mixed batch is
  the oracle (tests/mix_ref.py, mix_layout) applied to what ``tap`` saw, normalised by the unmixed
  kernel: |got - v| <= 2^-8 |v| + 2^-20, one bf16 rounding (unit roundoff 2^-8) of an fp32 blend whose
  own error on |v| <= 2.7 is below 2^-20; rows that do not blend are torch.equal.
"""
import copy
import json

import numpy as np
import pytest
import torch

from ddp_classification_pytorch_amd.data.mix import MixSampler
from tests import mix_ref as M

pytestmark = pytest.mark.gpu


def _no_autotune():
    from ddp_classification_pytorch_amd import _ext, tuning

    _ext.hip_ops().set_tuning(tuning.slot("autotune"), 0)


def _kind(plan):
    if (plan.box != 0).any():
        return "cutmix"
    return "mixup" if (plan.blend != 1).any() else "identity"


def _sampler_with(kinds, n, size):
    """A sampler (found by its seed: the draws are a pure function of it) whose steps 0.. have ``kinds``."""
    for seed in range(20000):
        s = MixSampler(0.8, 1.0, prob=0.7, seed=seed)
        if all(k is None or _kind(s.draw(n, size, size, i)) == k for i, k in enumerate(kinds)):
            return s
    raise AssertionError("no seed draws " + str(kinds))


def test_step_grapher_one_capture_serves_mixed_and_unmixed_steps():
    from ddp_classification_pytorch_amd.data import SyntheticLoader
    from ddp_classification_pytorch_amd.engine.graph import HostCounters, StepGrapher
    from ddp_classification_pytorch_amd.models import build_model, input_layout
    from ddp_classification_pytorch_amd.ops import functional as Fn
    from ddp_classification_pytorch_amd.optim import build_optimizer

    _no_autotune()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = build_model("cifar_resnet18", num_classes=10).to(dev)
    lay = input_layout(base)
    # steps 0, 1: the grapher's eager warm-up; step 2: capture + first replay; 3..5 replays
    sampler = _sampler_with([None, None, "mixup", "cutmix", "identity", "mixup"], 16, 32)

    def loader(mix):
        return SyntheticLoader(16, 6, size=32, num_classes=10, device=dev, seed=3, mix=mix, **lay)

    def make(model):
        opt = build_optimizer("sgd", model.parameters(), 0.05, 0.9, weight_decay=1e-4)

        def step(x, labels, partner=None, wlab=None):
            mix = None if partner is None else (partner, wlab)
            loss, _ = Fn.cross_entropy(model(x), labels, 10, return_rank=True, mix=mix)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()

        return opt, step

    m_eager, m_graph, m_plain = base, copy.deepcopy(base), copy.deepcopy(base)
    _, eager = make(m_eager)
    losses = []
    for batch in loader(sampler):
        assert len(batch) == 4 and batch[2].dtype == torch.int32 and batch[3].dtype == torch.float32
        losses.append(eager(*batch))
    og, graphed = make(m_graph)
    grapher = StepGrapher(graphed, warmup=2, counters=HostCounters([m_graph], [og]))
    for batch in loader(sampler):
        grapher(*batch)
    _, plain = make(m_plain)
    for batch in loader(None):
        plain(*batch)
    torch.cuda.synchronize()
    assert grapher.captures == 1 and grapher.calls == 6
    assert all(bool(torch.isfinite(v)) for v in losses)
    for (n, p1), p2 in zip(m_eager.named_parameters(), m_graph.parameters()):
        assert bool(torch.isfinite(p1).all()), n
        assert torch.equal(p1, p2), n
    # the mixing took effect: the unmixed batches end elsewhere
    assert not torch.equal(m_plain.fc.weight, m_eager.fc.weight)


def _run_main(tmp_path, tag, extra, monkeypatch):
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
                    "--epochs", "1", "--max-steps-per-epoch", "8", "--graph", "--no-autotune",
                    "--dataset", "CIFAR10", "--batchsize", "16", "--synthetic-train-size", "128",
                    "--synthetic-val-size", "32", "--workers", "0", "--log-interval", "1",
                    "--out-dir", str(out)] + extra)
    with open(out / "metrics.jsonl") as f:
        recs = [json.loads(line) for line in f]
    return [r for r in recs if r["kind"] == "train_iter"], seen["graphers"], seen["eager"], out


def _params(out):
    sd = torch.load(out / "last.pth", map_location="cpu", weights_only=True)["models"]
    return {(k, key): v for k, m in sd.items() for key, v in m.items()}


def test_main_graph_mixup_cutmix_end_to_end(tmp_path, monkeypatch):
    it, graphers, eager_calls, out = _run_main(tmp_path, "mix", ["--mixup-alpha", "0.2", "--cutmix-alpha", "1.0"],
                                               monkeypatch)
    assert len(it) == 8 and all(np.isfinite(r["loss"]) for r in it)
    assert len(graphers) == 1 and graphers[0].captures == 1 and eager_calls == 0
    mixed = _params(out)
    # without the flags: the same parameters run to run, and the identity plan through the mixed
    # kernels (--mix-prob 0) is a no-op, bit for bit
    _, g0, _, out0 = _run_main(tmp_path, "plain0", [], monkeypatch)
    _, _, _, out1 = _run_main(tmp_path, "plain1", [], monkeypatch)
    it2, g2, _, out2 = _run_main(tmp_path, "prob0", ["--mixup-alpha", "0.2", "--cutmix-alpha", "1.0", "--mix-prob", "0"],
                                 monkeypatch)
    assert g0[0].captures == 1 and g2[0].captures == 1 and len(it2) == 8
    a, b, c = _params(out0), _params(out1), _params(out2)
    assert len(a) > 20 and a.keys() == b.keys() == c.keys()
    for k, v in a.items():
        assert torch.equal(v, b[k]), k
        assert torch.equal(v, c[k]), k
    assert any(not torch.equal(v, mixed[k]) for k, v in a.items())  # and the mixed run trained on other batches


def test_shard_loader_mixes_what_tap_saw(tmp_path):
    from ddp_classification_pytorch_amd.data import ShardSampler
    from ddp_classification_pytorch_amd.data.shards import ShardLoader, aug_preset, write_shard
    from ddp_classification_pytorch_amd.ops import functional as Fn

    rng = np.random.default_rng(1)
    imgs = [(rng.integers(0, 256, (int(rng.integers(40, 80)), int(rng.integers(40, 80)), 3), dtype=np.uint8), i % 7)
            for i in range(45)]
    p = str(tmp_path / "g.dcps")
    write_shard(p, imgs)
    aug, _ = aug_preset("nested", train=True, size=32)
    mix = MixSampler(0.8, 1.0, mode="elem", seed=6, rank=0)
    sampler = ShardSampler(list(range(45)), num_replicas=1, rank=0, shuffle=True, seed=2)
    ld = ShardLoader(p, batch_size=16, sampler=sampler, aug=aug, out_size=32, device="cuda", threads=4, prefetch=2,
                     s2d=True, mix=mix)
    tapped = []
    ld.tap = lambda u8, meta, extra: tapped.append(u8.cpu().clone())
    ld.set_epoch(1)
    batches = [tuple(t.cpu() for t in b) for b in ld]
    ld.close()
    assert len(batches) == len(tapped) == 3
    worst, kinds = 0.0, set()
    for step, (b, u8) in enumerate(zip(batches, tapped)):
        assert len(b) == 4
        x, labels, partner, wlab = b
        n = u8.shape[0]
        assert u8.shape == (n, 32, 32, 3) and u8.dtype == torch.uint8 and x.shape == (n, 16, 16, 16)
        plan = mix.draw(n, 32, 32, step, epoch=1)
        assert np.array_equal(partner.numpy(), plan.partner) and np.array_equal(wlab.numpy(), plan.wlab)
        assert labels.shape == (n,) and labels.dtype == torch.int64
        A = Fn.to_device_nhwc(u8.cuda(), ld.mean, ld.std, cpad=8, nchw=False, in_scale=1.0 / 255.0, s2d=True).cpu()
        want = M.mix_layout(A, plan, 32, 32, "s2d2")
        err = (x.double() - want).abs()
        worst = max(worst, (err / (2.0 ** -8 * want.abs() + 2.0 ** -20)).max().item())
        same = torch.from_numpy(plan.blend == 1)
        assert torch.equal(x[same], want.to(torch.bfloat16)[same])
        kinds |= {"cutmix"} if (plan.box != 0).any() else set()
        kinds |= {"mixup"} if (plan.blend != 1).any() else set()
    print(f"shard loader mixed batch: worst err / bound {worst:.4f}")
    assert worst <= 1.0 and kinds == {"cutmix", "mixup"}
