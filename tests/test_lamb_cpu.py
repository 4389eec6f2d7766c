"""FusedLAMB without a GPU: its CPU path against the fp64 oracle (tests/lamb_ref.py) -- exact on the
lattice, within the derived bounds on random inputs --, the oracle's own preconditions and its
sensitivity to the slips the GPU tests are meant to catch, build_optimizer's grouping, the config
flags, state_dict, device_lr on the CPU, and the bucket engine (world 1 and 2-rank gloo) stepping LAMB
per bucket.

Bounds (derived in tests/lamb_ref.py for the kernels' chain): trust within K_TRUST u = 68 u, u =
2^-24; w, m, v per element within lamb_bounds, with one more rounding for each product that the CPU
path's torch ops do not fuse (``unfused=True``).
"""
import copy
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddp_classification_pytorch_amd.optim import FusedAdam, FusedLAMB, FusedSGD, build_optimizer
from tests import lamb_ref as R

TRUST_TOL = R.K_TRUST * R.U


def test_cpu_path_exact_on_lattice():
    """The lattice's precondition, independent of any GPU: lamb_step(exact=True) asserts that every
    intermediate is an fp32 number, so the fp32 CPU path equals the fp64 oracle bit for bit."""
    R.check_exact_steps(lambda ps: FusedLAMB(ps, **R.EXACT_HYPER), "cpu")


def test_oracle_refuses_inputs_off_the_lattice():
    gen = torch.Generator().manual_seed(2)
    w, g = R.exact_draw(40, 4097, gen)
    z = torch.zeros(4097)
    hy = R.EXACT_HYPER
    args = (1, hy["lr"], hy["betas"], hy["eps"], 0.0, 1.0, False)
    R.lamb_step(w, g, z, z, *args, exact=True)
    with pytest.raises(AssertionError, match="not exact"):
        R.lamb_step(w, g * 3, z, z, *args, exact=True)        # r = 3/5
    with pytest.raises(AssertionError, match="not exact"):
        R.lamb_step(w, g, z, z, 1, hy["lr"], (0.9, 0.75), hy["eps"], 0.0, 1.0, False, exact=True)
    g2 = g.clone()
    g2[int(g.nonzero()[0])] = 0.0                              # 4^a - 1 entries: |u| is no power of two
    with pytest.raises(AssertionError, match="not exact"):
        R.lamb_step(w, g2, z, z, *args, exact=True)


RANDOM_SIZES = [1, 3, 4095, 4096, 4097, 8195]
RANDOM_GRID = [
    dict(lr=0.05, weight_decay=0.0),
    dict(lr=0.05, weight_decay=16.0),          # wd |w| ~ 16 * 0.05 sqrt(n) against |r| ~ sqrt(n)
    dict(lr=0.1, weight_decay=16.0, grad_scale=0.5, eps=1e-3, betas=(0.8, 0.99)),
    dict(lr=0.05, weight_decay=8.0, bias_correction=False),
]


def _random_inputs(seed, sizes=RANDOM_SIZES):
    gen = torch.Generator().manual_seed(seed)
    ps = [0.05 * torch.randn(n, generator=gen) for n in sizes]
    gs = [0.5 + torch.rand(n, generator=gen) if n < 8 else torch.randn(n, generator=gen) for n in sizes]
    return ps, gs


@pytest.mark.parametrize("kw", RANDOM_GRID, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_cpu_path_random_within_bounds(kw):
    ps0, _ = _random_inputs(5)
    ps = [p.clone().requires_grad_(True) for p in ps0]
    opt = FusedLAMB(ps, **kw)
    worst = R.check_random_steps(opt, ps, RANDOM_SIZES, lambda step: _random_inputs(50 + step)[1], 3, unfused=True)
    print(f"lamb-cpu-errors {kw}: trust {worst['trust']:.2f} u (bound {R.K_TRUST} u), worst element "
          f"{worst['elem']:.3f} of its bound, kappa {worst['kappa']:.1f} (cap {R.KAPPA_CAP})")


def test_oracle_is_sensitive_to_the_slips_the_gpu_tests_catch():
    """On the random inputs: a chunk left out of either norm, |u| taken without wd * w, another
    tensor's trust ratio and a skipped bias correction each move the update by more than 100 trust
    tolerances.  On the lattice: losing the tail chunk -- one element for 4097 -- changes the fp32
    result."""
    kw = RANDOM_GRID[1]
    ps, gs = _random_inputs(5)
    trusts = []
    for n, p, g in zip(RANDOM_SIZES, ps, gs):
        z = torch.zeros(n)
        args = (p, g, z, z, 2, kw["lr"], (0.9, 0.999), 1e-6, kw["weight_decay"])
        true = R.lamb_step(*args)
        trusts.append(true["trust"])
        delta = true["p"] - R.f64(p)

        def moved(wrong):
            return float(((wrong["p"] - R.f64(p)) - delta).norm() / delta.norm())

        assert moved(R.lamb_step(*args, norm_without_wd=True)) > 100 * TRUST_TOL, n
        if n > 1:   # a single element moves by lr |w| sign(u) whatever scales r
            assert moved(R.lamb_step(*args, bias_correction=False)) > 100 * TRUST_TOL, n
        if n > R.CHUNK:
            for drop in (dict(drop_w=0), dict(drop_u=0)):
                assert moved(R.lamb_step(*args, **drop)) > 100 * TRUST_TOL, (n, drop)
    for i, (n, p, g) in enumerate(zip(RANDOM_SIZES, ps, gs)):
        z = torch.zeros(n)
        args = (p, g, z, z, 2, kw["lr"], (0.9, 0.999), 1e-6, kw["weight_decay"])
        true = R.lamb_step(*args)
        other = R.lamb_step(*args, trust=trusts[(i + 1) % len(trusts)])   # an entry-index slip
        assert float((other["p"] - true["p"]).norm() / (true["p"] - R.f64(p)).norm()) > 100 * TRUST_TOL, n
    gen = torch.Generator().manual_seed(9)
    hy = R.EXACT_HYPER
    for i, n in ((45, 4097), (46, 2 * R.CHUNK + 5)):
        w, g = R.exact_draw(i, n, gen)
        z = torch.zeros(n)
        ex = (w, g, z, z, 1, hy["lr"], hy["betas"], hy["eps"], 0.0, 1.0, False)
        true = R.lamb_step(*ex, exact=True)
        tail = (n - 1) // R.CHUNK
        for drop in (dict(drop_w=tail), dict(drop_u=tail), dict(drop_w=1), dict(drop_u=1)):
            assert not torch.equal(R.lamb_step(*ex, **drop)["p"].float(), true["p"].float()), (n, drop)


def test_zero_norms_and_non_adaptive_group_cpu():
    """w == 0, or g == 0 with zero moments and wd == 0: trust exactly 1, no NaN; adapt=False: trust 1
    and the oracle's update with that ratio."""
    gen = torch.Generator().manual_seed(3)
    w, g = torch.randn(100, generator=gen), torch.randn(100, generator=gen)
    z = torch.zeros(100)
    for pv, gv in ((z, g), (w, z), (z, z)):
        p = pv.clone().requires_grad_(True)
        p.grad = gv.clone()
        opt = FusedLAMB([p], lr=0.1)
        opt.step()
        assert float(opt.trust_of(p)) == 1.0
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(opt.state[p]["exp_avg_sq"]).all())
        ref = R.lamb_step(pv, gv, z, z, 1, 0.1)
        assert ref["trust"] == 1.0
        assert torch.allclose(p.detach().double(), ref["p"], rtol=1e-5, atol=1e-7)
    p = w.clone().requires_grad_(True)
    p.grad = g.clone()
    opt = FusedLAMB([dict(params=[p], adapt=False)], lr=0.1, weight_decay=0.5)
    opt.step()
    ref = R.lamb_step(w, g, z, z, 1, 0.1, wd=0.5, adapt=False)
    assert float(opt.trust_of(p)) == 1.0 == ref["trust"]
    assert R.lamb_step(w, g, z, z, 1, 0.1, wd=0.5)["trust"] != 1.0
    bnd = R.lamb_bounds(w, g, z, z, 1, 0.1, 1.0, wd=0.5, unfused=True)
    assert bool(((p.detach().double() - ref["p"]).abs() <= bnd["p"]).all())


def test_build_optimizer_lamb_groups():
    from ddp_classification_pytorch_amd.models import build_model

    m = build_model("cifar_resnet18", num_classes=10)
    opt = build_optimizer("lamb", m.parameters(), 0.5, 0.9, 1e-2, lamb_eps=1e-5, lamb_bias_correction=False)
    assert isinstance(opt, FusedLAMB) and isinstance(opt, FusedAdam) and len(opt.param_groups) == 2
    ga, gn = opt.param_groups
    assert ga["adapt"] and ga["weight_decay"] == 1e-2 and all(p.ndim >= 2 for p in ga["params"])
    assert not gn["adapt"] and gn["weight_decay"] == 0.0 and all(p.ndim <= 1 for p in gn["params"])
    assert all(g["eps"] == 1e-5 and g["bias_correction"] is False and g["lr"] == 0.5 for g in (ga, gn))
    assert len(ga["params"]) + len(gn["params"]) == len(list(m.parameters())) and gn["params"]
    keep = build_optimizer("lamb", m.parameters(), 0.5, 0.9, 1e-2, lamb_keep_1d=True)
    assert len(keep.param_groups) == 1 and keep.param_groups[0]["adapt"]
    assert keep.param_groups[0]["weight_decay"] == 1e-2
    d = FusedLAMB([torch.zeros(3, requires_grad=True)]).defaults
    assert d["betas"] == (0.9, 0.999) and d["eps"] == 1e-6 and d["bias_correction"] is True and d["adapt"] is True
    # the loop decides on the per-instance attribute, not on the method every fused optimizer has
    assert opt.device_lr is True and build_optimizer("lars", m.parameters(), 0.5).device_lr is True
    for name in ("sgd", "adam", "adamw"):
        assert hasattr(build_optimizer(name, m.parameters(), 0.5), "push_lr")
        assert build_optimizer(name, m.parameters(), 0.5).device_lr is False
        assert build_optimizer(name, m.parameters(), 0.5, device_lr=True).device_lr is True


def test_config_flags():
    from ddp_classification_pytorch_amd.config import build_parser
    from ddp_classification_pytorch_amd.optim import optimizer_flags

    a = build_parser().parse_args(["--workload", "arcface", "--optimizer", "lamb", "--lamb-eps", "1e-5",
                                   "--lamb-no-bias-correction", "--lamb-keep-1d", "--device-lr"])
    assert (a.optimizer, a.lamb_eps, a.lamb_bias_correction, a.lamb_keep_1d, a.device_lr) == ("lamb", 1e-5, False, True,
                                                                                             True)
    b = build_parser().parse_args(["--workload", "baseline"])
    assert (b.lamb_eps, b.lamb_bias_correction, b.lamb_keep_1d, b.device_lr) == (1e-6, True, False, False)
    f = optimizer_flags(a)
    assert (f["lamb_eps"], f["lamb_bias_correction"], f["lamb_keep_1d"], f["device_lr"]) == (1e-5, False, True, True)


def test_state_dict_round_trip():
    """Three steps, save, load into a fresh optimizer, two more: equal to five uninterrupted steps."""
    def make():
        gen = torch.Generator().manual_seed(7)
        ps = [torch.randn(33, 5, generator=gen).requires_grad_(True), torch.randn(17, generator=gen).requires_grad_(True)]
        return ps, FusedLAMB([dict(params=[ps[0]]), dict(params=[ps[1]], adapt=False, weight_decay=0.0)], lr=0.05,
                             weight_decay=0.5, eps=1e-5)

    def grads(ps, step):
        gen = torch.Generator().manual_seed(70 + step)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)

    ps, opt = make()
    for s in range(3):
        grads(ps, s)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())  # as through a checkpoint file: no storage shared with opt
    assert sd["param_groups"][0]["eps"] == 1e-5 and sd["param_groups"][1]["adapt"] is False
    assert all(not torch.is_tensor(v) for g in sd["param_groups"] for v in g.values())
    assert all(s["step"] == 3 for s in sd["state"].values())
    qs, opt2 = make()
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    opt2.load_state_dict(sd)
    for o, xs in ((opt, ps), (opt2, qs)):
        for s in (3, 4):
            grads(xs, s)
            o.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
        assert opt.state[p]["step"] == opt2.state[q]["step"] == 5
        assert torch.equal(opt.state[p]["exp_avg"], opt2.state[q]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], opt2.state[q]["exp_avg_sq"])


@pytest.mark.parametrize("cls,kw", [(FusedSGD, dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-2)),
                                    (FusedAdam, dict(lr=0.01, weight_decay=1e-2)),
                                    (FusedAdam, dict(lr=0.01, weight_decay=1e-2, decoupled=True))])
def test_device_lr_on_cpu_is_a_no_op(cls, kw):
    gen = torch.Generator().manual_seed(8)
    vals = [torch.randn(n, generator=gen) for n in (5, 130)]
    pa = [v.clone().requires_grad_(True) for v in vals]
    pb = [v.clone().requires_grad_(True) for v in vals]
    oa, ob = cls(pa, **kw), cls(pb, device_lr=True, **kw)
    assert oa.device_lr is False and ob.device_lr is True
    for step in range(3):
        for a, b in zip(pa, pb):
            a.grad = torch.randn(a.shape, generator=gen)
            b.grad = a.grad.clone()
        for o in (oa, ob):
            for g in o.param_groups:
                g["lr"] = kw["lr"] * (step + 1)
            o.push_lr()
            o.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))


# ----------------------------------------------------------------------------- the bucket engine
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(rank, step):
    g = torch.Generator().manual_seed(100 * step + rank)
    return torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)


def _make():
    from ddp_classification_pytorch_amd.models import build_model

    torch.manual_seed(0)
    m = build_model("cifar_resnet18", num_classes=10)
    return m, build_optimizer("lamb", m.parameters(), 0.02, weight_decay=1e-2)


def _train(net, model, opt, rank, steps, attach):
    from ddp_classification_pytorch_amd.ops import functional as Fn
    from ddp_classification_pytorch_amd.parallel.ddp import attach_optimizer

    if attach:
        attach_optimizer(net, opt)
    for s in range(steps):
        x, y = _data(rank, s)
        loss = Fn.cross_entropy(net(Fn.to_device_nhwc(x, cpad=8)), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def test_single_process_engine_steps_lamb_per_bucket_bit_equal():
    """Every parameter lies wholly inside one bucket, so the per-bucket step computes each tensor's
    norms from the same values as the full step(): bit-equal parameters."""
    from ddp_classification_pytorch_amd.parallel.reducer import GradSyncDDP

    m0, o0 = _make()
    ref = _train(m0, m0, o0, 0, 3, False)
    m1, o1 = _make()
    net = GradSyncDDP(m1, bucket_cap_mb=4, first_bucket_mb=0.5)
    got = _train(net, m1, o1, 0, 3, True)
    assert len(net.reducer.buckets) >= 3
    for k, v in ref.items():
        assert torch.equal(got[k], v), k
    assert all(o1.state[p]["step"] == 3 for p in m1.parameters())
    init = _make()[0].state_dict()
    assert any(not torch.equal(v, init[k]) for k, v in ref.items())


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ddp_classification_pytorch_amd.parallel.ddp import wrap_ddp

    out = {}
    for attach in (True, False):  # both arms in one process group: one spawn
        model, opt = _make()
        net = wrap_ddp(model, None, bucket_cap_mb=8, first_bucket_mb=1, engine="dcp")
        out[attach] = _train(net, model, opt, rank, 2, attach)
        out["buckets"] = len(net.reducer.buckets)
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_engine_steps_lamb_per_bucket_bit_equal():
    """2 ranks, different data per rank: LAMB fused per bucket == the engine's reduced gradients
    stepped by step() after backward, bit for bit, and the ranks agree bit for bit."""
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"r{k}.pt"), weights_only=True) for k in range(2)]
    assert r[0]["buckets"] >= 3
    for k, v in r[0][False].items():
        assert torch.equal(r[0][True][k], v), k
        assert torch.equal(r[1][True][k], r[0][True][k]), k
