"""FusedLARS without a GPU: its CPU path against the fp64 oracle (tests/lars_ref.py) -- exact on the
integer lattice, within the derived tolerance on random inputs --, the sensitivity of that oracle to
the slips the GPU tests are meant to catch, build_optimizer's grouping, state_dict, PolyDecay, and the
bucket engine (world 1 and 2-rank gloo) stepping LARS per bucket.

Tolerance (derived in test_lars_kernels_gpu.py for the kernels' chain, which bounds the CPU path's
shorter one too): trust within 34 u, u = 2^-24; update and momentum within that plus SGD's 2e-6.
"""
import copy
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddp_classification_pytorch_amd.optim import FusedLARS, FusedSGD, PolyDecay, build_optimizer
from tests import lars_ref as L

U = 2.0 ** -24
TRUST_TOL = 34 * U
STEP_TOL = TRUST_TOL + 2e-6


def _relerr(got, ref):
    got, ref = L.f64(got).reshape(-1), L.f64(ref).reshape(-1)
    err = (got - ref).norm()
    return 0.0 if err == 0 else (err / ref.norm()).item()


def test_cpu_path_exact_on_lattice():
    """The lattice's precondition, independent of any GPU: every intermediate of the exact cases is
    an fp32 number, so the fp32 CPU path equals the fp64 oracle bit for bit."""
    L.check_exact_steps(FusedLARS, "cpu")


def test_cpu_path_exact_weight_decay_case():
    L.check_exact_wd(FusedLARS, "cpu")


RANDOM_SIZES = [1, 3, 4095, 4096, 4097, 8195]
RANDOM_GRID = [
    dict(lr=0.1, momentum=0.0, eta=0.25),
    dict(lr=0.3, momentum=0.9, dampening=0.1, weight_decay=5e-2, eta=0.25, eps=1e-2),
    dict(lr=0.2, momentum=0.9, nesterov=True, weight_decay=5e-2, grad_scale=0.5, eta=0.5, eps=1e-8),
]


def _random_inputs(seed, sizes=RANDOM_SIZES):
    gen = torch.Generator().manual_seed(seed)
    ps = [0.05 * torch.randn(n, generator=gen) for n in sizes]
    gs = [0.5 + torch.rand(n, generator=gen) if n < 8 else torch.randn(n, generator=gen) for n in sizes]
    return ps, gs


@pytest.mark.parametrize("kw", RANDOM_GRID, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_cpu_path_random_within_tolerance(kw):
    ps0, _ = _random_inputs(5)
    ps = [p.clone().requires_grad_(True) for p in ps0]
    opt = FusedLARS(ps, **kw)
    h = opt.param_groups[0]
    for step in (1, 2, 3):
        _, gs = _random_inputs(50 + step)
        before = [p.detach().clone() for p in ps]
        bufs = [opt.state[p].get("momentum_buffer") for p in ps]
        bufs = [None if b is None else b.clone() for b in bufs]
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        for i, (p, g) in enumerate(zip(ps, gs)):
            ref_p, ref_buf, ref_t = L.lars_step(before[i], g, bufs[i], step == 1, h["lr"], h["momentum"], h["dampening"],
                                                h["weight_decay"], h["nesterov"], h["grad_scale"], h["eta"], h["eps"])
            name = (step, RANDOM_SIZES[i])
            assert abs(float(opt.trust_of(p)) - ref_t) <= TRUST_TOL * ref_t, name
            ref_delta = ref_p - L.f64(before[i])
            assert (L.f64(before[i]).norm() / ref_delta.norm()).item() <= 64, name
            assert _relerr(L.f64(p) - L.f64(before[i]), ref_delta) <= STEP_TOL, name
            if h["momentum"]:
                assert _relerr(opt.state[p]["momentum_buffer"], ref_buf) <= STEP_TOL, name


def test_oracle_is_sensitive_to_trust_and_dropped_chunks():
    """The GPU tests are not vacuous: on their own inputs, an update with the trust ratio forced to 1
    or with a full chunk left out of either norm (what a wrong chunk span or a skipped partial does)
    is more than 100 tolerances away from the true update; on the lattice, losing just the tail
    chunk -- a single element for 4097 -- already changes the fp32 result."""
    kw = RANDOM_GRID[1]
    ps, gs = _random_inputs(5)
    args = (True, kw["lr"], kw["momentum"], kw["dampening"], kw["weight_decay"], False, 1.0, kw["eta"], kw["eps"])
    for n, p, g in zip(RANDOM_SIZES, ps, gs):
        true_p, _, _ = L.lars_step(p, g, None, *args)
        delta = true_p - L.f64(p)
        wrong, _, _ = L.lars_step(p, g, None, *args, trust=1.0)
        assert _relerr(wrong - L.f64(p), delta) > 100 * STEP_TOL, n
        if n > L.CHUNK:
            for drop in (dict(drop_w=0), dict(drop_g=0)):
                wrong, _, _ = L.lars_step(p, g, None, *args, **drop)
                assert _relerr(wrong - L.f64(p), delta) > 100 * STEP_TOL, (n, drop)
    gen = torch.Generator().manual_seed(9)
    for i, n in ((4, 4097), (5, 8195)):
        pv, gv = L.exact_draw(i, n, gen)
        hy = L.EXACT_HYPER
        ex = (True, hy["lr"], hy["momentum"], 0.0, 0.0, False, hy["grad_scale"], hy["eta"], hy["eps"])
        true_p, _, _ = L.lars_step(pv, gv, None, *ex)
        tail = (n - 1) // L.CHUNK
        for drop in (dict(drop_w=tail), dict(drop_g=tail), dict(drop_w=1), dict(drop_g=1)):
            wrong, _, _ = L.lars_step(pv, gv, None, *ex, **drop)
            assert not torch.equal(wrong.float(), true_p.float()), (n, drop)


def test_zero_norms_and_non_adaptive_group_cpu():
    """w == 0, g == 0 or both: trust exactly 1; a non-adaptive group steps as FusedSGD does."""
    gen = torch.Generator().manual_seed(3)
    w, g = torch.randn(100, generator=gen), torch.randn(100, generator=gen)
    z = torch.zeros(100)
    for pv, gv in ((z, g), (w, z), (z, z)):
        p = pv.clone().requires_grad_(True)
        q = pv.clone().requires_grad_(True)
        p.grad, q.grad = gv.clone(), gv.clone()
        ol = FusedLARS([p], lr=0.1, momentum=0.9, weight_decay=0.1, eta=0.25)
        os_ = FusedSGD([q], lr=0.1, momentum=0.9, weight_decay=0.1)
        ol.step()
        os_.step()
        assert float(ol.trust_of(p)) == 1.0
        assert torch.equal(p.detach(), q.detach())
    p, q = w.clone().requires_grad_(True), w.clone().requires_grad_(True)
    p.grad, q.grad = g.clone(), g.clone()
    ol = FusedLARS([dict(params=[p], adapt=False)], lr=0.1, momentum=0.9, weight_decay=0.1)
    os_ = FusedSGD([q], lr=0.1, momentum=0.9, weight_decay=0.1)
    for _ in range(2):
        ol.step()
        os_.step()
    assert torch.equal(p.detach(), q.detach())
    assert torch.equal(ol.state[p]["momentum_buffer"], os_.state[q]["momentum_buffer"])


def test_build_optimizer_lars_groups():
    from ddp_classification_pytorch_amd.models import build_model

    m = build_model("cifar_resnet18", num_classes=10)
    opt = build_optimizer("lars", m.parameters(), 0.5, 0.9, 1e-4, lars_eta=2e-3, lars_eps=1e-6)
    assert isinstance(opt, FusedLARS) and len(opt.param_groups) == 2
    ga, gn = opt.param_groups
    assert ga["adapt"] and ga["weight_decay"] == 1e-4 and all(p.ndim >= 2 for p in ga["params"])
    assert not gn["adapt"] and gn["weight_decay"] == 0.0 and all(p.ndim <= 1 for p in gn["params"])
    assert all(g["eta"] == 2e-3 and g["eps"] == 1e-6 and g["lr"] == 0.5 and g["momentum"] == 0.9 for g in (ga, gn))
    assert len(ga["params"]) + len(gn["params"]) == len(list(m.parameters())) and gn["params"]
    keep = build_optimizer("lars", m.parameters(), 0.5, 0.9, 1e-4, lars_keep_1d=True)
    assert len(keep.param_groups) == 1 and keep.param_groups[0]["adapt"]
    assert keep.param_groups[0]["weight_decay"] == 1e-4
    assert len(keep.param_groups[0]["params"]) == len(list(m.parameters()))
    d = FusedLARS([torch.zeros(3, requires_grad=True)]).defaults
    assert d["eta"] == 1e-3 and d["eps"] == 1e-8 and d["adapt"] is True


def test_config_flags():
    from ddp_classification_pytorch_amd.config import build_parser

    a = build_parser().parse_args(["--workload", "baseline", "--optimizer", "lars", "--lars-eta", "0.002", "--lars-eps",
                                   "1e-6", "--lars-keep-1d", "--lr-decay", "poly"])
    assert (a.optimizer, a.lars_eta, a.lars_eps, a.lars_keep_1d, a.lr_decay) == ("lars", 0.002, 1e-6, True, "poly")
    b = build_parser().parse_args(["--workload", "baseline"])
    assert (b.lars_eta, b.lars_eps, b.lars_keep_1d, b.lr_decay) == (1e-3, 1e-8, False, "none")


def test_state_dict_round_trip():
    def make():
        gen = torch.Generator().manual_seed(7)
        ps = [torch.randn(33, 5, generator=gen).requires_grad_(True), torch.randn(17, generator=gen).requires_grad_(True)]
        return ps, FusedLARS([dict(params=[ps[0]]), dict(params=[ps[1]], adapt=False, weight_decay=0.0)], lr=0.2,
                             momentum=0.9, weight_decay=1e-2, eta=0.1)

    def grads(ps, step):
        gen = torch.Generator().manual_seed(70 + step)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)

    ps, opt = make()
    for s in range(2):
        grads(ps, s)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())  # as through a checkpoint file: no storage shared with opt
    assert sd["param_groups"][0]["eta"] == 0.1 and sd["param_groups"][1]["adapt"] is False
    assert all(not torch.is_tensor(v) for g in sd["param_groups"] for v in g.values())
    qs, opt2 = make()
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    opt2.load_state_dict(sd)
    for o, xs in ((opt, ps), (opt2, qs)):
        grads(xs, 2)
        o.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(opt.state[p]["momentum_buffer"], opt2.state[q]["momentum_buffer"])


def test_poly_decay_lr_at():
    pd = PolyDecay([], total=100, target_lr=0.8, warm=20)
    assert pd.lr_at(0) == 0.8            # the ramp below the warm-up end belongs to LinearWarmup
    assert pd.lr_at(20) == 0.8           # warm-up end: the full rate
    assert pd.lr_at(60) == pytest.approx(0.8 * 0.25, rel=1e-15)   # midpoint: (1 - 1/2)^2
    assert pd.lr_at(99) == pytest.approx(0.8 * (1.0 / 80.0) ** 2, rel=1e-12)   # the last step
    assert pd.lr_at(100) == 0.0 and pd.lr_at(150) == 0.0
    assert PolyDecay([], total=10, target_lr=1.0).lr_at(5) == 0.25   # no warm-up
    p = torch.zeros(2, requires_grad=True)
    opt = FusedLARS([p], lr=0.8)
    assert PolyDecay(opt, total=100, target_lr=0.8, warm=20).set(60) == opt.param_groups[0]["lr"]


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
    return m, build_optimizer("lars", m.parameters(), 0.5, 0.9, 1e-4, lars_eta=0.02)


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


def test_single_process_engine_steps_lars_per_bucket_bit_equal():
    """Every parameter lies wholly inside one bucket, so the per-bucket step computes each tensor's
    norm from the same values as the full step(): bit-equal parameters."""
    from ddp_classification_pytorch_amd.parallel.reducer import GradSyncDDP

    m0, o0 = _make()
    ref = _train(m0, m0, o0, 0, 3, False)
    m1, o1 = _make()
    net = GradSyncDDP(m1, bucket_cap_mb=4, first_bucket_mb=0.5)
    got = _train(net, m1, o1, 0, 3, True)
    assert len(net.reducer.buckets) >= 3
    for k, v in ref.items():
        assert torch.equal(got[k], v), k
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


def test_two_rank_gloo_engine_steps_lars_per_bucket_bit_equal():
    """2 ranks, different data per rank: LARS fused per bucket == the engine's reduced gradients
    stepped by step() after backward, bit for bit, and the ranks agree bit for bit."""
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"r{k}.pt"), weights_only=True) for k in range(2)]
    assert r[0]["buckets"] >= 3
    for k, v in r[0][False].items():
        assert torch.equal(r[0][True][k], v), k
        assert torch.equal(r[1][True][k], r[0][True][k]), k
