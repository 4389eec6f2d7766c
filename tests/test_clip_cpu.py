"""Global gradient-norm clipping, the non-finite skip and the trust clamps on the CPU path.

* The oracle's (tests/clip_ref.py) preconditions.
* The CPU path of the four optimizers: the clipped step is the plain step with
  grad_scale' = fl32(grad_scale * coef), the norm and the coefficient are the oracle's, a skipped step
  writes nothing, LARS trust_clip and LAMB phi follow the oracle.
* Sensitivity: the checks fail on a coefficient applied twice, a norm that misses a tensor or the tail
  of a chunk, a missing +1e-6, and a skip that still writes momentum.
* The bucket engine: world 1 and 2-rank gloo with clipping on, updates issued from the end of backward.
"""
import copy
import math
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddp_classification_pytorch_amd.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, build_optimizer, optimizer_flags
from tests import clip_ref as C
from tests import lars_ref as L

SIZES = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5, 7, 11]
MAKERS = {
    "sgd": (FusedSGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-3, grad_scale=0.5), ("momentum_buffer",)),
    "adam": (FusedAdam, dict(lr=1e-2, weight_decay=1e-3, grad_scale=0.5), ("exp_avg", "exp_avg_sq")),
    "lars": (FusedLARS, dict(lr=0.1, momentum=0.9, weight_decay=1e-3, grad_scale=0.5, eta=0.02), ("momentum_buffer",)),
    "lamb": (FusedLAMB, dict(lr=1e-2, weight_decay=1e-2, grad_scale=0.5), ("exp_avg", "exp_avg_sq")),
}


def _params(seed, sizes=SIZES):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen).requires_grad_(True) for n in sizes]


def _grads(seed, scale, sizes=SIZES):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * scale for n in sizes]


def _groups(ps):
    """Two groups with different grad_scale: the norm weights each group with its own."""
    return [dict(params=ps[:5]), dict(params=ps[5:], grad_scale=2.0)]


def _scales(opt):
    return [g["grad_scale"] for g in opt.param_groups for _ in g["params"]]


# ----------------------------------------------------------------------------- the oracle
def test_oracle_preconditions():
    assert C.eps_is_absorbed(32.0) and C.eps_is_absorbed(64.0)
    assert not C.eps_is_absorbed(16.0)      # spacing 1.9e-6 at 16: 16 + 1e-6 rounds up
    assert C.clip_coef(32.0, 1.0) == 2.0 ** -5 and C.clip_coef(32.0, 64.0) == 1.0
    assert C.clip_coef(16.0, 1.0) != 2.0 ** -4
    assert math.isnan(float(C.clip_coef(float("nan"), 1.0)))      # a NaN norm gives a NaN coefficient
    assert C.clip_coef(float("inf"), 1.0) == 0.0
    assert C.clip_coef(5.0, 0.0) == 1.0                             # off
    assert C.skips(float("nan"), True) and C.skips(float("inf"), True) and not C.skips(3.0, True)
    assert not C.skips(float("nan"), False)
    assert C.eff_scale(0.5, 2.0 ** -5) == 2.0 ** -6
    gen = torch.Generator().manual_seed(0)
    gs = C.norm_lattice(SIZES, 5, -1, gen)                          # 4^6 entries of +-1/2: norm 32
    assert sum(int((g != 0).sum()) for g in gs) == 4 ** 6 and C.global_norm64(gs) == 32.0
    assert C.global_norm64(gs, drop=2) != 32.0 and C.global_norm64(gs, drop_tail_of=4) != 32.0
    assert C.lars_trust_clip(0.5, 0.25) == 1.0 and C.lars_trust_clip(0.125, 0.25) == 0.5
    assert C.lars_trust_clip(0.125, 0.0) == 1.0
    assert C.lamb_trust_phi(8.0, 2.0, 1.0, 4.0) == 2.0 and C.lamb_trust_phi(0.5, 2.0, 1.0, 4.0) == 0.5
    assert C.lamb_trust_phi(8.0, 2.0) == 4.0 and C.lamb_trust_phi(0.0, 2.0, 1.0, 4.0) == 1.0
    assert C.K_NORM == 13.5


# ----------------------------------------------------------------------------- twin equality on the CPU path
def _state_of(opt, ps, keys):
    return [[opt.state[p][k].clone() for k in keys if k in opt.state[p]] for p in ps]


@pytest.mark.parametrize("name", sorted(MAKERS))
@pytest.mark.parametrize("gscale,clipped", [(1.0, True), (1e-4, False)])
def test_clipped_step_is_the_plain_step_with_scaled_grad_scale(name, gscale, clipped):
    cls, kw, keys = MAKERS[name]
    ps = _params(1)
    opt = cls(_groups(ps), max_grad_norm=1.0, **kw)
    assert opt.needs_global_norm
    for step in (1, 2):
        grads = _grads(10 + step, gscale)
        twin_ps = [p.detach().clone().requires_grad_(True) for p in ps]
        sd = copy.deepcopy(opt.state_dict())
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        norm = C.global_norm(grads, _scales(opt))
        coef = C.clip_coef(norm, 1.0)
        assert (coef < 1) == clipped
        assert float(opt.grad_norm()) == float(norm) and float(opt.clip_coef()) == float(coef)
        assert int(opt.skipped_steps()) == 0
        twin = cls(_groups(twin_ps), **kw)
        twin.load_state_dict(sd)
        for g in twin.param_groups:
            g["grad_scale"] = C.eff_scale(g["grad_scale"], coef)
        for p, g in zip(twin_ps, grads):
            p.grad = g.clone()
        twin.step()
        for i, (p, q) in enumerate(zip(ps, twin_ps)):
            assert torch.equal(p, q), (step, i)
            for a, b in zip(_state_of(opt, [p], keys)[0], _state_of(twin, [q], keys)[0]):
                assert torch.equal(a, b), (step, i)
            if hasattr(opt, "trust_of"):
                assert torch.equal(torch.as_tensor(opt.trust_of(p)), torch.as_tensor(twin.trust_of(q))), (step, i)


@pytest.mark.parametrize("name", sorted(MAKERS))
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_skipped_step_writes_nothing_and_the_next_step_is_normal(name, bad):
    cls, kw, keys = MAKERS[name]
    ps = _params(2)
    opt = cls(_groups(ps), max_grad_norm=1.0, skip_nonfinite=True, **kw)
    for p, g in zip(ps, _grads(20, 1.0)):
        p.grad = g
    opt.step()
    before = [p.detach().clone() for p in ps], _state_of(opt, ps, keys)
    steps = [opt.state[p].get("step") for p in ps]
    grads = _grads(21, 1.0)
    grads[3][17] = bad
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()
    assert int(opt.skipped_steps()) == 1
    for i, p in enumerate(ps):
        assert torch.equal(p, before[0][i]), i
        for a, b in zip(_state_of(opt, [p], keys)[0], before[1][i]):
            assert torch.equal(a, b), i
    if steps[0] is not None:  # Adam / LAMB: the bias-correction count advances on a skipped step too
        assert [opt.state[p]["step"] for p in ps] == [s + 1 for s in steps]
    for p, g in zip(ps, _grads(22, 1.0)):
        p.grad = g
    opt.step()
    assert int(opt.skipped_steps()) == 1 and math.isfinite(float(opt.grad_norm()))
    assert all(not torch.equal(p, b) and bool(torch.isfinite(p).all()) for p, b in zip(ps, before[0]))
    # without skip_nonfinite the NaN shows in the coefficient, as clip_grad_norm_ gives
    ps2 = _params(2)
    opt2 = cls(_groups(ps2), max_grad_norm=1.0, **kw)
    for p, g in zip(ps2, grads):
        p.grad = g
    opt2.step()
    if math.isnan(bad):
        assert math.isnan(float(opt2.clip_coef()))
    else:
        assert float(opt2.clip_coef()) == 0.0
    assert opt2.skipped_steps() is not None and int(opt2.skipped_steps()) == 0


def test_skip_without_clipping_applies_coefficient_one_and_off_is_off():
    ps = _params(3)
    opt = FusedSGD(ps, lr=0.1, momentum=0.9, skip_nonfinite=True)
    ref_ps = _params(3)
    ref = FusedSGD(ref_ps, lr=0.1, momentum=0.9)
    assert opt.needs_global_norm and not ref.needs_global_norm and ref.grad_norm() is None
    for p, q, g in zip(ps, ref_ps, _grads(30, 5.0)):
        p.grad, q.grad = g, g.clone()
    opt.step()
    ref.step()
    assert float(opt.clip_coef()) == 1.0 and float(opt.grad_norm()) > 1.0
    assert all(torch.equal(p, q) for p, q in zip(ps, ref_ps))
    with pytest.raises(ValueError):
        FusedSGD(_params(3), max_grad_norm=-1.0)
    with pytest.raises(RuntimeError, match="norm_params"):
        opt.step_params(ps)


def test_parameter_without_gradient_takes_no_part():
    ps = _params(4)
    opt = FusedSGD(ps, lr=0.1, max_grad_norm=1.0)
    grads = _grads(40, 1.0)
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()
    assert float(opt.grad_norm()) == float(C.global_norm(grads))
    ps[5].grad = None
    opt.step()
    assert float(opt.grad_norm()) == float(C.global_norm(grads, drop=5))


def test_trust_clamps_follow_the_oracle_and_defaults_change_nothing():
    ps, ps_c, ps_d = _params(5), _params(5), _params(5)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-3, eta=0.02)
    plain, clip, dflt = FusedLARS(ps, **kw), FusedLARS(ps_c, trust_clip=True, **kw), FusedLARS(ps_d, trust_clip=False, **kw)
    grads = _grads(50, 1.0)
    grads[0] = grads[0] * 1e-3      # a large trust ratio: above lr
    for a, b, c, g in zip(ps, ps_c, ps_d, grads):
        a.grad, b.grad, c.grad = g, g.clone(), g.clone()
    plain.step(), clip.step(), dflt.step()
    hit = set()
    for a, b, c in zip(ps, ps_c, ps_d):
        want = C.lars_trust_clip(np.float32(float(plain.trust_of(a))), 0.05)
        assert float(clip.trust_of(b)) == float(want)
        hit.add(float(want) == 1.0)
        assert torch.equal(a, c)
    assert hit == {True, False}
    kw = dict(lr=1e-2, weight_decay=1e-2)
    ps, ps_c = _params(6), _params(6)
    plain, clamp = FusedLAMB(ps, **kw), FusedLAMB(ps_c, phi_min=2.0, phi_max=50.0, **kw)
    for a, b, g in zip(ps, ps_c, _grads(60, 1.0)):
        a.grad, b.grad = g, g.clone()
    before = [p.detach().clone() for p in ps]
    plain.step(), clamp.step()
    kinds = set()
    for a, b, w in zip(ps, ps_c, before):
        wn = np.float32(L.sumsq(w) ** 0.5)
        un = wn / np.float32(float(plain.trust_of(a)))
        got, want = float(clamp.trust_of(b)), float(C.lamb_trust_phi(wn, un, 2.0, 50.0))
        assert abs(got - want) <= 4 * C.U * want      # un is recovered through one more division
        kinds.add("lo" if wn < 2 else "hi" if wn > 50 else "in")
    assert kinds == {"lo", "hi", "in"}
    with pytest.raises(ValueError):
        FusedLAMB(_params(6), phi_min=3.0, phi_max=1.0)


def test_flags_reach_the_optimizers():
    from ddp_classification_pytorch_amd.config import build_parser

    a = build_parser().parse_args(["--clip-grad-norm", "1.5", "--skip-nonfinite", "--lars-trust-clip", "--lamb-phi-min",
                                 "0.5", "--lamb-phi-max", "8"])
    kw = optimizer_flags(a)
    for name in ("sgd", "adam", "lars", "lamb"):
        opt = build_optimizer(name, _params(7), 0.1, **kw)
        assert opt.max_grad_norm == 1.5 and opt.skip_nonfinite and opt.needs_global_norm, name
    assert build_optimizer("lars", _params(7), 0.1, **kw).trust_clip is True
    lamb = build_optimizer("lamb", _params(7), 0.1, **kw)
    assert (lamb.phi_min, lamb.phi_max) == (0.5, 8.0)
    off = optimizer_flags(build_parser().parse_args([]))
    opt = build_optimizer("sgd", _params(7), 0.1, **off)
    assert not opt.needs_global_norm and opt.max_grad_norm == 0.0


# ----------------------------------------------------------------------------- sensitivity
def _reference_step(ps, bufs, grads, max_norm, skip_nonfinite, lr, momentum, mutate=None):
    """Momentum SGD with clipping from the oracle's pieces -> (params, buffers, norm, coef);
    ``mutate``: one of the wrong implementations the checks must catch."""
    kw = {}
    if mutate == "misses-tensor":
        kw = dict(drop=len(grads) - 3)
    if mutate == "misses-chunk-tail":
        kw = dict(drop_tail_of=4)
    norm = C.global_norm(grads, **kw)
    coef = C.clip_coef(norm, max_norm, eps=0.0 if mutate == "no-eps" else C.EPS)
    skip = C.skips(norm, skip_nonfinite)
    gs = C.eff_scale(1.0, coef)
    if mutate == "coef-twice":
        gs = C.eff_scale(gs, coef)
    out_p, out_b = [], []
    for p, b, g in zip(ps, bufs, grads):
        d = g * gs
        nb = momentum * b + d
        if skip:
            out_p.append(p.clone())
            out_b.append(nb if mutate == "skip-writes-momentum" else b.clone())
        else:
            out_p.append(p - lr * nb)
            out_b.append(nb)
    return out_p, out_b, norm, coef


def _check_against_optimizer(mutate=None):
    """The checks: FusedSGD (CPU path) against the reference, bit for bit, on a clipped step with a small
    norm (where the 1e-6 shows) and on a NaN step with skipping."""
    lr, mom = 0.25, 0.5
    for scene, (scale, max_norm, poison) in enumerate([(1e-5, 2.0 ** -12, False), (1.0, 1.0, True)]):
        ps = _params(70 + scene)
        opt = FusedSGD(ps, lr=lr, momentum=mom, max_grad_norm=max_norm, skip_nonfinite=True)
        for p, g in zip(ps, _grads(80, scale)):   # the first step creates the buffers
            p.grad = g
        opt.step()
        p0 = [p.detach().clone() for p in ps]
        b0 = [opt.state[p]["momentum_buffer"].clone() for p in ps]
        grads = _grads(81, scale)
        if poison:
            grads[1][2] = float("nan")
        for p, g in zip(ps, grads):
            p.grad = g
        opt.step()
        ref_p, ref_b, norm, coef = _reference_step(p0, b0, grads, max_norm, True, lr, mom, mutate)
        if not poison:
            assert float(opt.grad_norm()) == float(norm), "norm"
            assert float(opt.clip_coef()) == float(coef), "coef"
            assert float(coef) < 1.0
        for p, b, rp, rb in zip(ps, [opt.state[p]["momentum_buffer"] for p in ps], ref_p, ref_b):
            assert torch.equal(p.detach(), rp), "param"
            assert torch.equal(b, rb), "buffer"


def test_checks_pass_on_the_right_step():
    _check_against_optimizer()


@pytest.mark.parametrize("mutate", ["coef-twice", "misses-tensor", "misses-chunk-tail", "no-eps", "skip-writes-momentum"])
def test_checks_fail_on_a_wrong_step(mutate):
    with pytest.raises(AssertionError):
        _check_against_optimizer(mutate)


# ----------------------------------------------------------------------------- the bucket engine
def _mlp():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(16, 48), torch.nn.Tanh(), torch.nn.Linear(48, 48), torch.nn.Tanh(),
                               torch.nn.Linear(48, 8))


def _opt(model, name="lars"):
    return build_optimizer(name, model.parameters(), 0.5, 0.9, 1e-4, lars_eta=0.02, max_grad_norm=0.05, skip_nonfinite=True)


def _batch(rank, step):
    gen = torch.Generator().manual_seed(100 * rank + step)
    return torch.randn(12, 16, generator=gen), torch.randint(0, 8, (12,), generator=gen)


def _loss(net, rank, step):
    x, y = _batch(rank, step)
    return torch.nn.functional.cross_entropy(net(x), y)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _averaged_reference(world, steps):
    """One process stepping on the gradients averaged over the ranks' batches (g / world summed in rank order,
    as the engine packs and all-reduces them)."""
    model = _mlp()
    opt = _opt(model)
    coefs = []
    for s in range(steps):
        acc = None
        for r in range(world):
            opt.zero_grad(set_to_none=True)
            _loss(model, r, s).backward()
            gs = [p.grad / world for p in model.parameters()]
            acc = gs if acc is None else [a + g for a, g in zip(acc, gs)]
        for p, g in zip(model.parameters(), acc):
            p.grad = g
        opt.step()
        coefs.append(float(opt.clip_coef()))
    return {n: p.detach().clone() for n, p in model.named_parameters()}, coefs


def test_single_process_engine_clips_from_finalize_bit_equal():
    from ddp_classification_pytorch_amd.parallel.reducer import GradSyncDDP

    ref, coefs = _averaged_reference(1, 3)
    assert all(c < 1.0 for c in coefs)
    model = _mlp()
    opt = _opt(model)
    net = GradSyncDDP(model, bucket_cap_mb=0.002, first_bucket_mb=0.001)
    net.attach_optimizer(opt)
    calls = []
    for name in ("norm_params", "step_after_norms", "step_params"):
        fn = getattr(opt, name)
        setattr(opt, name, lambda *a, _f=fn, _n=name: (calls.append(_n), _f(*a))[1])
    for s in range(3):
        opt.zero_grad(set_to_none=True)
        _loss(net, 0, s).backward()
        opt.step()
    nb = len(net.reducer.buckets)
    assert nb >= 3
    # per backward: one norm pass per bucket, then ONE update from the end of backward; never per bucket
    assert calls == (["norm_params"] * nb + ["step_after_norms"]) * 3
    for k, v in ref.items():
        assert torch.equal(dict(model.named_parameters())[k].detach(), v), k


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ddp_classification_pytorch_amd.parallel.reducer import GradSyncDDP

    model = _mlp()
    opt = _opt(model)
    net = GradSyncDDP(model, bucket_cap_mb=0.002, first_bucket_mb=0.001)
    net.attach_optimizer(opt)
    coefs = []
    for s in range(3):
        opt.zero_grad(set_to_none=True)
        _loss(net, rank, s).backward()
        opt.step()
        coefs.append(float(opt.clip_coef()))
    torch.save({"params": {n: p.detach().clone() for n, p in model.named_parameters()}, "coefs": coefs,
                "buckets": len(net.reducer.buckets)}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_engine_with_clipping_keeps_replicas_identical():
    """2 ranks, different data per rank, clipping on: the ranks agree bit for bit after three steps and
    equal one process stepping on the averaged gradients."""
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"r{k}.pt"), weights_only=True) for k in range(2)]
    ref, coefs = _averaged_reference(2, 3)
    assert r[0]["buckets"] >= 3 and all(c < 1.0 for c in coefs)
    assert r[0]["coefs"] == r[1]["coefs"] == coefs
    for k, v in ref.items():
        assert torch.equal(r[0]["params"][k], r[1]["params"][k]), k
        assert torch.equal(r[0]["params"][k], v), k
