"""The LAMB kernels of csrc/optim.hip (mt_lamb_moments, lamb_trust, mt_lamb_update) through FusedLAMB,
against the fp64 oracle of tests/lamb_ref.py, and the device learning rate of FusedSGD / FusedAdam.

* Exact: on the lattice of lamb_ref every intermediate is an fp32 number (test_lamb_cpu.py shows that
  without a GPU), so w, m, v and the trust ratios must equal the oracle bit for bit -- over tails,
  chunk boundaries, a tensor of 301 chunks and 70 small tensors whose trust ratios are all different
  powers of two.
* Alignment: the same values through views at float offsets 0..3 give the same bits.
* Zero norms give trust exactly 1 and no NaN; a non-adaptive group takes one launch with trust 1.
* Random inputs, bias correction on, wd |w| comparable to |r|: the trust ratio within K_TRUST u = 68 u
  of fp64 and, teacher-forced, every element of w, m and v within lamb_bounds -- both derived in
  lamb_ref from the kernels' chain of fp32 operations.
* FusedSGD(device_lr=True) and FusedAdam(device_lr=True) step bit-equal to the host-rate kernels.
"""
import pytest
import torch

from ddp_classification_pytorch_amd.optim import FusedAdam, FusedLAMB, FusedSGD
from tests import lamb_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [1, 3, 4095, 4096, 4097, 8195]
LATE = 2


# ----------------------------------------------------------------------------- exact
def test_exact_on_lattice_three_steps():
    R.check_exact_steps(lambda ps: FusedLAMB(ps, **R.EXACT_HYPER), DEV, sync=torch.cuda.synchronize)


# ----------------------------------------------------------------------------- alignment
def _at_offset(values, off):
    """``values`` as a view ``off`` floats into a fresh 16-byte aligned buffer."""
    holder = torch.zeros(values.numel() + 4, device=DEV)
    assert holder.data_ptr() % 16 == 0
    v = holder[off:off + values.numel()]
    v.copy_(values)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _aligned_run(which, off, carried, kw):
    """Two steps over SIZES with the parameters, gradients or moments (``which``) at float offset
    ``off``; ``carried``: moments preset (step counts 3 and 4), else from zero (1 and 2)."""
    gen = torch.Generator().manual_seed(77)
    vals = [0.05 * torch.randn(n, generator=gen) for n in SIZES]
    ms = [0.3 * torch.randn(n, generator=gen) for n in SIZES]
    vs = [0.1 * torch.rand(n, generator=gen) for n in SIZES]
    ps = [_at_offset(v, off if which == "p" else 0).requires_grad_(True) for v in vals]
    opt = FusedLAMB(ps, **kw)
    for p, m, v in zip(ps, ms, vs):
        z = torch.zeros_like(m)
        opt.state[p] = dict(step=2 if carried else 0, exp_avg=_at_offset(m if carried else z, off if which == "m" else 0),
                            exp_avg_sq=_at_offset(v if carried else z, off if which == "v" else 0))
    trusts = []
    for step in (1, 2):
        for p, n in zip(ps, SIZES):
            p.grad = _at_offset(torch.randn(n, generator=gen), off if which == "g" else 0)
        opt.step()
        trusts.append(torch.stack([opt.trust_of(p) for p in ps]).clone())
    torch.cuda.synchronize()
    assert all(opt.state[p]["step"] == (4 if carried else 2) for p in ps)
    return ([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps],
            [opt.state[p]["exp_avg_sq"].clone() for p in ps], trusts)


@pytest.mark.parametrize("adapt", [True, False], ids=["adaptive", "one-launch"])
@pytest.mark.parametrize("carried", [True, False], ids=["carried", "zero-moments"])
def test_alignment_offsets_give_identical_bits(carried, adapt):
    kw = dict(lr=0.05, weight_decay=8.0, eps=1e-4, grad_scale=0.5, adapt=adapt)
    base = _aligned_run("p", 0, carried, kw)
    for which in ("p", "g", "m", "v"):
        for off in (1, 2, 3):
            got = _aligned_run(which, off, carried, kw)
            for i, n in enumerate(SIZES):
                name = (which, off, n)
                assert torch.equal(got[3][0][i], base[3][0][i]) and torch.equal(got[3][1][i], base[3][1][i]), name
                for k in range(3):
                    assert torch.equal(got[k][i], base[k][i]), (name, k)
    assert all((float(t) != 1.0) == adapt for t in base[3][0])


# ----------------------------------------------------------------------------- zero norms, adapt=False
def test_zero_norms_give_trust_one_and_no_nan():
    gen = torch.Generator().manual_seed(3)
    for n in (3, 4097):
        w, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        z = torch.zeros(n)
        for pv, gv in ((z, g), (w, z), (z, z)):
            p = pv.to(DEV).requires_grad_(True)
            p.grad = gv.to(DEV)
            opt = FusedLAMB([p], lr=0.1)
            opt.step()
            torch.cuda.synchronize()
            assert float(opt.trust_of(p)) == 1.0
            st = opt.state[p]
            assert all(bool(torch.isfinite(t).all()) for t in (p, st["exp_avg"], st["exp_avg_sq"]))
            forced = R.lamb_step(pv, gv, z, z, 1, 0.1, trust=1.0)
            bnd = R.lamb_bounds(pv, gv, z, z, 1, 0.1, 1.0)
            assert bool(((R.f64(p) - forced["p"]).abs() <= bnd["p"]).all())
            if not gv.any():
                assert torch.equal(p.detach().cpu(), pv)   # u == 0: nothing moves


# ----------------------------------------------------------------------------- tolerance
def _params(seed):
    gen = torch.Generator().manual_seed(seed)
    return [(0.05 * torch.randn(n, generator=gen)).to(DEV).requires_grad_(True) for n in SIZES]


def _grads(gen, step):
    """As test_lars_kernels_gpu.py: 25 % exact zeros in the large tensors, one-signed tiny ones,
    step 4 scaled x10."""
    out = []
    for n in SIZES:
        if n < 8:
            g = 0.5 + torch.rand(n, generator=gen)
        else:
            g = torch.randn(n, generator=gen)
            g[torch.rand(n, generator=gen) < 0.25] = 0.0
        out.append(g * (10.0 if step == 4 else 1.0))
    return out


# bias correction on; |w_i| ~ 0.05 and |r_i| <~ 1, so wd = 8 .. 16 makes wd |w| comparable to |r|
LAMB_GRID = [
    dict(lr=0.05, weight_decay=16.0),
    dict(lr=0.05, weight_decay=8.0, eps=1e-3, grad_scale=0.5),
    dict(lr=0.1, weight_decay=16.0, betas=(0.8, 0.99)),
    dict(lr=0.05, weight_decay=0.0),
]


@pytest.mark.parametrize("kw", LAMB_GRID, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_lamb_trust_and_teacher_forced_update(kw):
    """Five steps (the device step counter reads 1..5, the late parameter's 1..3)."""
    ps = _params(11)
    opt = FusedLAMB(ps, **kw)
    gen = torch.Generator().manual_seed(12)
    worst = R.check_random_steps(opt, ps, SIZES, lambda step: _grads(gen, step), 5, sync=torch.cuda.synchronize,
                                 late=LATE)
    counters = sorted(int(ds[0]) for ds in opt._dsteps.values())
    assert counters == [3, 5], counters
    print(f"lamb-errors {kw}: trust {worst['trust']:.2f} u (bound {R.K_TRUST} u = {R.K_TRUST * R.U:.3e}), worst "
          f"element of w, m, v at {worst['elem']:.3f} of its bound, kappa {worst['kappa']:.1f} (cap {R.KAPPA_CAP})")


def test_non_adaptive_group_steps_in_one_launch():
    """adapt=False: trust_of == 1, the same per-element bounds, and the norm scratch is never written
    (the moments kernel applied the update itself: no norm or trust kernel ran)."""
    ps = _params(21)
    opt = FusedLAMB(ps, lr=0.05, weight_decay=8.0, adapt=False)
    gen = torch.Generator().manual_seed(22)
    worst = R.check_random_steps(opt, ps, SIZES, lambda step: _grads(gen, step), 3, sync=torch.cuda.synchronize)
    assert worst["trust"] == 0.0
    tabs = list(opt._tables.values())
    assert len(tabs) == 1 and not bool(tabs[0].partials.any()) and bool((tabs[0].trust == 1).all())
    print(f"lamb-errors non-adaptive: worst element of w, m, v at {worst['elem']:.3f} of its bound")


# ----------------------------------------------------------------------------- device learning rate
def _pair_steps(make, state_keys):
    """Three steps of the host-rate and the device-rate optimizer on the same values, the rate changed
    before every step, a fresh parameter arriving at step 2, gradients aligned and at an odd offset."""
    gen = torch.Generator().manual_seed(41)
    vals = [0.05 * torch.randn(n, generator=gen) for n in SIZES]
    pa = [v.to(DEV).requires_grad_(True) for v in vals]
    pb = [v.to(DEV).requires_grad_(True) for v in vals]
    oa, ob = make(pa, False), make(pb, True)
    assert oa.device_lr is False and ob.device_lr is True
    for step, lr in ((1, 0.1), (2, 0.25), (3, 0.03)):
        for i, n in enumerate(SIZES):
            g = torch.randn(n, generator=gen)
            for p in (pa[i], pb[i]):
                p.grad = None if (i == LATE and step < 2) else _at_offset(g, step % 2)
        for o in (oa, ob):
            for grp in o.param_groups:
                grp["lr"] = lr
            o.push_lr()
            o.step()
        torch.cuda.synchronize()
        for i, n in enumerate(SIZES):
            assert torch.equal(pa[i].detach(), pb[i].detach()), (step, n)
            for k in state_keys:
                if k in oa.state[pa[i]]:
                    assert torch.equal(oa.state[pa[i]][k], ob.state[pb[i]][k]), (step, n, k)
    assert float(ob._lr_dev[0][0]) == pytest.approx(0.03, rel=1e-7) and not oa._lr_dev
    return pa


def test_fused_sgd_device_lr_bit_equal():
    kw = dict(momentum=0.9, nesterov=True, weight_decay=5e-2)
    pa = _pair_steps(lambda ps, d: FusedSGD(ps, lr=0.1, device_lr=d, **kw), ["momentum_buffer"])
    # the changing rate took effect: the same gradients at a constant rate end elsewhere
    gen = torch.Generator().manual_seed(41)
    vals = [0.05 * torch.randn(n, generator=gen) for n in SIZES]
    pc = [v.to(DEV).requires_grad_(True) for v in vals]
    oc = FusedSGD(pc, lr=0.1, device_lr=True, **kw)
    for step in (1, 2, 3):
        for i, n in enumerate(SIZES):
            g = torch.randn(n, generator=gen)
            pc[i].grad = None if (i == LATE and step < 2) else g.to(DEV)
        oc.step()
    assert not torch.equal(pc[-1].detach(), pa[-1].detach())


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_fused_adam_device_lr_bit_equal(decoupled):
    _pair_steps(lambda ps, d: FusedAdam(ps, lr=0.1, weight_decay=5e-2, decoupled=decoupled, device_lr=d),
                ["exp_avg", "exp_avg_sq"])
