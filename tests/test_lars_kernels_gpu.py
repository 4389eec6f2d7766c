"""The LARS kernels of csrc/optim.hip (mt_norm2, lars_trust, mt_lars) through FusedLARS, against the
fp64 oracle of tests/lars_ref.py.

* Exact: on the integer lattice with power-of-two hyper-parameters every intermediate is an fp32
  number (test_lars_cpu.py shows that without a GPU), so parameters, momentum and trust ratios must
  equal the oracle bit for bit -- over tails, chunk boundaries, a tensor of more than 256 chunk
  partials and ~70 small tensors whose trust ratios are all different powers of two.
* Alignment: the same values through views at element offsets 0..3 give the same bits.
* Zero norms give trust exactly 1; a non-adaptive group steps exactly as FusedSGD does.
* Tolerance on random inputs, teacher-forced as in test_optim_kernels_gpu.py.

The tolerance, from the implemented chain (u = 2^-24, first order, every term of the sums of squares
non-negative so relative errors carry through the additions):

    per lane      16 fused multiply-adds in series (x*x is not rounded on its own)       16 u
    wave          6 butterfly levels (wave_sum)                                           6 u
    workgroup     0 + r0 + r1 + r2 + r3 (block_sum; the first addition is exact)          3 u
                  => a chunk partial is within 25 u of its sum of squares
    merge         fp64, fixed order: <= 2^-53 per addition, nothing at this scale         0
    norms         sqrt halves the relative error (12.5 u); |grad_scale| is applied in
                  fp64; one rounding to fp32 each                                         13.5 u
    numerator     eta as fp32 (1 u) * |w| (13.5 u), one rounding                          15.5 u
    denominator   fma(wd, |w|, |g~|): wd as fp32 (1 u) on its share, both terms <= 14.5 u,
                  one rounding (15.5 u); + eps: eps as fp32 on its share and one rounding 17.5 u
    divide        one rounding                                                            1 u

    trust: K = 15.5 + 17.5 + 1 = 34, K u = 2.03e-6.

The update and the momentum buffer are linear in the trust ratio, so they carry that bound plus the
2e-6 that test_optim_kernels_gpu.py allows mt_sgd's element chain (the extra rounding of
trust * (g~ + wd w) stays inside that allowance: it counts five roundings, the chain without weight
decay inside sgd_elem has four).
"""
import pytest
import torch

from ddp_classification_pytorch_amd.optim import FusedLARS, FusedSGD
from tests import head_ref as R
from tests import lars_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
K_TRUST = 34
TRUST_TOL = K_TRUST * U
STEP_TOL = TRUST_TOL + 2e-6

SIZES = [1, 3, 4095, 4096, 4097, 8195]
LATE = 2


# ----------------------------------------------------------------------------- exact
def test_exact_on_lattice_three_steps():
    L.check_exact_steps(FusedLARS, DEV, sync=torch.cuda.synchronize)


def test_exact_weight_decay_in_denominator():
    L.check_exact_wd(FusedLARS, DEV, sync=torch.cuda.synchronize)


# ----------------------------------------------------------------------------- alignment
def _at_offset(values, off):
    """``values`` as a view ``off`` floats into a fresh 16-byte aligned buffer."""
    holder = torch.zeros(values.numel() + 4, device=DEV)
    assert holder.data_ptr() % 16 == 0
    v = holder[off:off + values.numel()]
    v.copy_(values)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _aligned_run(which, off, with_buf, kw):
    """Two steps over SIZES with the parameters, gradients or momentum buffers (``which``) at float
    offset ``off``; ``with_buf``: momentum buffers preset (both steps are not-first launches)."""
    gen = torch.Generator().manual_seed(77)
    vals = [0.05 * torch.randn(n, generator=gen) for n in SIZES]
    bufs = [torch.randn(n, generator=gen) for n in SIZES]
    ps = [_at_offset(v, off if which == "p" else 0).requires_grad_(True) for v in vals]
    opt = FusedLARS(ps, **kw)
    if with_buf:
        for p, b in zip(ps, bufs):
            opt.state[p]["momentum_buffer"] = _at_offset(b, off if which == "b" else 0)
    trusts = []
    for step in (1, 2):
        for p, n in zip(ps, SIZES):
            p.grad = _at_offset(torch.randn(n, generator=gen), off if which == "g" else 0)
        opt.step()
        trusts.append(torch.stack([opt.trust_of(p) for p in ps]).clone())
    torch.cuda.synchronize()
    return ([p.detach().clone() for p in ps], [opt.state[p]["momentum_buffer"].clone() for p in ps], trusts)


@pytest.mark.parametrize("with_buf", [True, False], ids=["carried", "first"])
def test_alignment_offsets_give_identical_bits(with_buf):
    kw = dict(lr=0.3, momentum=0.9, dampening=0.1, weight_decay=5e-2, eta=0.25, eps=1e-3, grad_scale=0.5)
    base = _aligned_run("p", 0, with_buf, kw)
    for which in ("p", "g", "b") if with_buf else ("p", "g"):
        for off in (1, 2, 3):
            got = _aligned_run(which, off, with_buf, kw)
            for i, n in enumerate(SIZES):
                name = (which, off, n)
                assert torch.equal(got[2][0][i], base[2][0][i]) and torch.equal(got[2][1][i], base[2][1][i]), name
                assert torch.equal(got[0][i], base[0][i]), name
                assert torch.equal(got[1][i], base[1][i]), name
    assert all(float(t) != 1.0 for t in base[2][0])


# ----------------------------------------------------------------------------- zero norms, adapt=False
def test_zero_norms_give_trust_one():
    gen = torch.Generator().manual_seed(3)
    for n in (3, 4097):
        w, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        z = torch.zeros(n)
        for pv, gv in ((z, g), (w, z), (z, z)):
            p = pv.to(DEV).requires_grad_(True)
            q = pv.to(DEV).requires_grad_(True)
            p.grad, q.grad = gv.to(DEV), gv.to(DEV)
            ol = FusedLARS([p], lr=0.1, momentum=0.9, weight_decay=0.1, eta=0.25)
            os_ = FusedSGD([q], lr=0.1, momentum=0.9, weight_decay=0.1)
            ol.step()
            os_.step()
            torch.cuda.synchronize()
            assert float(ol.trust_of(p)) == 1.0
            assert torch.equal(p.detach(), q.detach())


@pytest.mark.parametrize("kw", [dict(lr=0.1, momentum=0.9, weight_decay=5e-2, nesterov=True),
                                dict(lr=0.3, momentum=0.9, dampening=0.1, grad_scale=0.5),
                                dict(lr=0.2, momentum=0.0, weight_decay=5e-2)])
def test_non_adaptive_group_equals_fused_sgd_bitwise(kw):
    """One optimizer, an adaptive and a non-adaptive group: the latter's parameters and momentum
    equal FusedSGD's on the same tensors, bit for bit (gradients aligned and at an odd offset)."""
    gen = torch.Generator().manual_seed(41)
    vals = [0.05 * torch.randn(n, generator=gen) for n in SIZES]
    pa = [v.to(DEV).requires_grad_(True) for v in vals]   # adaptive
    pn = [v.to(DEV).requires_grad_(True) for v in vals]   # not adaptive
    ps = [v.to(DEV).requires_grad_(True) for v in vals]   # FusedSGD
    ol = FusedLARS([dict(params=pa), dict(params=pn, adapt=False)], eta=0.25, **kw)
    os_ = FusedSGD(ps, **kw)
    for step in (1, 2, 3):
        for i, n in enumerate(SIZES):
            g = torch.randn(n, generator=gen)
            for p in (pa[i], pn[i], ps[i]):
                p.grad = None if (i == LATE and step < 3) else _at_offset(g, step % 2)
        ol.step()
        os_.step()
        torch.cuda.synchronize()
        for i, n in enumerate(SIZES):
            assert torch.equal(pn[i].detach(), ps[i].detach()), (step, n)
            if kw["momentum"] and pn[i].grad is not None:
                assert torch.equal(ol.state[pn[i]]["momentum_buffer"], os_.state[ps[i]]["momentum_buffer"]), (step, n)
            if pn[i].grad is not None:
                assert float(ol.trust_of(pn[i])) == 1.0 and float(ol.trust_of(pa[i])) != 1.0
                assert not torch.equal(pa[i].detach(), pn[i].detach()), (step, n)


# ----------------------------------------------------------------------------- tolerance
def _params(seed):
    gen = torch.Generator().manual_seed(seed)
    return [(0.05 * torch.randn(n, generator=gen)).to(DEV).requires_grad_(True) for n in SIZES]


def _grads(gen, step):
    """As test_optim_kernels_gpu.py: 25 % exact zeros in the large tensors, one-signed tiny ones,
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


# SGD_GRID of test_optim_kernels_gpu.py with eta, eps and wd; lr * eta >= 1/40, so the update is at
# least |p| / 40 (|delta| ~ lr eta |w|): the stored parameter's rounding stays below the tolerance
LARS_GRID = [
    dict(lr=0.1, momentum=0.0, eta=0.25),
    dict(lr=0.1, momentum=0.0, weight_decay=5e-2, eta=0.25, eps=1e-3),
    dict(lr=0.5, momentum=0.9, eta=0.125, eps=0.0),
    dict(lr=0.3, momentum=0.9, dampening=0.1, weight_decay=5e-2, eta=0.25, eps=1e-2),
    dict(lr=0.2, momentum=0.9, nesterov=True, eta=0.5),
    dict(lr=0.2, momentum=0.9, nesterov=True, weight_decay=5e-2, grad_scale=0.5, eta=0.25, eps=1e-3),
    dict(lr=0.4, momentum=0.0, grad_scale=0.5, eta=0.125, weight_decay=0.5),
]


@pytest.mark.parametrize("kw", LARS_GRID, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_lars_update_teacher_forced(kw):
    ps = _params(11)
    opt = FusedLARS(ps, **kw)
    h = opt.param_groups[0]
    gen = torch.Generator().manual_seed(12)
    worst = {"trust": 0.0, "update": 0.0, "buf": 0.0}
    fails = []
    for step in range(1, 6):
        gs = _grads(gen, step)
        before = [p.detach().clone() for p in ps]
        bufs = [opt.state[p].get("momentum_buffer") for p in ps]
        bufs = [None if b is None else b.clone() for b in bufs]
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if (i == LATE and step < 3) else g.to(DEV)
        opt.step()
        torch.cuda.synchronize()
        for i, (p, g) in enumerate(zip(ps, gs)):
            name = (step, SIZES[i])
            if p.grad is None:
                assert torch.equal(p.detach(), before[i]) and "momentum_buffer" not in opt.state[p], name
                continue
            first = bufs[i] is None
            assert first == (step == (3 if i == LATE else 1)) or h["momentum"] == 0
            ref_p, ref_buf, ref_t = L.lars_step(before[i], g, bufs[i], first, h["lr"], h["momentum"], h["dampening"],
                                                h["weight_decay"], h["nesterov"], h["grad_scale"], h["eta"], h["eps"])
            assert ref_t != 1.0
            et = abs(float(opt.trust_of(p)) - ref_t) / ref_t
            ref_delta = ref_p - R.f64(before[i])
            ratio = (R.f64(before[i]).norm() / ref_delta.norm()).item()
            assert ratio <= 64, (name, ratio)
            eu = R.relerr(R.f64(p.detach()) - R.f64(before[i]), ref_delta)
            eb = R.relerr(opt.state[p]["momentum_buffer"], ref_buf) if h["momentum"] != 0 else 0.0
            worst = {"trust": max(worst["trust"], et), "update": max(worst["update"], eu), "buf": max(worst["buf"], eb)}
            if et > TRUST_TOL or eu > STEP_TOL or eb > STEP_TOL:
                fails.append((name, et, eu, eb))
    print(f"lars-errors {kw}: trust {worst['trust']:.3e} (bound {TRUST_TOL:.3e}) update {worst['update']:.3e} "
          f"momentum {worst['buf']:.3e} (bound {STEP_TOL:.3e})")
    assert not fails, fails
