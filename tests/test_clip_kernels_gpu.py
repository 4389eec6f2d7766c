"""mt_gnorm2 / gnorm_finish and the clip block in the update kernels (csrc/optim.hip), through the
four fused optimizers and the raw ops.

Shapes: the smallest that reach every loop edge -- 1, 3, 4095, 4096, 4097 and 2*4096+5 elements, one
tensor of 301 chunks (the merge has more partials than threads), 70 tensors of a few elements, and
parameter / gradient / state views at float offsets 0..3 (the 4-byte loops).

1. Twin equality: a clipped step == the plain step with grad_scale' = fl32(grad_scale * coef), bit for bit.
2. The norm is exact on a lattice; the coefficient is then an exact power of two.
3. The norm's bits do not depend on the route (step() or norm_params() over subsets in any order) or on
   the tensors' alignment.
4. On random inputs the norm is within clip_ref.K_NORM u of fp64.
5. A NaN / inf gradient: with skip_nonfinite nothing is written; without it the coefficient is NaN / 0.
6. A parameter without a gradient takes no part (no stale slot of the step before).
7. LARS trust_clip and LAMB phi on the exact lattices of lars_ref / lamb_ref.
"""
import copy
import math

import numpy as np
import pytest
import torch

from ddp_classification_pytorch_amd.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD
from tests import clip_ref as C
from tests import lamb_ref as R
from tests import lars_ref as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CHUNK = 4096
EDGE = [1, 3, 4095, 4096, 4097, 2 * CHUNK + 5]
BIG = 300 * CHUNK + 5                        # 301 chunks
SMALL = [5 + 3 * i for i in range(70)]
SIZES = EDGE + [BIG] + SMALL

MAKERS = {
    "sgd": (FusedSGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-3, grad_scale=0.5), ("momentum_buffer",)),
    "adam": (FusedAdam, dict(lr=1e-2, weight_decay=1e-3, grad_scale=0.5), ("exp_avg", "exp_avg_sq")),
    "lars": (FusedLARS, dict(lr=0.1, momentum=0.9, weight_decay=1e-3, grad_scale=0.5, eta=0.02), ("momentum_buffer",)),
    "lamb": (FusedLAMB, dict(lr=1e-2, weight_decay=1e-2, grad_scale=0.5), ("exp_avg", "exp_avg_sq")),
}


def _at_offset(values, off):
    """``values`` on the device as a view ``off`` floats into a fresh 16-byte aligned buffer."""
    holder = torch.zeros(values.numel() + 8, device=DEV)
    assert holder.data_ptr() % 16 == 0
    v = holder[off:off + values.numel()]
    v.copy_(values)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _draw(seed, scale=1.0, sizes=SIZES):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * scale for n in sizes]


@pytest.fixture(scope="module")
def values():
    """Host values shared (and left unchanged) by the tests: parameters and three gradient sets."""
    return dict(p=_draw(1), g=[_draw(10), _draw(11), _draw(12)])


def _params(vals, shift=0):
    """Parameter i at float offset (i + shift) % 4."""
    return [_at_offset(v, (i + shift) % 4).requires_grad_(True) for i, v in enumerate(vals)]


def _set_grads(ps, grads, shift=1, scale=1.0):
    for i, (p, g) in enumerate(zip(ps, grads)):
        p.grad = None if g is None else _at_offset(g * scale, (i + shift) % 4)


def _groups(ps):
    """Two groups with their own grad_scale: the norm weights each group with its own."""
    k = len(EDGE) + 1
    return [dict(params=ps[:k]), dict(params=ps[k:], grad_scale=2.0)]


def _scales(opt):
    return [g["grad_scale"] for g in opt.param_groups for _ in g["params"]]


def _offset_state(opt, ps, keys):
    """Move the optimizer's state tensors into views at float offsets 1..3."""
    for i, p in enumerate(ps):
        for k in keys:
            if k in opt.state[p]:
                opt.state[p][k] = _at_offset(opt.state[p][k], 1 + i % 3)
    getattr(opt, "_fast", {}).clear()   # the SGD family's cached tables point at the old buffers


# ----------------------------------------------------------------------------- 1. twin equality
@pytest.mark.parametrize("name", sorted(MAKERS))
@pytest.mark.parametrize("gscale,clipped", [(1.0, True), (2.0 ** -14, False)])
def test_clipped_step_equals_plain_step_with_scaled_grad_scale(values, name, gscale, clipped):
    cls, kw, keys = MAKERS[name]
    ps = _params(values["p"])
    opt = cls(_groups(ps), max_grad_norm=1.0, **kw)
    for step in (1, 2):       # a first step (fresh state) and a carried one (state views at offsets 1..3)
        if step == 2:
            _offset_state(opt, ps, keys)
        twin_ps = _params([p.detach().cpu() for p in ps], shift=2)
        sd = copy.deepcopy(opt.state_dict())
        _set_grads(ps, values["g"][step], scale=gscale)
        opt.step()
        coef = np.float32(float(opt.clip_coef()))
        assert (coef < 1) == clipped and coef > 0, (step, coef)
        if not clipped:
            assert coef == 1.0      # exactly 1: the twin below IS the plain optimizer
        twin = cls(_groups(twin_ps), **kw)
        twin.load_state_dict(sd)
        for g in twin.param_groups:
            g["grad_scale"] = C.eff_scale(g["grad_scale"], coef)
        _set_grads(twin_ps, values["g"][step], shift=3, scale=gscale)
        twin.step()
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(ps, twin_ps)):
            assert torch.equal(p, q), (step, SIZES[i])
            assert not torch.equal(p.detach().cpu(), values["p"][i]), (step, SIZES[i])
            for k in keys:
                assert torch.equal(opt.state[p][k], twin.state[q][k]), (step, SIZES[i], k)
            if hasattr(opt, "trust_of"):
                assert torch.equal(opt.trust_of(p), twin.trust_of(q)), (step, SIZES[i])


# ----------------------------------------------------------------------------- 2. exact on the lattice
@pytest.mark.parametrize("max_norm,want_coef", [(4.0, 2.0 ** -4), (2.0 ** -3, 2.0 ** -9), (128.0, 1.0)])
def test_norm_and_coefficient_are_exact_on_the_lattice(max_norm, want_coef):
    gen = torch.Generator().manual_seed(7)
    grads = C.norm_lattice(SIZES, 5, -3, gen)        # 4^8 entries of +-1/8: |g| = 32; grad_scale 2: norm 64
    assert sum(int((g != 0).sum()) for g in grads) == 4 ** 8 and all(int((g != 0).sum()) > 0 for g in grads)
    norm = C.global_norm(grads, [2.0] * len(grads))
    assert norm == 64.0 and C.eps_is_absorbed(norm)   # the precondition: 64 + 1e-6 rounds back to 64
    coef = C.clip_coef(norm, max_norm)
    assert coef == want_coef
    for shift in (0, 1):
        ps = _params([torch.zeros(n) for n in SIZES])
        opt = FusedSGD(ps, lr=0.0, grad_scale=2.0, max_grad_norm=max_norm)
        _set_grads(ps, grads, shift=shift)
        opt.step()
        assert torch.equal(opt.grad_norm().cpu(), torch.tensor(float(norm))), shift
        assert torch.equal(opt.clip_coef().cpu(), torch.tensor(float(coef))), shift
        assert int(opt.skipped_steps()) == 0


# ----------------------------------------------------------------------------- 3. route and alignment
def test_norm_bits_do_not_depend_on_route_or_alignment(values):
    def make(shift):
        ps = _params(values["p"], shift)
        return ps, FusedLARS(_groups(ps), lr=0.1, momentum=0.9, max_grad_norm=1.0)

    ps, opt = make(0)
    _set_grads(ps, values["g"][0])
    opt.step()
    ref_norm, ref_coef = opt.grad_norm().clone(), opt.clip_coef().clone()
    ref_p = [p.detach().clone() for p in ps]
    assert float(ref_coef) < 1.0
    subsets = [list(range(0, len(SIZES), 3)), list(range(1, len(SIZES), 3)), list(range(2, len(SIZES), 3))]
    for order, shift, gshift in (((0, 1, 2), 0, 1), ((2, 0, 1), 1, 3), ((1, 2, 0), 3, 0)):
        ps, opt = make(shift)
        _set_grads(ps, values["g"][0], shift=gshift)
        for k in order:
            opt.norm_params([ps[i] for i in reversed(subsets[k])])
        opt.step_after_norms()
        assert torch.equal(opt.grad_norm(), ref_norm), order
        assert torch.equal(opt.clip_coef(), ref_coef), order
        for i, (p, q) in enumerate(zip(ps, ref_p)):
            assert torch.equal(p, q), (order, SIZES[i])
    # all tensors at every alignment through step()
    for shift in (1, 2, 3):
        ps = [_at_offset(v, shift).requires_grad_(True) for v in values["p"]]
        opt = FusedLARS(_groups(ps), lr=0.1, momentum=0.9, max_grad_norm=1.0)
        for p, g in zip(ps, values["g"][0]):
            p.grad = _at_offset(g, shift)
        opt.step()
        assert torch.equal(opt.grad_norm(), ref_norm), shift


# ----------------------------------------------------------------------------- 4. the bound
def test_norm_within_its_bound_on_random_inputs(values):
    """Measured on MI355X: 0.28 / 0.39 / 0.69 u at the three scales against the bound of 13.5 u
    (profiles/r14/clip_step.txt)."""
    worst = 0.0
    for k, scale in enumerate((1.0, 1e-3, 37.0)):
        ps = _params(values["p"])
        opt = FusedAdam(_groups(ps), lr=1e-3, grad_scale=0.5, max_grad_norm=1.0)
        _set_grads(ps, values["g"][k], scale=scale)
        opt.step()
        ref = C.global_norm64([g * scale for g in values["g"][k]], _scales(opt))
        err = abs(float(opt.grad_norm()) - ref) / ref / C.U
        print(f"norm error: scale {scale:g}  {err:.3f} u  (bound {C.K_NORM} u)")
        worst = max(worst, err)
        assert err <= C.K_NORM * C.SLACK, (scale, err)
    print(f"norm error worst: {worst:.3f} u")


# ----------------------------------------------------------------------------- 5. skipping
@pytest.mark.parametrize("name", sorted(MAKERS))
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_gradient_skips_the_step(values, name, bad):
    cls, kw, keys = MAKERS[name]
    ps = _params(values["p"])
    opt = cls(_groups(ps), max_grad_norm=1.0, skip_nonfinite=True, **kw)
    for k in (0, 2):               # two finite steps: the carried (not-first) launch has run and owns its scratch
        _set_grads(ps, values["g"][k])
        opt.step()
    _offset_state(opt, ps, keys)
    before_p = [p.detach().clone() for p in ps]
    before_s = [[opt.state[p][k].clone() for k in keys] for p in ps]
    before_t = [opt.trust_of(p).clone() for p in ps] if hasattr(opt, "trust_of") else None
    steps = [opt.state[p].get("step") for p in ps]
    poisoned = [g.clone() for g in values["g"][1]]
    poisoned[4][CHUNK] = bad       # the first element of a second chunk
    _set_grads(ps, poisoned)
    opt.step()
    torch.cuda.synchronize()
    assert int(opt.skipped_steps()) == 1
    assert not math.isfinite(float(opt.grad_norm()))
    for i, p in enumerate(ps):
        assert torch.equal(p, before_p[i]), SIZES[i]
        for k, b in zip(keys, before_s[i]):
            assert torch.equal(opt.state[p][k], b), (SIZES[i], k)
        if before_t is not None:
            assert torch.equal(opt.trust_of(p), before_t[i]), SIZES[i]
    if steps[0] is not None:       # Adam / LAMB: the bias-correction count advances all the same
        assert [opt.state[p]["step"] for p in ps] == [s + 1 for s in steps]
    _set_grads(ps, values["g"][0])
    opt.step()
    assert int(opt.skipped_steps()) == 1 and math.isfinite(float(opt.grad_norm()))
    for i, p in enumerate(ps):
        assert not torch.equal(p, before_p[i]) and bool(torch.isfinite(p).all()), SIZES[i]
    # without skip_nonfinite: clip_grad_norm_'s coefficient (NaN for a NaN norm, 0 for inf)
    ps2 = _params(values["p"])
    opt2 = cls(_groups(ps2), max_grad_norm=1.0, **kw)
    _set_grads(ps2, poisoned)
    opt2.step()
    c = float(opt2.clip_coef())
    assert math.isnan(c) if math.isnan(bad) else c == 0.0
    assert int(opt2.skipped_steps()) == 0


def _table(rows):
    from ddp_classification_pytorch_amd.ops import functional as Fn

    n = [r[5] for r in rows]
    chunks = [[i, c] for i, k in enumerate(n) for c in range((k + CHUNK - 1) // CHUNK)]
    return (Fn.table_to_device([list(r) for r in rows], torch.int64, DEV).view(-1, 6),
            Fn.table_to_device(chunks, torch.int32, DEV).view(-1, 2))


@pytest.mark.parametrize("off", [0, 1])
def test_raw_ops_with_a_set_skip_flag_leave_the_bf16_shadow_alone(off):
    """The ops' trailing control-block argument: a set flag returns before parameters, state and the bf16
    shadow are touched; a coefficient of 1/2 without the flag halves grad_scale; None is today's step."""
    from ddp_classification_pytorch_amd import _ext

    K = _ext.hip_ops()
    gen = torch.Generator().manual_seed(3)
    n = CHUNK + 8
    vals = [torch.randn(n, generator=gen) for _ in range(4)]

    def run(op, ctl, gs):
        p, g, s1, s2 = (_at_offset(v, off) for v in vals)
        s2.abs_()
        shadow = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=DEV)[off:off + n]
        table, chunks = _table([(p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), shadow.data_ptr(), n)])
        if op == "lars":
            K.mt_lars(table, chunks, None, None, None, 0.1, 0.9, 0.0, 1e-3, False, False, gs, 0.0, 0.0, None, ctl)
        elif op == "adam":
            K.mt_adam(table, chunks, 1e-2, 0.9, 0.999, 1e-8, 1e-3, 3, False, gs, None, None, ctl)
        else:
            K.mt_lamb(table, chunks, None, None, None, 1e-2, 0.9, 0.999, 1e-6, 1e-2, 3, True, gs, None, None, ctl)
        torch.cuda.synchronize()
        return [t.clone() for t in (p, s1, s2, shadow)]

    def ctl(coef, skip):
        c = torch.zeros(8, dtype=torch.float32, device=DEV)
        c[0] = coef
        c.view(torch.int32)[1] = skip
        return c

    for op in ("lars", "adam", "lamb"):
        plain = run(op, None, 0.5)
        half = run(op, ctl(0.5, 0), 1.0)
        skipped = run(op, ctl(0.5, 1), 1.0)
        start = [_at_offset(vals[0], off), _at_offset(vals[2], off), _at_offset(vals[3], off).abs_()]
        for a, b in zip(plain, half):
            assert torch.equal(a, b), op
        assert not torch.equal(plain[0], start[0]) and not bool((plain[3] == 7.0).any()), op
        assert torch.equal(skipped[0], start[0]) and torch.equal(skipped[1], start[1]), op
        if op != "lars":
            assert torch.equal(skipped[2], start[2]), op
        assert bool((skipped[3] == 7.0).all()), op


# ----------------------------------------------------------------------------- 6. no gradient
def test_parameter_without_gradient_takes_no_part_in_the_next_norm(values):
    ps = _params(values["p"])
    opt = FusedSGD(_groups(ps), lr=0.1, momentum=0.9, max_grad_norm=1.0)
    _set_grads(ps, values["g"][0])
    opt.step()
    with_all = opt.grad_norm().clone()
    missing = (4, len(EDGE))       # a two-chunk tensor and the 301-chunk one
    grads = [None if i in missing else g for i, g in enumerate(values["g"][0])]
    _set_grads(ps, grads)
    opt.step()                     # their slots still hold the sums of the step before
    got = opt.grad_norm().clone()
    ps2 = _params(values["p"])
    fresh = FusedSGD(_groups(ps2), lr=0.1, momentum=0.9, max_grad_norm=1.0)
    _set_grads(ps2, grads)
    fresh.step()
    assert torch.equal(got, fresh.grad_norm()) and not torch.equal(got, with_all)
    ref = C.global_norm64(grads, _scales(opt))
    assert abs(float(got) - ref) / ref <= C.K_NORM * C.SLACK * C.U
    _set_grads(ps, values["g"][0])  # and back
    opt.step()
    assert torch.equal(opt.grad_norm(), with_all)


# ----------------------------------------------------------------------------- 7. trust clipping
def test_lars_trust_clip_on_the_exact_lattice():
    gen = torch.Generator().manual_seed(99)
    sizes = L.EXACT_SIZES
    h = L.EXACT_HYPER
    ps = [torch.zeros(n, device=DEV).requires_grad_(True) for n in sizes]
    opt = FusedLARS(ps, trust_clip=True, **h)
    kinds = set()
    draws = [L.exact_draw(i, n, gen) for i, n in enumerate(sizes)]
    for p, (pv, gv) in zip(ps, draws):
        p.data.copy_(pv)
        p.grad = gv.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    for i, (p, (pv, gv)) in enumerate(zip(ps, draws)):
        kw, kg = L.exact_exponents(i)
        raw = h["eta"] * 2.0 ** (kw - kg + 1)             # the lattice's unclipped ratio, a power of two
        assert L.trust_ratio(pv, gv, 0.0, h["grad_scale"], h["eta"], 0.0) == raw
        want = C.lars_trust_clip(raw, h["lr"])
        kinds.add("below" if raw < h["lr"] else "above" if raw > h["lr"] else "on")
        assert torch.equal(opt.trust_of(p).cpu(), torch.tensor(float(want))), (sizes[i], raw)
        _, ref_buf, _ = L.lars_step(pv, gv, None, True, h["lr"], h["momentum"], 0.0, 0.0, False, h["grad_scale"],
                                        h["eta"], 0.0, trust=float(want))
        # the clipped ratio went into the update: d = trust (grad_scale g) is exact on the lattice (w - lr d is
        # not: the clipped ratio no longer scales with |w|, so the sum need not be an fp32 number)
        assert L.is_fp32(ref_buf) and torch.equal(opt.state[p]["momentum_buffer"].cpu(), ref_buf.float()), sizes[i]
    assert kinds == {"below", "above", "on"}
    # off (the default, and said explicitly): the unclamped optimizer, bit for bit
    L.check_exact_steps(lambda params, **kw: FusedLARS(params, trust_clip=False, **kw), DEV, sync=torch.cuda.synchronize)


def test_lamb_phi_on_the_exact_lattice():
    gen = torch.Generator().manual_seed(98)
    sizes = R.EXACT_SIZES
    h = R.EXACT_HYPER
    lo, hi = 2.0 ** -10, 2.0 ** 10
    ps = [torch.zeros(n, device=DEV).requires_grad_(True) for n in sizes]
    opt = FusedLAMB(ps, phi_min=lo, phi_max=hi, **h)
    kinds = set()
    draws = [R.exact_draw(i, n, gen) for i, n in enumerate(sizes)]
    for p, (w, g) in zip(ps, draws):
        p.data.copy_(w)
        p.grad = g.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    for i, (p, (w, g)) in enumerate(zip(ps, draws)):
        a = R.grad_count_exp(sizes[i])
        wn, un = 2.0 ** (R.exact_trust_exp(i) + a - 1), 2.0 ** (a - 1)
        assert L.sumsq(w) ** 0.5 == wn
        want = float(C.lamb_trust_phi(wn, un, lo, hi))
        kinds.add("below" if wn < lo else "above" if wn > hi else "on" if wn in (lo, hi) else "inside")
        assert torch.equal(opt.trust_of(p).cpu(), torch.tensor(want)), (sizes[i], wn)
        ref = R.lamb_step(w, g, torch.zeros_like(w), torch.zeros_like(w), 1, h["lr"], h["betas"], h["eps"], 0.0, 1.0,
                          False, trust=want)
        assert ref["un"] == un and torch.equal(p.detach().cpu(), ref["p"].float()), sizes[i]
    assert kinds == {"below", "above", "on", "inside"}
    R.check_exact_steps(lambda params: FusedLAMB(params, phi_min=0.0, phi_max=math.inf, **h), DEV,
                        sync=torch.cuda.synchronize)
