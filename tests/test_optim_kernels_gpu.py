"""The multi-tensor kernels of csrc/optim.hip against fp64 / exact references (tests/head_ref.py).

* SGD and Adam/AdamW, teacher-forced: before every step the fp32 parameters and optimizer state are
  copied to fp64, the textbook update is applied there, and the *update* p_after - p_before and each
  state buffer are compared (a parameter-level comparison hides an error of the step under the O(1)
  parameter).  Parameters are small (0.05 randn) against steps of 1e-2 .. 0.5, and the tests assert
  |p| / |delta| <= 64, so the fp32 rounding of the stored parameter (rms 2.6e-8 |p|) stays below
  the tolerances: 1e-5 for Adam (the CPU fp32 path of the same formulas measures <= 1e-6 against
  this reference, leaving 10x for expm1f / logf), 2e-6 for SGD (five fp32 roundings per element).
* the SGD 16-byte path against the 4-byte path, bit for bit.
* mt_copy: all four type modes, exact.
* the CDR radix select: exact threshold and masked gradients at ties, zeros, k = 1, k = n and
  chunk-boundary sizes.
"""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.algos.cdr import cdr_mask_gradients
from ddp_classification_pytorch_amd.ops import functional as Fn
from ddp_classification_pytorch_amd.optim import FusedAdam, FusedSGD
from tests import head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# tails that are no multiple of 4, the exact chunk size (4096) and one past it
SIZES = [1, 3, 4095, 4096, 4097, 8195]
LATE = 2        # index (in SIZES) of the parameter whose first gradient arrives at step 3
X10_STEP = 4    # the step whose gradients are scaled x10


def _params(seed, sizes=SIZES):
    gen = torch.Generator().manual_seed(seed)
    return [(0.05 * torch.randn(n, generator=gen)).to(DEV).requires_grad_(True) for n in sizes]


def _grads(gen, step, sizes=SIZES):
    """Random gradients; the large tensors carry 25 % exact zeros, the tiny ones are in [0.5, 1.5)
    (one sign, away from zero: a momentum or first-moment average of a single element never cancels
    to an update that is tiny against the parameter)."""
    out = []
    for n in sizes:
        if n < 8:
            g = 0.5 + torch.rand(n, generator=gen)
        else:
            g = torch.randn(n, generator=gen)
            g[torch.rand(n, generator=gen) < 0.25] = 0.0
        out.append(g * (10.0 if step == X10_STEP else 1.0))
    return out


def _check_update(name, before, after, ref_after, tol):
    ref_delta = ref_after - R.f64(before)
    ratio = (R.f64(before).norm() / ref_delta.norm()).item()
    assert ratio <= 64, (name, ratio)
    err = R.relerr(R.f64(after) - R.f64(before), ref_delta)
    assert err <= tol, (name, err)


def _check_state(name, got, ref, tol):
    err = R.relerr(got, ref)
    assert err <= tol, (name, err)


SGD_GRID = [
    dict(lr=0.1, momentum=0.0),
    dict(lr=0.1, momentum=0.0, weight_decay=5e-2),
    dict(lr=0.5, momentum=0.9),
    dict(lr=0.3, momentum=0.9, dampening=0.1, weight_decay=5e-2),
    dict(lr=0.2, momentum=0.9, nesterov=True),
    dict(lr=0.2, momentum=0.9, nesterov=True, weight_decay=5e-2, grad_scale=0.5),
    dict(lr=0.4, momentum=0.0, grad_scale=0.5),
]


@pytest.mark.parametrize("kw", SGD_GRID, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_sgd_update_teacher_forced(kw):
    tol = 2e-6
    ps = _params(11)
    opt = FusedSGD(ps, **kw)
    h = opt.param_groups[0]
    gen = torch.Generator().manual_seed(12)
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
            # its first gradient: a first=True launch of its own (step 3 for the late parameter)
            first = bufs[i] is None
            assert first == (step == (3 if i == LATE else 1)) or h["momentum"] == 0
            ref_p, ref_buf = R.sgd_step(before[i], g, bufs[i], first, h["lr"], h["momentum"], h["dampening"],
                                        h["weight_decay"], h["nesterov"], h["grad_scale"])
            _check_update(name, before[i], p.detach(), ref_p, tol)
            if h["momentum"] != 0:
                _check_state(name, opt.state[p]["momentum_buffer"], ref_buf, tol)


ADAM_GRID = [
    dict(lr=1e-2),
    dict(lr=1e-2, weight_decay=1e-1),
    dict(lr=1e-2, weight_decay=1e-1, decoupled=True),
    dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-3),
    dict(lr=1e-2, weight_decay=1e-1, decoupled=True, betas=(0.8, 0.99), grad_scale=0.5),
    dict(lr=1e-2, weight_decay=1e-1, eps=1e-3, grad_scale=0.5),
]


def _adam_steps(kw, sizes, steps, late):
    tol = 1e-5
    ps = _params(21, sizes)
    opt = FusedAdam(ps, **kw)
    h = opt.param_groups[0]
    gen = torch.Generator().manual_seed(22)
    for step in range(1, steps + 1):
        gs = _grads(gen, step, sizes)
        before = [p.detach().clone() for p in ps]
        st = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) if "step" in opt.state[p]
              else (torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if (i == late and step < 3) else g.to(DEV)
        opt.step()
        torch.cuda.synchronize()
        for i, (p, g) in enumerate(zip(ps, gs)):
            name = (step, sizes[i])
            if p.grad is None:
                assert torch.equal(p.detach(), before[i]) and "step" not in opt.state[p], name
                continue
            t = opt.state[p]["step"]
            assert t == (step - 2 if i == late else step), name  # two step counts in one group
            ref_p, ref_m, ref_v = R.adam_step(before[i], g, st[i][0], st[i][1], t, h["lr"], h["betas"], h["eps"],
                                              h["weight_decay"], h["decoupled"], h["grad_scale"])
            _check_update(name, before[i], p.detach(), ref_p, tol)
            _check_state(name, opt.state[p]["exp_avg"], ref_m, tol)
            _check_state(name, opt.state[p]["exp_avg_sq"], ref_v, tol)


@pytest.mark.parametrize("kw", ADAM_GRID, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_adam_update_teacher_forced(kw):
    """Every eager GPU step takes the in-kernel bias correction -expm1f(t logf(beta)) (step_dev)."""
    _adam_steps(kw, SIZES, 5, LATE)


def test_adam_bias_correction_30_steps():
    """Bias correction away from step 1: at t = 30, 1 - 0.999^t = 0.03 (still far from 1) and
    1 - 0.9^t = 0.96."""
    _adam_steps(dict(lr=1e-2, weight_decay=1e-1), [1, 3, 4097], 30, 1)


@pytest.mark.parametrize("kw", [dict(lr=0.1, momentum=0.9, weight_decay=5e-2, nesterov=True),
                                dict(lr=0.3, momentum=0.9, dampening=0.1), dict(lr=0.2, momentum=0.0, grad_scale=0.5)])
def test_sgd_16_byte_path_matches_4_byte_path_bitwise(kw):
    """The same steps with the gradients in aligned storage (full chunks take the 16-byte path) and
    as views one element into a buffer (every chunk takes the 4-byte loop): identical parameters and
    momentum."""
    pa, pb = _params(31), _params(31)
    oa, ob = FusedSGD(pa, **kw), FusedSGD(pb, **kw)
    gen = torch.Generator().manual_seed(32)
    for step in range(1, 4):
        gs = _grads(gen, step)
        for p, q, g in zip(pa, pb, gs):
            p.grad = g.to(DEV)
            assert p.grad.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
            holder = torch.empty(g.numel() + 1, device=DEV)
            holder[1:].copy_(g)
            q.grad = holder[1:]
            assert q.grad.data_ptr() % 16 == 4
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        for n, p, q in zip(SIZES, pa, pb):
            assert torch.equal(p.detach(), q.detach()), (step, n)
            if kw["momentum"]:
                assert torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"]), (step, n)


@pytest.mark.parametrize("scale", [1.0, 1.0 / 8, 1.0 / 3])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_mt_copy_exact(mode, scale):
    """dst = src * scale per table entry; mode bit 0: bf16 source, bit 1: bf16 destination.  Source
    and destination are views at odd element offsets; everything around them stays untouched."""
    K = _ext.hip_ops()
    src_dt = torch.bfloat16 if mode & 1 else torch.float32
    dst_dt = torch.bfloat16 if mode & 2 else torch.float32
    gen = torch.Generator().manual_seed(40 + mode)
    total = sum(SIZES) + 2 * len(SIZES) + 8
    src = torch.randn(total, generator=gen).to(src_dt).to(DEV)
    dst = torch.full((total,), -7.0, dtype=dst_dt, device=DEV)
    rows, chunks, views, so, do = [], [], [], 1, 3
    for i, n in enumerate(SIZES):
        sv, dv = src[so:so + n], dst[do:do + n]
        rows.append([dv.data_ptr(), sv.data_ptr(), 0, 0, 0, n])
        chunks.extend((i, c) for c in range((n + 4095) // 4096))
        views.append((so, do, n))
        so, do = so + n + 1 + (i % 2), do + n + 2 - (i % 2)   # odd and even gaps
    table = Fn.table_to_device(rows, torch.int64, DEV).view(-1, 6)
    ch = Fn.table_to_device(chunks, torch.int32, DEV).view(-1, 2)
    K.mt_copy(table, ch, scale, mode)
    torch.cuda.synchronize()
    want = torch.full((total,), -7.0, dtype=dst_dt)
    srcc = src.cpu()
    for so, do, n in views:
        prod = srcc[so:so + n].float() * torch.tensor(scale, dtype=torch.float32)
        want[do:do + n] = prod.to(dst_dt)
    assert torch.equal(dst.cpu(), want)


# ----------------------------------------------------------------------------- CDR radix select
def _cdr_case(params, grads, ratio, clip=0.8, check_k=None):
    """Run cdr_mask_gradients on the GPU and the reference on the CPU -> (threshold, reference
    threshold); asserts exact equality of the threshold and of every gradient."""
    pd = [p.to(DEV).requires_grad_(True) for p in params]
    for p, g in zip(pd, grads):
        p.grad = g.to(DEV)
    return pd, _cdr_call(pd, params, grads, ratio, clip, check_k)


def _cdr_call(pd, params, grads, ratio, clip=0.8, check_k=None):
    n = sum(p.numel() for p in params if p.dim() in (2, 4))
    if check_k is not None:
        assert int(ratio * n) == check_k
    for p, g in zip(params, grads):  # normal fp32 products or exact zeros only
        pr = (g * p).abs()
        assert torch.isfinite(pr).all() and ((pr == 0) | (pr >= 2.0 ** -126)).all()
    ref_thr, ref_g = R.cdr_select(params, grads, ratio, clip)
    thr = cdr_mask_gradients(pd, nonzero_ratio=ratio, clip=clip)
    torch.cuda.synchronize()
    assert torch.equal(thr.detach().cpu().float().reshape(()), ref_thr.reshape(())), (float(thr), float(ref_thr))
    for p, rg in zip(pd, ref_g):
        assert torch.equal(p.grad.cpu(), rg), tuple(p.shape)
    return ref_thr


def _cdr_tensors(seed):
    """4096 and 4097 elements (a tensor ending at a chunk boundary and one element past it) next to a
    1-D tensor the mask must not touch."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(64, 64, generator=gen), torch.randn(17, 241, generator=gen), torch.randn(37, generator=gen)]
    grads = [torch.randn(p.shape, generator=gen) for p in params]
    assert params[0].numel() == 4096 and params[1].numel() == 4097
    return params, grads


N_CDR = 4096 + 4097


@pytest.mark.parametrize("ratio,k", [(1.5 / N_CDR, 1), (1.0, N_CDR), (0.8, int(0.8 * N_CDR)), (0.0, 0)])
def test_cdr_select_k_extremes(ratio, k):
    params, grads = _cdr_tensors(50)
    _cdr_case(params, grads, ratio, check_k=k)


def test_cdr_select_zeros_reach_k():
    """40 % of the products are exactly zero (dead filters: a zero gradient, or a zero weight under a
    live gradient) and k reaches into them: the threshold is 0 and every gradient is kept (scaled by
    clip), those on zero weights included."""
    params, grads = _cdr_tensors(51)
    gen = torch.Generator().manual_seed(52)
    for p, g in zip(params[:2], grads[:2]):
        u = torch.rand(g.shape, generator=gen)
        g[u < 0.2] = 0.0
        p[(u >= 0.2) & (u < 0.4)] = 0.0
    zeros = sum(int(((g * p) == 0).sum()) for p, g in zip(params[:2], grads[:2]))
    assert N_CDR - zeros < int(0.8 * N_CDR)
    pd, thr = _cdr_case(params, grads, 0.8)
    assert float(thr) == 0.0
    assert all(int((q.grad != 0).sum()) == int((g != 0).sum()) for q, g in zip(pd[:2], grads[:2]))


def test_cdr_select_ties_at_threshold():
    """A product duplicated 100 times straddles k: all 100 are kept."""
    params, grads = _cdr_tensors(53)
    params = [torch.ones_like(params[0]), -torch.ones_like(params[1]), params[2]]  # |g * w| = |g|
    gen = torch.Generator().manual_seed(54)
    for g in grads[:2]:
        idx = torch.randperm(g.numel(), generator=gen)[:50]
        g.view(-1)[idx] = 0.5 * (torch.randint(0, 2, (50,), generator=gen) * 2.0 - 1.0)
    above = sum(int((g.abs() > 0.5).sum()) for g in grads[:2])
    k = above + 50
    pd, thr = _cdr_case(params, grads, (k + 0.5) / N_CDR, check_k=k)
    assert float(thr) == 0.5
    assert sum(int((p.grad != 0).sum()) for p in pd[:2]) == above + 100


def test_cdr_select_16_distinct_values():
    """Products quantised to 16 distinct values: every radix pass lands in a crowded bin."""
    params, grads = _cdr_tensors(55)
    gen = torch.Generator().manual_seed(56)
    vals = 0.1 * torch.arange(1, 17, dtype=torch.float32)
    params = [torch.full_like(params[0], 2.0), torch.full_like(params[1], -0.5), params[2]]
    grads = [vals[torch.randint(0, 16, tuple(g.shape), generator=gen)] * (torch.randint(0, 2, tuple(g.shape),
             generator=gen) * 2.0 - 1.0) for g in grads[:2]] + [grads[2]]
    for ratio in (0.5, 0.05, 0.97):
        _cdr_case(params, [g.clone() for g in grads], ratio)


def test_cdr_select_table_cache_second_call():
    """A second call with new gradients written into the same storage reuses the cached pointer
    table: it must see the new values."""
    params, grads = _cdr_tensors(57)
    pd, _ = _cdr_case(params, grads, 0.8)
    ptrs = [p.grad.data_ptr() for p in pd]
    _, grads2 = _cdr_tensors(58)
    for p, g in zip(pd, grads2):
        p.grad.copy_(g.to(DEV))
    assert ptrs == [p.grad.data_ptr() for p in pd]
    _cdr_call(pd, params, grads2, 0.3)
