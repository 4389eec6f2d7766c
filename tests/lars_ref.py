"""fp64 reference of the LARS step (csrc/optim.hip: mt_norm2 / lars_trust / mt_lars kernels;
optim/fused.py: FusedLARS) and the integer lattice on which that step is exact in fp32, shared by
test_lars_cpu.py, test_lars_kernels_gpu.py and test_lars_graph_gpu.py.

    g~    = grad_scale * g
    trust = eta * |w| / (|g~| + wd * |w| + eps)    if adapt and |w| > 0 and |g~| > 0, else 1
    d     = trust * (g~ + wd * w)
    buf   = d  (first gradient)  |  momentum * buf + (1 - dampening) * d
    w    -= lr * (d + momentum * buf  if nesterov else  buf)

The lattice: tensors whose entries are 0, +-1, +-2 times one power of two, with a prescribed number
of +-1 and +-2 entries at prescribed positions.  Their sum of squares (ones + 4 twos) 4^s is an
integer times a power of four, summed exactly by fp32 in any order; with ones + 4 twos = 4^a the norm
is exactly 2^(a + s).  With power-of-two hyper-parameters every intermediate of the step is then an
fp32 number, and the result is independent of the order of any reduction -- but not of which
elements, chunks or tensors enter it.
"""
import torch

F64 = torch.float64
CHUNK = 4096


def f64(t):
    return t.detach().to("cpu").to(F64)


def sumsq(x, drop_chunk=None):
    """Sum of squares in fp64; ``drop_chunk``: leave out that 4096-element chunk (sensitivity)."""
    x = f64(x).reshape(-1)
    if drop_chunk is not None:
        x = x.clone()
        x[drop_chunk * CHUNK:(drop_chunk + 1) * CHUNK] = 0.0
    return float((x * x).sum())


def trust_ratio(p, g, wd=0.0, grad_scale=1.0, eta=1e-3, eps=1e-8, adapt=True, drop_w=None, drop_g=None):
    if not adapt:
        return 1.0
    wn = sumsq(p, drop_w) ** 0.5
    gn = abs(grad_scale) * sumsq(g, drop_g) ** 0.5
    if wn > 0 and gn > 0:
        return eta * wn / (gn + wd * wn + eps)
    return 1.0


def lars_step(p, g, buf, first, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, grad_scale=1.0,
              eta=1e-3, eps=1e-8, adapt=True, trust=None, drop_w=None, drop_g=None):
    """One LARS update in fp64 -> (new p, new momentum buffer or None, trust).  The hyper-parameters
    stay the caller's doubles.  ``trust``: force that ratio; ``drop_w`` / ``drop_g``: leave a chunk
    out of a norm (both only for the sensitivity checks)."""
    if trust is None:
        trust = trust_ratio(p, g, wd, grad_scale, eta, eps, adapt, drop_w, drop_g)
    p, g = f64(p), f64(g) * grad_scale
    d = trust * (g + wd * p)
    if momentum != 0:
        buf = d.clone() if first else momentum * f64(buf) + (1.0 - dampening) * d
        d = d + momentum * buf if nesterov else buf
    else:
        buf = None
    return p - lr * d, buf, trust


# ----------------------------------------------------------------------------- the lattice
def lattice(n, ones, twos, scale_exp=0, must=(), gen=None):
    """fp32 [n]: ``ones`` entries of +-2^s and ``twos`` entries of +-2^(s+1) (s = scale_exp), zero
    elsewhere; sum of squares (ones + 4 twos) 4^s.  The positions in ``must`` are non-zero; the
    others and the signs come from ``gen``."""
    k = ones + twos
    assert 0 < k <= n and len(set(must)) == len(must) <= k and all(0 <= m < n for m in must)
    gen = gen or torch.Generator().manual_seed(0)
    taken = torch.zeros(n, dtype=torch.bool)
    must = torch.tensor(list(must), dtype=torch.int64)
    taken[must] = True
    free = (~taken).nonzero().reshape(-1)
    pick = free[torch.randperm(free.numel(), generator=gen)[:k - must.numel()]]
    pos = torch.cat([must, pick])
    pos = pos[torch.randperm(k, generator=gen)]  # which positions carry the twos is random too
    mag = torch.cat([torch.ones(ones, dtype=F64), torch.full((twos,), 2.0, dtype=F64)])
    sign = torch.randint(0, 2, (k,), generator=gen).to(F64) * 2.0 - 1.0
    out = torch.zeros(n, dtype=F64)
    out[pos] = mag * sign * 2.0 ** scale_exp
    out32 = out.float()
    assert torch.equal(out32.double(), out)
    return out32


def pow2_counts(n):
    """(ones, twos, a): the largest 4^a = ones + 4 twos that fits into n entries, with both
    magnitudes present when 4^a >= 8."""
    a = 0
    while True:
        q = 4 ** (a + 1)
        need = q if q < 8 else q // 2 + q // 8
        if need > n:
            break
        a += 1
    q = 4 ** a
    if q < 8:
        return q, 0, a
    return q // 2, q // 8, a


def pow2_lattice(n, k, must=(), gen=None, counts=None):
    """fp32 [n] on the lattice with norm exactly 2^k."""
    ones, twos, a = counts or pow2_counts(n)
    assert ones + 4 * twos == 4 ** a
    return lattice(n, ones, twos, k - a, must, gen)


def edge_positions(n):
    """The positions whose loss changes a norm: the last element and, for a tensor of more than
    one chunk, the first element of the second chunk."""
    must = [n - 1]
    if n > CHUNK and CHUNK != n - 1:
        must.append(CHUNK)
    return must


def is_fp32(t):
    """Every value of the fp64 tensor is an fp32 number."""
    return bool(torch.equal(t.float().double(), t))


# ----------------------------------------------------------------------------- the exact cases
# powers of two throughout, eps = 0: the step is exact in fp32 on the lattice
EXACT_HYPER = dict(lr=2.0 ** -2, momentum=0.5, grad_scale=0.5, eta=2.0 ** -3, eps=0.0)
EDGE_SIZES = [1, 3, 4095, 4096, 4097, 8195]
BIG = 300 * CHUNK + 5           # more than 256 chunk partials for one tensor
SMALL_SIZES = [5 + 3 * i for i in range(70)]   # 5 .. 212, distinct from each other and the edge sizes
EXACT_SIZES = EDGE_SIZES + [BIG] + SMALL_SIZES
EXACT_LATE = 2                  # index of the parameter whose first gradient arrives at step 3


def exact_exponents(i):
    """(log2 |w|, log2 |g|) of tensor i: |w| = 2^c, |g| = 2^-c with c distinct per tensor, so the
    trust ratio eta 2^(2c + 1) (grad_scale 1/2) is a different power of two for every tensor."""
    c = i - 38
    return c, -c


def exact_draw(i, n, gen):
    """(p, g) of tensor i on the lattice (new positions and signs at every call, the same norms)."""
    kw, kg = exact_exponents(i)
    counts = (2 ** 20, 0, 10) if n == BIG else None   # 2^20 entries of +-1
    must = edge_positions(n)
    return pow2_lattice(n, kw, must, gen, counts), pow2_lattice(n, kg, must, gen, counts)


def check_exact_steps(opt_cls, device, sizes=EXACT_SIZES, sync=lambda: None):
    """Three steps of ``opt_cls`` on the lattice against the oracle rounded once to fp32:
    torch.equal on parameters, momentum buffers and trust ratios.  p and g are re-drawn every step,
    the momentum is carried (step 1 is first=True, steps 2-3 are not); parameter EXACT_LATE gets its
    first gradient at step 3."""
    gen = torch.Generator().manual_seed(1234)
    ps = [torch.zeros(n, device=device).requires_grad_(True) for n in sizes]
    opt = opt_cls(ps, **EXACT_HYPER)
    h = opt.param_groups[0]
    trusts = set()
    for step in (1, 2, 3):
        draws = [exact_draw(i, n, gen) for i, n in enumerate(sizes)]
        bufs = []
        for i, (p, (pv, gv)) in enumerate(zip(ps, draws)):
            p.data.copy_(pv)
            p.grad = None if (i == EXACT_LATE and step < 3) else gv.to(device)
            b = opt.state[p].get("momentum_buffer")
            bufs.append(None if b is None else b.detach().cpu().clone())
        opt.step()
        sync()
        for i, (p, (pv, gv)) in enumerate(zip(ps, draws)):
            name = (step, sizes[i])
            if p.grad is None:
                assert torch.equal(p.detach().cpu(), pv) and "momentum_buffer" not in opt.state[p], name
                continue
            first = bufs[i] is None
            assert first == (step == (3 if i == EXACT_LATE else 1)), name
            ref_p, ref_buf, ref_t = lars_step(pv, gv, bufs[i], first, h["lr"], h["momentum"], h["dampening"],
                                              h["weight_decay"], h["nesterov"], h["grad_scale"], h["eta"], h["eps"])
            kw, kg = exact_exponents(i)
            assert ref_t == h["eta"] * 2.0 ** (kw - kg + 1), name   # the lattice delivers the norms it promises
            assert is_fp32(ref_p) and is_fp32(ref_buf), name      # the oracle's result is an fp32 number
            trusts.add(ref_t)
            assert float(opt.trust_of(p)) == ref_t, (name, float(opt.trust_of(p)), ref_t)
            assert torch.equal(opt.state[p]["momentum_buffer"].cpu(), ref_buf.float()), name
            assert torch.equal(p.detach().cpu(), ref_p.float()), name
    assert len(trusts) == len(sizes)


def check_exact_wd(opt_cls, device, sync=lambda: None):
    """Weight decay in the denominator: |g~| = 48, |w| = 64, wd = 1/4 give 48 + 16 = 64, trust = eta."""
    gen = torch.Generator().manual_seed(4321)
    hyper = dict(EXACT_HYPER, weight_decay=0.25)
    cases = [(4097, (2048, 512, 0), (1152, 288, 1)), (5, (4, 0, 5), (1, 2, 5))]
    ps = [torch.zeros(n, device=device).requires_grad_(True) for n, _, _ in cases]
    opt = opt_cls(ps, **hyper)
    bufs = [None, None]
    for step in (1, 2):
        draws = []
        for p, (n, cw, cg) in zip(ps, cases):
            pv = lattice(n, cw[0], cw[1], cw[2], edge_positions(n), gen)
            gv = lattice(n, cg[0], cg[1], cg[2], edge_positions(n), gen)
            assert sumsq(pv) == 64.0 ** 2 and sumsq(gv) == 96.0 ** 2
            p.data.copy_(pv)
            p.grad = gv.to(device)
            draws.append((pv, gv))
        opt.step()
        sync()
        for i, (p, (pv, gv)) in enumerate(zip(ps, draws)):
            ref_p, ref_buf, ref_t = lars_step(pv, gv, bufs[i], step == 1, hyper["lr"], hyper["momentum"], 0.0, 0.25,
                                              False, hyper["grad_scale"], hyper["eta"], 0.0)
            assert ref_t == hyper["eta"] and is_fp32(ref_p) and is_fp32(ref_buf)
            assert float(opt.trust_of(p)) == ref_t, (step, i)
            assert torch.equal(opt.state[p]["momentum_buffer"].cpu(), ref_buf.float()), (step, i)
            assert torch.equal(p.detach().cpu(), ref_p.float()), (step, i)
            bufs[i] = ref_buf.float()
