"""fp64 reference of the LAMB step (csrc/optim.hip: mt_lamb_moments / lamb_trust / mt_lamb_update;
optim/fused.py: FusedLAMB), its first-order rounding-error bounds, and the lattice on which one step
is exact in fp32; shared by test_lamb_cpu.py, test_lamb_kernels_gpu.py and test_lamb_graph_gpu.py.

    g~ = grad_scale * g
    m  = b1 m + (1 - b1) g~            v = b2 v + (1 - b2) g~^2
    r  = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)     bc_i = 1 - b_i^t, or 1 with bias_correction=False
    u  = r + wd * w
    trust = |w| / |u|   if adapt and |w| > 0 and |u| > 0, else 1
    w -= lr * trust * u

The lattice: bias_correction=False, b1 = 1/2, b2 = 3/4, wd = 0, gradient entries 0 or +-2^s and
eps = 2^(s-1).  From zero moments m = g/2, sqrt(v) = |g|/2, the denominator is 2^s (or 2^(s-1) where
g = 0) and r is 0 or +-1/2; from the carried state m = g/2, v = g^2/4 a next gradient g/2 of the
same sign gives the same m, v and r.  With 4^a non-zero gradient entries |u| = 2^(a-1); with w from
lars_ref's lattice |w| is a power of two; with a power-of-two lr every intermediate is an fp32
number, whatever the order of any reduction -- but not whichever elements, chunks or tensors enter it.
"""
import torch

from tests import lars_ref as L

F64 = torch.float64
CHUNK = L.CHUNK
U = 2.0 ** -24
f64 = L.f64


def _fp32(x):
    """The fp64 tensor or number is an fp32 number."""
    x = torch.as_tensor(x, dtype=F64)
    return bool(torch.equal(x.float().double(), x))


def bias_corrections(betas, t, bias_correction=True):
    if not bias_correction:
        return 1.0, 1.0
    return 1.0 - betas[0] ** t, 1.0 - betas[1] ** t


def lamb_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-6, wd=0.0, grad_scale=1.0, bias_correction=True,
              adapt=True, trust=None, drop_w=None, drop_u=None, norm_without_wd=False, exact=False):
    """One LAMB update in fp64 -> dict(p, m, v, u, r, trust, wn, un).  The hyper-parameters stay the
    caller's doubles.  ``trust``: force that ratio; ``drop_w`` / ``drop_u``: leave a chunk out of a
    norm; ``norm_without_wd``: take |u| without the wd * w term (all three only for the sensitivity
    checks).  ``exact``: assert that every intermediate is an fp32 number (the lattice's promise)."""
    b1, b2 = betas
    bc1, bc2 = bias_corrections(betas, t, bias_correction)
    p, m, v = f64(p), f64(m), f64(v)
    gs = f64(g) * grad_scale
    a, c = (1.0 - b1) * gs, (1.0 - b2) * (gs * gs)
    m2, v2 = b1 * m + a, b2 * v + c
    s = v2.sqrt()
    denom = s / bc2 ** 0.5 + eps
    mh = m2 / bc1
    r = mh / denom
    u = r + wd * p
    wn = L.sumsq(p, drop_w) ** 0.5
    un = L.sumsq(r if norm_without_wd else u, drop_u) ** 0.5
    if trust is None:
        trust = wn / un if (adapt and wn > 0 and un > 0) else 1.0
    lt = lr * trust
    p2 = p - lt * u
    if exact:
        for name, x in (("g~", gs), ("(1-b1) g~", a), ("g~^2", gs * gs), ("(1-b2) g~^2", c), ("m", m2), ("v", v2),
                        ("sqrt v", s), ("denominator", denom), ("m / bc1", mh), ("r", r), ("u", u), ("|w|", wn),
                        ("|u|", un), ("trust", trust), ("lr trust", lt), ("lr trust u", lt * u), ("w", p2)):
            assert _fp32(x), f"the lattice step is not exact in fp32 at {name}"
    return dict(p=p2, m=m2, v=v2, u=u, r=r, trust=trust, wn=wn, un=un)


# ----------------------------------------------------------------------------- rounding-error bounds
# First-order bounds of the kernels' chain of fp32 operations, in absolute terms per element (u =
# 2^-24 per rounding of an operation or of a hyper-parameter to fp32; one rounding per fmaf):
#
#   g~  = gin * gs                          1 |g~|
#   a   = omb1 * g~                         3 |a|            (omb1, g~, the product)
#   m'  = fmaf(b1, m, a)                    1 |b1 m| + 3 |a| + 1 |m'|
#   gg  = g~ * g~ ; c = omb2 * gg           3 gg ; 5 c
#   v'  = fmaf(b2, v, c)                    1 b2 v + 5 c + 1 v'
#   s   = sqrt(v')                          e(v') / (2 s) + 1 s
#   bc1, bc2 = -expm1f(t * lb)              4 relative (lb 1, the product 1, expm1f 1 ulp = 2; the
#                                           argument's error is not amplified: x e^x / (e^x - 1) <= 1)
#   rbc2 = 1 / sqrtf(bc2)                   4 relative (2 + 1 + 1);  0 for both without bias correction
#   den = fmaf(s, rbc2, eps)                rbc2 e(s) + 4 s rbc2 + 1 eps + 1 den
#   mh  = m' / bc1                          e(m') / bc1 + 5 |mh|
#   r   = mh / den                          e(mh) / den + |r| e(den) / den + 1 |r|
#   u   = fmaf(wd, w, r)                    e(r) + 1 |wd w| + 1 |u|          (wd = 0: u = r)
#   w'  = fmaf(-(lr * trust), u, w)         lt e(u) + 2 |lt u| + 1 |w'|      (lr as fp32, the product)
#
# A no-cancellation element (every sum's terms of one sign) has e(u) <= 20 |u|: m' 4, v' 6, s 4, den 9,
# mh 9, r 19, u 20.  Mixed signs in m' and u amplify that by (|b1 m| + |a|) / |m'| and (|r| + |wd w|) /
# |u|.  KAPPA_CAP = 40 allows the tensor-wide (2-norm) amplification a factor 2; the tests assert, from
# this oracle alone, that their inputs stay below it.
#
# The trust ratio (as the 34 u of LARS): a chunk partial is within 25 u of the sum of squares of the
# fp32 values it adds (16 fused multiply-adds in series, 6 butterfly levels, 3 additions of block_sum);
# the merge is fp64; sqrt halves (12.5 u) and one rounding to fp32 gives 13.5 u for |w| and, with the
# elements' own error kappa, 13.5 + kappa for |u|; one rounding for the division:
#   K_TRUST = 13.5 + 13.5 + KAPPA_CAP + 1 = 68,  K u = 4.05e-6.
SLACK = 1.001     # second-order terms
KAPPA_CAP = 40.0
K_TRUST = 13.5 + 13.5 + KAPPA_CAP + 1.0


def lamb_bounds(p, g, m, v, t, lr, trust, betas=(0.9, 0.999), eps=1e-6, wd=0.0, grad_scale=1.0,
                bias_correction=True, unfused=False):
    """Per-element absolute error bounds dict(m, v, u, p) of the fp32 chain above against lamb_step
    (``trust`` forced to the same value in both), and kappa = |e(u)|_2 / (u |u|_2).  ``unfused``: the
    CPU path's torch ops round the product inside each of the five fused multiply-adds on its own
    (b1 m, b2 v, s rbc2, wd w, lt u): one more u on that term."""
    x = 1.0 if unfused else 0.0
    b1, b2 = betas
    bc1, bc2 = bias_corrections(betas, t, bias_correction)
    kb = 4.0 if bias_correction else 0.0
    p, m, v = f64(p), f64(m), f64(v)
    gs = f64(g) * grad_scale
    a, c = (1.0 - b1) * gs, (1.0 - b2) * (gs * gs)
    m2, v2 = b1 * m + a, b2 * v + c
    e_m = (1 + x) * (b1 * m).abs() + 3 * a.abs() + m2.abs()
    e_v = (1 + x) * b2 * v + 5 * c + v2
    s = v2.sqrt()
    e_s = torch.where(s > 0, e_v / (2 * s).clamp_min(1e-300), torch.zeros_like(s)) + s
    rbc2 = 1.0 / bc2 ** 0.5
    den = s * rbc2 + eps
    e_den = rbc2 * e_s + (kb + x) * s * rbc2 + eps + den
    mh = m2 / bc1
    e_mh = e_m / bc1 + (kb + 1) * mh.abs()
    r = mh / den
    e_r = e_mh / den + r.abs() * e_den / den + r.abs()
    u = r + wd * p
    e_u = e_r + ((1 + x) * (wd * p).abs() + u.abs() if wd != 0 else 0.0)
    lt = abs(lr * trust)
    p2 = p - lr * trust * u
    e_p = lt * e_u + (2 + x) * (lt * u).abs() + p2.abs()
    un = float(u.norm())
    kappa = float(e_u.norm()) / un if un > 0 else 0.0
    k = U * SLACK
    return dict(m=k * e_m, v=k * e_v, u=k * e_u, p=k * e_p, kappa=kappa)


def check_random_steps(opt, ps, sizes, grads_of, steps, sync=lambda: None, unfused=False, late=None):
    """``steps`` steps of ``opt`` (one parameter group) against the oracle, teacher-forced: every step
    starts from the optimizer's own w, m, v, and its own trust ratio is fed to the oracle for the
    per-element bounds on w, m and v; the trust ratio itself must be within K_TRUST u of the oracle's.
    ``late``: index of a parameter whose first gradient arrives at step 3.
    -> the worst (trust error in u, per-element error / its bound, kappa)."""
    def cpu(t):
        return t.detach().cpu().clone()

    h = opt.param_groups[0]
    worst = dict(trust=0.0, elem=0.0, kappa=0.0)
    for step in range(1, steps + 1):
        gs = grads_of(step)
        before = []
        for i, (p, g) in enumerate(zip(ps, gs)):
            st = opt.state.get(p, {})
            z = torch.zeros(p.numel())
            before.append((cpu(p), cpu(st["exp_avg"]) if "exp_avg" in st else z,
                           cpu(st["exp_avg_sq"]) if "exp_avg_sq" in st else z))
            p.grad = None if (i == late and step < 3) else g.to(p.device)
        opt.step()
        sync()
        for i, (p, g) in enumerate(zip(ps, gs)):
            name = (step, sizes[i])
            w0, m0, v0 = before[i]
            if p.grad is None:
                assert torch.equal(cpu(p), w0) and "exp_avg" not in opt.state[p], name
                continue
            hy = (opt.state[p]["step"], h["lr"], h["betas"], h["eps"], h["weight_decay"], h["grad_scale"],
                  h["bias_correction"])
            assert hy[0] == (step - 2 if i == late else step), name
            ref = lamb_step(w0, g, m0, v0, *hy)
            got_t = float(opt.trust_of(p))
            if h["adapt"]:
                assert ref["trust"] != 1.0, name
                et = abs(got_t - ref["trust"]) / ref["trust"] / U
            else:
                assert got_t == 1.0, name
                et = 0.0
            forced = lamb_step(w0, g, m0, v0, *hy, trust=got_t)
            bnd = lamb_bounds(w0, g, m0, v0, hy[0], hy[1], got_t, *hy[2:], unfused=unfused)
            if h["adapt"]:   # the inputs keep the trust bound's precondition (no norm without adapt)
                assert bnd["kappa"] <= KAPPA_CAP, (name, bnd["kappa"])
            ee = 0.0
            for key, got in (("p", p), ("m", opt.state[p]["exp_avg"]), ("v", opt.state[p]["exp_avg_sq"])):
                err = (f64(got) - forced[key]).abs()
                rel = float((err / bnd[key].clamp_min(1e-300)).max())
                assert bool((err <= bnd[key]).all()), (name, key, rel)
                ee = max(ee, rel)
            assert et <= K_TRUST, (name, et)
            worst = dict(trust=max(worst["trust"], et), elem=max(worst["elem"], ee),
                         kappa=max(worst["kappa"], bnd["kappa"]))
    return worst


# ----------------------------------------------------------------------------- the lattice
S_EXP = -4                      # gradient entries 0 or +-2^S_EXP
EXACT_HYPER = dict(lr=2.0 ** -3, betas=(0.5, 0.75), eps=2.0 ** (S_EXP - 1), weight_decay=0.0, bias_correction=False)
EDGE_SIZES = [1, 3, 4, 4095, 4096, 4097, 2 * CHUNK + 5]
BIG = 300 * CHUNK + 5           # 301 chunks: more than 256 partials for one tensor
SMALL_SIZES = [5 + 3 * i for i in range(70)]
EXACT_SIZES = EDGE_SIZES + [BIG] + SMALL_SIZES
EXACT_LATE = 2                  # index of the parameter whose first gradient arrives at step 3


def grad_count_exp(n):
    """a: the largest 4^a <= n (4^10 for BIG) -- the number of non-zero gradient entries."""
    a = 0
    while 4 ** (a + 1) <= n and a < 10:
        a += 1
    return a


def exact_trust_exp(i):
    """log2 of tensor i's trust ratio: a different power of two for every tensor."""
    return i - 38


def exact_draw(i, n, gen, grad_exp=S_EXP):
    """(w, g) of tensor i on the lattice (new positions and signs at every call, the same norms):
    4^a entries of +-2^grad_exp in g, so |u| = 2^(a-1), and |w| = 2^(exact_trust_exp(i) + a - 1)."""
    a = grad_count_exp(n)
    must = L.edge_positions(n)
    counts = (2 ** 20, 0, 10) if n == BIG else None
    w = L.pow2_lattice(n, exact_trust_exp(i) + a - 1, must, gen, counts)
    g = L.lattice(n, 4 ** a, 0, grad_exp, must, gen)
    return w, g


def check_exact_steps(make_opt, device, sizes=EXACT_SIZES, sync=lambda: None):
    """Three steps of ``make_opt(params)`` on the lattice against the oracle: torch.equal on w, m, v
    and the trust ratios.  Every step starts from values written here: step 1 from zero moments and a
    gradient g; steps 2 and 3 from the carried state m = g/2, v = g^2/4 of a fresh g and the next
    gradient g/2.  Parameter EXACT_LATE gets its first gradient (zero moments) at step 3."""
    gen = torch.Generator().manual_seed(4242)
    ps = [torch.zeros(n, device=device).requires_grad_(True) for n in sizes]
    opt = make_opt(ps)
    h = opt.param_groups[0]
    trusts = set()
    for step in (1, 2, 3):
        cases = []
        for i, (p, n) in enumerate(zip(ps, sizes)):
            w, g = exact_draw(i, n, gen)
            late = i == EXACT_LATE and step < 3
            carried = step > 1 and i != EXACT_LATE
            m0, v0 = (g / 2, g * g / 4) if carried else (torch.zeros(n), torch.zeros(n))
            gin = g / 2 if carried else g
            p.data.copy_(w)
            p.grad = None if late else gin.to(device)
            if carried:
                opt.state[p]["exp_avg"].copy_(m0)
                opt.state[p]["exp_avg_sq"].copy_(v0)
            cases.append((w, gin, m0, v0, late))
        opt.step()
        sync()
        for i, (p, (w, gin, m0, v0, late)) in enumerate(zip(ps, cases)):
            name = (step, sizes[i])
            if late:
                assert torch.equal(p.detach().cpu(), w) and "exp_avg" not in opt.state[p], name
                continue
            t = opt.state[p]["step"]
            assert t == (1 if i == EXACT_LATE else step), name
            ref = lamb_step(w, gin, m0, v0, t, h["lr"], h["betas"], h["eps"], h["weight_decay"], h["grad_scale"],
                            h["bias_correction"], exact=True)
            assert ref["trust"] == 2.0 ** exact_trust_exp(i), name   # the lattice delivers the norms it promises
            trusts.add(ref["trust"])
            assert float(opt.trust_of(p)) == ref["trust"], (name, float(opt.trust_of(p)), ref["trust"])
            assert torch.equal(opt.state[p]["exp_avg"].cpu(), ref["m"].float()), name
            assert torch.equal(opt.state[p]["exp_avg_sq"].cpu(), ref["v"].float()), name
            assert torch.equal(p.detach().cpu(), ref["p"].float()), name
            assert not torch.equal(ref["p"].float(), w), name
    assert len(trusts) == len(sizes)
