"""fp64 oracle for the BatchNorm, pooling and channel-scale kernels (helper module, not collected).

The references are written from the definitions -- the textbook batch-norm forward and backward,
"first maximum in window order" for the max pool, plain means for the average pools -- and not from
ops/_ref.py, which mirrors the kernels' own formulas and doubles as the CPU path.

Exact problems (the lattice of tests/exact_oracle.py carried over to this family): small-integer
bf16 ``x`` / ``dy`` / ``res``, power-of-two ``scale`` / ``invstd`` / gate, integer ``shift`` /
``mean`` and, for the training backward, a power-of-two row count.  Every intermediate of the
kernel's formula is then an fp32 number, so the output is ONE bf16 rounding of an exact number
whatever the summation order or the FMA contraction, and the comparison is ``torch.equal``.  The
builders assert their preconditions (fp32 round trips, shares of rounded / tied outputs, share of
``z == 0``, share of tied pooling windows) on the reference alone.

Statistics are not a lattice (Welford merges round): ``stat_bounds`` derives per-channel bounds
from the length of the dependent fp32 chain of each route.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

from tests.exact_oracle import (BF16, F32, LEAKY_SLOPE, _seed, assert_exact, bf16_tie, bf16_trunc,  # noqa: F401
                                bf16_ulp, int_vector, lattice, lattice_shares, mismatch_report, pow2_scales,
                                rounded)

U32 = 2.0 ** -24  # unit roundoff of fp32
MIN_SHARE_ELEMS = 2048  # problems of at least this many elements assert their precondition shares themselves
ACTS = (0, 1, 2)
NONDIV_C = (24, 72, 320, 1000, 1032, 2040)  # 256 % (C/8) != 0: idle row slots, ragged finalize groups
BN_C = (8, 24, 72, 320, 1000, 1032, 2040, 2048)


def rpi_of(C):
    """rows per pass of a 256-thread workgroup (RowTile): 256 / (C/8) row slots, the rest idle"""
    return 256 // (C // 8)


def fp32_exact(t):
    t = t.double()
    return bool(torch.equal(t.float().double(), t))


def need_fp32(**named):
    for k, v in named.items():
        assert fp32_exact(v), f"intermediate {k} is not an fp32 number"


# ----------------------------------------------------------------------------- definitions (fp64)
def act_f(z, act, slope):
    if act == 1:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == 2:
        return torch.where(z >= 0, z, z * slope)
    return z


def act_d(z, act, slope):
    """act'(z): ReLU is 0 AT z == 0 (and at -0.0), leaky ReLU is 1 at z == 0 (and at -0.0)"""
    one = torch.ones_like(z)
    if act == 1:
        return torch.where(z > 0, one, torch.zeros_like(z))
    if act == 2:
        return torch.where(z >= 0, one, one * slope)
    return one


def mask_bytes(active):
    """bool [..., C] -> uint8 [..., C/8], bit e of byte c = channel 8c + e"""
    a = active.reshape(*active.shape[:-1], active.shape[-1] // 8, 8).to(torch.int32)
    w = (1 << torch.arange(8, dtype=torch.int32))
    return (a * w).sum(-1).to(torch.uint8)


def bn_z(x, scale, shift, res=None, rscale=None, rshift=None):
    z = x.double() * scale.double() + shift.double()
    if res is not None:
        r = res.double()
        if rscale is not None:
            r = r * rscale.double() + rshift.double()
        z = z + r
    return z


def bn_bwd_textbook(dy, xv, z, mean, invstd, scale, act, slope, count=None):
    """dz = dy act'(z); s1 = sum dz; s2 = sum dz xhat; dx = scale (dz - s1/M - xhat s2/M)
    (count None: eval / frozen statistics, dx = scale dz)"""
    dz = dy.double() * act_d(z, act, slope)
    xhat = (xv.double() - mean.double()) * invstd.double()
    s1, s2 = dz.sum(0), (dz * xhat).sum(0)
    if count is None:
        return dz, s1, s2, scale.double() * dz
    return dz, s1, s2, scale.double() * (dz - s1 / count - xhat * s2 / count)


def stats64(x):
    """per-channel (n, mean, M2) of [M, C] in fp64"""
    x = x.double()
    mu = x.mean(0)
    return float(x.shape[0]), mu, ((x - mu) ** 2).sum(0)


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def maxpool_first(v, k, s, p):
    """[N,H,W,C] fp64 -> (max, window index kh*k + kw of the FIRST maximum in window order, share of
    windows whose maximum is tied).  Taps outside the image do not take part."""
    N, H, W, C = v.shape
    Ho, Wo = out_hw(H, W, k, s, p)
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=torch.float64)
    idx = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8)
    hits = torch.zeros((N, Ho, Wo, C), dtype=torch.int32)
    ho, wo = torch.arange(Ho), torch.arange(Wo)
    taps = []
    for kh in range(k):
        for kw in range(k):
            hi, wi = ho * s - p + kh, wo * s - p + kw
            ok = ((hi >= 0) & (hi < H))[:, None] & ((wi >= 0) & (wi < W))[None, :]
            cand = v[:, hi.clamp(0, H - 1)][:, :, wi.clamp(0, W - 1)]
            cand = torch.where(ok[None, :, :, None], cand, torch.full_like(cand, -math.inf))
            taps.append(cand)
            take = cand > best
            best = torch.where(take, cand, best)
            idx = torch.where(take, torch.full_like(idx, kh * k + kw), idx)
    for cand in taps:
        hits += (cand == best).int()
    return best, idx, (hits > 1).double().mean().item()


def maxpool_bwd_exact(dy, idx, H, W, k, s, p):
    """scatter of dy to the argmax pixel of its window, summed in fp64"""
    N, Ho, Wo, C = dy.shape
    dx = torch.zeros((N, H, W, C), dtype=torch.float64)
    n, ho, wo, c = torch.meshgrid(torch.arange(N), torch.arange(Ho), torch.arange(Wo), torch.arange(C), indexing="ij")
    kh, kw = idx.long() // k, idx.long() % k
    hi, wi = ho * s - p + kh, wo * s - p + kw
    assert bool(((hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)).all()), "argmax outside the image"
    dx.index_put_((n, hi, wi, c), dy.double(), accumulate=True)
    return dx


def ad_cell(o, I, O):
    return (o * I) // O, -((-(o + 1) * I) // O)  # [floor(o I / O), ceil((o+1) I / O))


def adaptive_avg_sum(x, OH, OW):
    """-> (window sums [N,OH,OW,C] fp64, window sizes [OH,OW])"""
    N, H, W, C = x.shape
    s = torch.zeros((N, OH, OW, C), dtype=torch.float64)
    cnt = torch.zeros((OH, OW), dtype=torch.float64)
    for oh in range(OH):
        h0, h1 = ad_cell(oh, H, OH)
        for ow in range(OW):
            w0, w1 = ad_cell(ow, W, OW)
            s[:, oh, ow] = x[:, h0:h1, w0:w1].double().sum((1, 2))
            cnt[oh, ow] = (h1 - h0) * (w1 - w0)
    return s, cnt


def adaptive_avg_bwd_terms(dy, H, W):
    """per input pixel the list of (dy cell, window size) it belongs to -> [(mask-free) (oh, ow, cnt)]"""
    N, OH, OW, C = dy.shape
    cells = [[[] for _ in range(W)] for _ in range(H)]
    for oh in range(OH):
        h0, h1 = ad_cell(oh, H, OH)
        for ow in range(OW):
            w0, w1 = ad_cell(ow, W, OW)
            for h in range(h0, h1):
                for w in range(w0, w1):
                    cells[h][w].append((oh, ow, (h1 - h0) * (w1 - w0)))
    return cells


def f32_recip(n):
    """fp32(1 / n) as fp64: the reciprocal the kernels multiply by"""
    return torch.tensor(1.0, dtype=F32).div(torch.tensor(float(n), dtype=F32)).double()


def two_roundings(sum_exact, n):
    """A mean taken as ``bf16(fp32(sum) * fp32(1/n))``: with n not a power of two the product rounds to
    fp32 before the bf16 store.  -> (the kernel's bit-exact output, the one-rounding value sum / n, the
    per-element bound |out - sum / n| that two roundings imply).  ``n`` a number or a tensor
    broadcastable to the sums; the sums themselves are lattice integers fp32 holds."""
    need_fp32(sum=sum_exact)
    nt = torch.as_tensor(n, dtype=torch.float64)
    inv = torch.ones_like(nt).float().div(nt.float()).double()
    prod = (sum_exact.double() * inv).float()  # fp64 product of two fp32 numbers is exact; one rounding to fp32
    got = prod.to(BF16)
    one = sum_exact.double() / nt
    # fp32(1/n) is within u of 1/n relatively, the fp32 product within u again, the bf16 store within
    # half a bf16 ulp of the product: |out - sum/n| <= 2 u |sum/n| (1 + u) + ulp_bf16(prod) / 2
    bound = 2.0 * U32 * one.abs() * (1 + U32) + 0.5 * bf16_ulp(prod.double())
    return got, one, bound


# ----------------------------------------------------------------------------- exact BN problems
def _plant(flags, value, into):
    return torch.where(flags, value.to(into.dtype), into)


@functools.lru_cache(maxsize=None)
def bn_base(C, M, small=False):
    """inputs of one [M, C] BN problem, shared by every (act, residual) combination.

    ``small``: the ranges of the exact training backward (x, dy within +-7, mean within +-2): its
    intermediates carry the products S2 (x - mean) / M, which must stay fp32 numbers.
    About 30 % of the positions are candidates, planted so that z == 0 exactly: ``x = -shift / scale`` where that is
    a lattice integer (``x = +-0.0`` in the channels whose shift is +-0.0), or ``res = -(x scale +
    shift)`` for the residual forms; channels 0 mod 8 carry ``shift = -0.0``, so ``x = -0.0`` there gives
    ``z = -0.0 * scale + -0.0 = -0.0``."""
    key = ("bn", C, M, small)
    mx = 7 if small else 127
    x = lattice((M, C), -mx, mx, _seed("x", key))
    dy = lattice((M, C), -7, 7, _seed("dy", key))
    res = lattice((M, C), -100, 100, _seed("r", key))
    scale = pow2_scales(C, _seed("sc", key), exps=(-1, 0, 1) if small else (-1, 2, 3, 3))
    shift = int_vector(C, -3 if small else -64, 3 if small else 64, _seed("sh", key))
    shift[torch.arange(C) % 4 == 0] = 0.0
    shift[torch.arange(C) % 8 == 0] = -0.0
    rscale = pow2_scales(C, _seed("rsc", key), exps=(0, 1))
    rshift = int_vector(C, -8, 8, _seed("rsh", key))
    mean = int_vector(C, -2, 2, _seed("mu", key))
    invstd = pow2_scales(C, _seed("is", key), exps=(-1, 0, 1)).abs()
    g = torch.Generator().manual_seed(_seed("plant", key))
    plant = torch.rand((M, C), generator=g) < 0.3
    neg0 = torch.rand((M, C), generator=g) < 0.5
    # no residual: x = -shift / scale
    x0 = -(shift.double() / scale.double()).expand(M, C)
    ok = plant & (x0 == x0.round()) & (x0.abs() <= mx)
    zero_sh = (shift == 0).expand(M, C)
    x0 = torch.where(zero_sh & neg0, torch.full_like(x0, -0.0), torch.where(zero_sh, torch.zeros_like(x0), x0))
    xz = _plant(ok, x0, x)
    # residual forms: res = -(x scale + shift), res2 = (-(x scale + shift) - rshift) / rscale
    r0 = -(x.double() * scale.double() + shift.double())
    okr = plant & (r0 == r0.round()) & (r0.abs() <= 256)
    rz = _plant(okr, r0, res)
    r2 = (r0 - rshift.double()) / rscale.double()
    okr2 = plant & (r2 == r2.round()) & (r2.abs() <= 256)
    rz2 = _plant(okr2, r2, res)
    return SimpleNamespace(C=C, M=M, x=xz, x_res=x, dy=dy, res=rz, res2=rz2, scale=scale, shift=shift, rscale=rscale,
                           rshift=rshift, mean=mean, invstd=invstd, small=small)


def bn_case(b, act, res, slope=LEAKY_SLOPE, two=False, count=None, inv=False):
    """One exact case of the base problem ``b``: forward y / mask bytes, backward sums / dx / dres.

    ``two``: the residual is a raw BN input normalised on the fly (bn2_act_mask).  ``count``: rows of
    the training backward (None: eval statistics, dx = scale dz).  ``inv``: InplaceABN backward from
    the output -- ``x`` is read as y = act(z), z = act^-1(y), mean / invstd carry beta / 1/gamma."""
    x = b.x_res if res else b.x
    r = (b.res2 if two else b.res) if res else None
    if inv:
        assert act in (0, 2) and not res
        y_in = x.double()
        z = torch.where(y_in < 0, y_in / slope, y_in) if act == 2 else y_in
        xv = z
    else:
        z = bn_z(x, b.scale, b.shift, r, b.rscale if two else None, b.rshift if two else None)
        xv = x.double()
    need_fp32(z=z)
    y = act_f(z, act, slope)
    dz, s1, s2, dx = bn_bwd_textbook(b.dy, xv, z, b.mean, b.invstd, b.scale, act, slope, count)
    out = SimpleNamespace(b=b, act=act, has_res=res, x=x, res=r, z=z, y=y, want_y=rounded(y, BF16),
                          want_mask=mask_bytes(z > 0), dz=dz, want_dres=rounded(dz, BF16),
                          want_sums=rounded(torch.stack([s1, s2]), F32), dx=dx, want_dx=rounded(dx, BF16),
                          count=count, slope=slope)
    # the kernel's own formula, intermediate by intermediate: each must be an fp32 number
    need_fp32(dz=dz, s1=s1, s2=s2, s2raw=s2 / b.invstd.double())
    if count is not None:
        folded_check(dz, xv, s1, s2, b.scale, b.mean, b.invstd, count, dx)
    if z.numel() >= MIN_SHARE_ELEMS:
        # the shares, per problem and on the reference alone (a problem of a few rows cannot carry a
        # share; those are covered over their channel count's cases by check_bn_shares in the CPU test)
        check_bn_shares([out], "dx" if count is not None else "y")
    return out


def folded_check(dz, xv, s1, s2, scale, mean, invstd, count, dx):
    """the kernels' folded form dx = ca dz + cb x + cc, intermediate by intermediate"""
    sc, mu, is_ = scale.double(), mean.double(), invstd.double()
    a2, a3 = s1 / count, s2 / count * is_
    cb, cc = -sc * a3, -sc * a2 + sc * a3 * mu
    t1, t2 = sc * dz, cb * xv
    need_fp32(a2=a2, a3=a3, cb=cb, sca2=sc * a2, sca3=sc * a3, sca3mu=sc * a3 * mu, cc=cc, t1=t1, t2=t2,
              t12=t1 + t2, out=t1 + t2 + cc, xmu=xv - mu, dzxmu=dz * (xv - mu))
    assert torch.equal(t1 + t2 + cc, dx), "folded and textbook forms of dx differ in fp64"


def bn2_case(b):
    """both input gradients of act(BN(x) + BN_r(r)) from the masked gradient g = dy (bn2_bwd_elemt):
    r = the rows of x shifted by one, its BN's mean / invstd the main one's reversed"""
    M = float(b.M)
    r = b.x.roll(1, 0)
    rmean, rinvstd, rscale = b.mean.flip(0), b.invstd.flip(0), b.rscale
    z = torch.ones((b.M, b.C), dtype=torch.float64)
    dz, s1, s2, dx = bn_bwd_textbook(b.dy, b.x.double(), z, b.mean, b.invstd, b.scale, 0, 0.0, M)
    folded_check(dz, b.x.double(), s1, s2, b.scale, b.mean, b.invstd, M, dx)
    _, r1, r2, dr = bn_bwd_textbook(b.dy, r.double(), z, rmean, rinvstd, rscale, 0, 0.0, M)
    folded_check(dz, r.double(), r1, r2, rscale, rmean, rinvstd, M, dr)
    return SimpleNamespace(r=r, rmean=rmean, rinvstd=rinvstd, rscale=rscale, sums=rounded(torch.stack([s1, s2]), F32),
                           rsums=rounded(torch.stack([r1, r2]), F32), dx=dx, dr=dr, want_dx=rounded(dx, BF16),
                           want_dr=rounded(dr, BF16))


def shares(cases, field="y"):
    """(needs rounding, ties, z == 0, z == -0.0) over a list of cases"""
    v = torch.cat([getattr(c, field).reshape(-1) for c in cases])
    z = torch.cat([c.z.reshape(-1) for c in cases])
    norep, ties = lattice_shares(v)
    z0 = (z == 0).double().mean().item()
    zneg = ((z == 0) & torch.signbit(z)).double().mean().item()
    return norep, ties, z0, zneg


def check_bn_shares(cases, field="y", rounds=True):
    norep, ties, z0, zneg = shares(cases, field)
    assert z0 >= 0.05, f"only {z0:.1%} of the elements sit at z == 0"
    if rounds:
        assert norep >= 0.05, f"only {norep:.1%} of the outputs need rounding"
        assert ties >= 0.01, f"only {ties:.1%} of the outputs are ties"
    return norep, ties, z0, zneg


def bn_rows(C):
    """row counts of the elementwise cases: 1, rpi - 1, rpi, and 4 rpi g + 3 for grids of g = 1 and 3
    workgroups (each thread then runs the 4-deep loop once and the tail loop for three row slots)"""
    r = rpi_of(C)
    return sorted({1, max(1, r - 1), r, r + 1, 4 * r + 3, 12 * r + 3})


def bwd_rows(C):
    """power-of-two row counts of the exact training backward (1 / count exact)"""
    if C <= 72:
        return (64, 1024)  # 1024 rows: four passes of the 28 .. 256 row slots
    return (64, 256) if C <= 320 else (64,)


# ----------------------------------------------------------------------------- statistics
MERGE_OPS = 12  # dependent fp32 operations of one Welford.merge on the M2 chain (nt, d, f, d f, mean +=, d d, n, f, +, +=, slack 2 for a division that is not correctly rounded)


def stat_chain(route, **kw):
    """Length of the longest chain of dependent fp32 operations behind one channel's (mean, M2).

    raw     chan_welford_partial: L rows per thread x 3 operations (d, d d, +=), 6 to turn the shifted
            sums into (mean, M2), rpi slot merges; then merge_partials over P partials.
    direct  merge_slabs: ceil(R / 64) merges per row stream, 8 + 8 stream merges.
    split   bn_slab_partial: ceil(tps / 4) merges per wave + 3; then merge_partials over P splits.
    given   merge_partials over P (chunked by 128 when P > 256: a chunk level first).
    merge_partials over P: ceil(P / 16) merges per wave + 15 wave merges.  Every route ends in the W = 1
    merge of bn_finalize; the slab / given routes start from inputs rounded to fp32 (1)."""
    def mp(P):
        return math.ceil(P / 16) + 15

    if route == "raw":
        return 3 * kw["L"] + 6 + MERGE_OPS * (kw["rpi"] + mp(kw["P"]) + 1)
    if route == "direct":
        return 1 + MERGE_OPS * (math.ceil(kw["R"] / 64) + 16 + 1)
    if route == "split":
        return 1 + MERGE_OPS * (math.ceil(kw["tps"] / 4) + 3 + mp(kw["P"]) + 1)
    if route == "given":
        P = kw["P"]
        if P > 256:
            return 1 + MERGE_OPS * (mp(128) + mp(math.ceil(P / 128)) + 1)
        return 1 + MERGE_OPS * (mp(P) + 1)
    if route == "ranks":
        return 1 + MERGE_OPS * kw["W"]
    raise KeyError(route)


def stat_bounds(x, D):
    """Per-channel bounds on the fp32 statistics of the rows ``x`` [M, C] after a chain of D dependent
    operations: |mean - mu| <= Km u (|mu| + sigma), |M2 - M2*| <= K2 u M2*, u = 2^-24.

    Every quantity on the mean chain is a mean of a subset of the rows or a difference of two, so its
    magnitude is at most |mu| + T sigma with T = max |x - mu| / sigma (>= 1); each operation adds at
    most u of that (first order): Km = 2 D T, the 2 covering the higher-order terms (D u << 1).
    The M2 chain carries sums of squared deviations from a shift or a partial mean that lies within the
    data: each term at most (2 T sigma)^2 per row, 4 T^2 M2* in total, plus the cross term 2 d (delta d)
    n of a mean difference d <= 2 T sigma known to delta d <= D u (|mu| + T sigma):
    K2 = 2 D (4 T^2 + 4 T (|mu| / sigma + T)).
    -> (n, mu, M2*, mean bound, M2 bound); a channel with M2* == 0 has M2 bound 0 (every deviation is an
    exact zero) and mean bound D u |mu|."""
    n, mu, m2 = stats64(x)
    sigma = (m2 / n).sqrt()
    dev = (x.double() - mu).abs().amax(0)
    T = torch.where(sigma > 0, dev / sigma.clamp_min(1e-300), torch.ones_like(sigma)).clamp_min(1.0)
    km = 2.0 * D * T
    ratio = torch.where(sigma > 0, mu.abs() / sigma.clamp_min(1e-300), torch.zeros_like(sigma))
    k2 = 2.0 * D * (4 * T * T + 4 * T * (ratio + T))
    return n, mu, m2, km * U32 * (mu.abs() + sigma), k2 * U32 * m2


def slabs_of(x):
    """per-128-row (mean, M2) of [M, C] in fp64, rounded to fp32: what a conv epilogue hands over"""
    M, C = x.shape
    R = (M + 127) // 128
    out = torch.zeros((R, 2, C), dtype=torch.float64)
    full = M // 128
    if full:
        blk = x[:128 * full].double().reshape(full, 128, C)
        mu = blk.mean(1)
        out[:full, 0], out[:full, 1] = mu, ((blk - mu[:, None]) ** 2).sum(1)
    if full < R:
        blk = x[128 * full:].double()
        mu = blk.mean(0)
        out[full, 0], out[full, 1] = mu, ((blk - mu) ** 2).sum(0)
    return out.float()


def partials_of(x, P, empty=()):
    """(n, mean, M2) of P consecutive row groups of [M, C] (fp64 -> fp32); groups in ``empty`` hold no
    rows (n = 0, mean = M2 = 0) and their rows go to the next group"""
    M, C = x.shape
    live = [p for p in range(P) if p not in empty]
    cuts = [round(i * M / len(live)) for i in range(len(live) + 1)]
    out = torch.zeros((P, 3, C), dtype=torch.float64)
    for j, p in enumerate(live):
        blk = x[cuts[j]:cuts[j + 1]].double()
        if blk.shape[0] == 0:
            continue
        mu = blk.mean(0)
        out[p, 0], out[p, 1], out[p, 2] = float(blk.shape[0]), mu, ((blk - mu) ** 2).sum(0)
    return out.float()


@functools.lru_cache(maxsize=None)
def stat_rows(M, C, kind="plain"):
    """rows for the statistics tests (bf16 lattice): channel 0 constant, channel 1 all zero, channel 2
    with mean / sigma = 301 -- the values 150 and 151, the closest pair of bf16 numbers to a ratio of 300 -- the rest
    uniform integers with per-channel offsets"""
    key = ("st", M, C, kind)
    x = lattice((M, C), -31, 31, _seed("x", key)).double()
    x = x + int_vector(C, -20, 20, _seed("off", key)).double()
    x[:, 0] = 37.0
    x[:, 1] = 0.0
    g = torch.Generator().manual_seed(_seed("hi", key))
    x[:, 2] = 150.0 + torch.randint(0, 2, (M,), generator=g).double()
    xb = x.to(BF16)
    assert torch.equal(xb.double(), x)
    return xb


# ----------------------------------------------------------------------------- pooling problems
POOL_GEOS = ((3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 2, 0), (2, 1, 0), (5, 2, 2))
POOL_SIZES = ((1, 1), (2, 2), (7, 5), (17, 15), (2, 6))


def pool_valid(H, W, k, s, p):
    """geometries with at least one whole window position (H + 2p >= k): every window then holds at
    least one pixel of the image, since p <= k / 2"""
    return H + 2 * p >= k and W + 2 * p >= k


@functools.lru_cache(maxsize=None)
def pool_problem(N, H, W, C, k, s, p):
    """tie-heavy lattice: values on five levels, so most windows hold their maximum more than once"""
    key = ("pool", N, H, W, C, k, s, p)
    x = lattice((N, H, W, C), -2, 2, _seed("x", key)) * 3
    y, idx, tied = maxpool_first(x.double(), k, s, p)
    Ho, Wo = out_hw(H, W, k, s, p)
    dy = lattice((N, Ho, Wo, C), -100, 100, _seed("dy", key))
    dx = maxpool_bwd_exact(dy, idx, H, W, k, s, p)
    need_fp32(dx=dx)
    if y.numel() >= MIN_SHARE_ELEMS and min(H, W) >= k > 1:
        assert tied >= 0.20, f"only {tied:.1%} of the windows hold a tied maximum"
    return SimpleNamespace(x=x, y=y, want_y=rounded(y, BF16), idx=idx, tied=tied, dy=dy, dx=dx,
                           want_dx=rounded(dx, BF16), geo=(k, s, p), shape=(N, H, W, C))


@functools.lru_cache(maxsize=None)
def bn_pool_problem(N, H, W, C, k, s, p, act):
    """BN (+ ReLU) -> max pool fused: a = bf16(act(x scale + shift)) pooled; backward with the gathered
    gradient rounded to bf16 first (a lattice integer within +-256 stays itself only up to 256: dy is
    kept within +-28 so that a sum of <= ceil(k/s)^2 <= 9 of them does), masked where z <= 0, then the
    training BN backward over the M = N H W input rows -- N H W a power of two for an exact 1 / count."""
    key = ("bnpool", N, H, W, C, k, s, p, act)
    M = N * H * W
    x = lattice((N, H, W, C), -3, 3, _seed("x", key))
    scale = pow2_scales(C, _seed("sc", key), exps=(0, 1))
    shift = int_vector(C, -2, 2, _seed("sh", key))
    mean = int_vector(C, -2, 2, _seed("mu", key))
    invstd = pow2_scales(C, _seed("is", key), exps=(-1, 0, 1)).abs()
    z = bn_z(x, scale, shift)
    a = rounded(act_f(z, act, 0.0), BF16).double()
    y, idx, tied = maxpool_first(a, k, s, p)
    Ho, Wo = out_hw(H, W, k, s, p)
    dy = lattice((N, Ho, Wo, C), -28, 28, _seed("dy", key))
    g = maxpool_bwd_exact(dy, idx, H, W, k, s, p)
    assert torch.equal(rounded(g, BF16).double(), g), "gathered pool gradient must be a bf16 number"
    if act == 1:
        g = torch.where(z > 0, g, torch.zeros_like(g))
    xf, gf, zf = x.double().reshape(M, C), g.reshape(M, C), z.reshape(M, C)
    count = M if (M & (M - 1)) == 0 else None
    dz, s1, s2, dx = bn_bwd_textbook(gf, xf, zf, mean, invstd, scale, 0, 0.0, count)
    need_fp32(s1=s1, s2=s2, s2raw=s2 / invstd.double())
    out = SimpleNamespace(x=x, scale=scale, shift=shift, mean=mean, invstd=invstd, z=z, y=y, want_y=rounded(y, BF16),
                          idx=idx, tied=tied, dy=dy, want_sums=rounded(torch.stack([s1, s2]), F32), count=count,
                          geo=(k, s, p), shape=(N, H, W, C), act=act)
    if count is not None:
        sc, mu, is_ = scale.double(), mean.double(), invstd.double()
        a2, a3 = s1 / count, s2 / count * is_
        cb, cc = -sc * a3, -sc * a2 + sc * a3 * mu
        need_fp32(a2=a2, a3=a3, cb=cb, cc=cc, sca3mu=sc * a3 * mu, t1=sc * dz, t2=cb * xf, t12=sc * dz + cb * xf,
                  out=sc * dz + cb * xf + cc)
        assert torch.equal(sc * dz + cb * xf + cc, dx)
        out.dx, out.want_dx = dx.reshape(N, H, W, C), rounded(dx, BF16).reshape(N, H, W, C)
    if y.numel() >= MIN_SHARE_ELEMS and min(H, W) >= k:
        assert tied >= 0.20, f"only {tied:.1%} of the windows hold a tied maximum"
    if z.numel() >= MIN_SHARE_ELEMS:
        assert (z == 0).double().mean().item() >= 0.05, "fewer than 5 % of the elements at z == 0"
        if count is not None:
            norep, ties = lattice_shares(dx)
            assert norep >= 0.05 and ties >= 0.01, f"dx: {norep:.1%} need rounding, {ties:.1%} ties"
    return out


@functools.lru_cache(maxsize=None)
def gap_problem(N, HW, C):
    key = ("gap", N, HW, C)
    x = lattice((N, HW, C), -127, 127, _seed("x", key))
    s = x.double().sum(1)
    dy = lattice((N, C), -127, 127, _seed("dy", key)) * 2
    add = lattice((N, HW, C), -100, 100, _seed("add", key))
    return SimpleNamespace(x=x, sum=s, dy=dy, add=add, N=N, HW=HW, C=C)


@functools.lru_cache(maxsize=None)
def chan_scale_problem(N, HW, C):
    """y = relu?(x g + res), gate a power of two; a fifth of the positions candidates for a planted z == 0"""
    key = ("cs", N, HW, C)
    x = lattice((N, HW, C), -127, 127, _seed("x", key))
    gate = pow2_scales(N * C, _seed("g", key), exps=(-1, 0, 1, 2, 3)).reshape(N, C).to(BF16)
    res = lattice((N, HW, C), -100, 100, _seed("r", key))
    dy = lattice((N, HW, C), -7, 7, _seed("dy", key))
    gen = torch.Generator().manual_seed(_seed("plant", key))
    plant = torch.rand((N, HW, C), generator=gen) < 0.2
    xg = x.double() * gate.double()[:, None, :]
    r0 = -xg
    ok = plant & (r0 == r0.round()) & (r0.abs() <= 256)
    res = _plant(ok, r0, res)
    # no residual: z == 0 needs x == 0
    x0 = _plant(plant, torch.zeros_like(x), x)
    out = SimpleNamespace(N=N, HW=HW, C=C, gate=gate, dy=dy, cases={})
    for relu in (False, True):
        for has_res in (False, True):
            xx = x if has_res else x0
            z = xx.double() * gate.double()[:, None, :] + (res.double() if has_res else 0.0)
            dz = dy.double() * (act_d(z, 1, 0.0) if relu else 1.0)
            dg = (dz * xx.double()).sum(1)
            dx = dz * gate.double()[:, None, :]
            need_fp32(z=z, dg=dg, dx=dx)
            out.cases[(relu, has_res)] = SimpleNamespace(
                x=xx, res=res if has_res else None, z=z, y=act_f(z, 1, 0.0) if relu else z, dz=dz, dg=dg, dx=dx,
                want_y=rounded(act_f(z, 1, 0.0) if relu else z, BF16), want_dx=rounded(dx, BF16),
                want_dg=rounded(dg, BF16), want_dres=rounded(dz, BF16))
    return out


ADAPTIVE = (((10, 13), (7, 7)), ((14, 14), (7, 7)), ((7, 7), (7, 7)), ((2, 2), (7, 7)), ((3, 5), (7, 7)),
            ((1, 1), (7, 7)))


@functools.lru_cache(maxsize=None)
def adaptive_problem(N, H, W, C, OH, OW):
    key = ("ad", N, H, W, C, OH, OW)
    x = lattice((N, H, W, C), -127, 127, _seed("x", key))
    s, cnt = adaptive_avg_sum(x, OH, OW)
    want_y, one_y, bound_y = two_roundings(s, cnt[None, :, :, None])
    dy = lattice((N, OH, OW, C), -127, 127, _seed("dy", key)) * 2
    # backward: acc += fp32(dy * fp32(1/cnt)) per containing cell, in (oh, ow) order; each product is
    # rounded to fp32 and so is each partial sum -- replayed in that order (the kernel's candidate scan
    # is ascending in oh, then ow)
    # A compiler may contract ``acc += g * inv`` into one FMA, which skips the product's rounding; where
    # a pixel sits in several cells whose 1 / cnt is inexact the two forms can differ in the last bit,
    # so both are modelled and the kernel must equal one of them per element (``want_dx`` product
    # rounded, ``want_dx_fma`` contracted).  With every cnt a power of two (up-sampling, H | OH windows
    # of 1, 2 or 4 pixels) the two coincide and the result is exact.
    cells = adaptive_avg_bwd_terms(dy, H, W)
    acc = torch.zeros((N, H, W, C), dtype=F32)
    accf = torch.zeros((N, H, W, C), dtype=F32)
    one = torch.zeros((N, H, W, C), dtype=torch.float64)
    mag = torch.zeros((N, H, W, C), dtype=torch.float64)
    ncell = torch.zeros((H, W), dtype=torch.float64)
    for h in range(H):
        for w in range(W):
            ncell[h, w] = len(cells[h][w])
            for (oh, ow, c) in cells[h][w]:
                term = dy[:, oh, ow].double() * f32_recip(c)  # exact in fp64 (8 x 24 bits)
                acc[:, h, w] = (acc[:, h, w].double() + term.float().double()).float()
                accf[:, h, w] = (accf[:, h, w].double() + term).float()
                one[:, h, w] += dy[:, oh, ow].double() / c
                mag[:, h, w] += (dy[:, oh, ow].double() / c).abs()
    # per term u for fp32(1 / cnt) and u for the product, u per partial sum; then half a bf16 ulp
    e32 = (2.0 + ncell)[None, :, :, None] * U32 * mag * (1 + 1e-6)
    bound = e32 + 0.5 * bf16_ulp(one.abs() + e32)
    return SimpleNamespace(x=x, want_y=want_y, one_y=one_y, bound_y=bound_y, dy=dy, want_dx=acc.to(BF16),
                           want_dx_fma=accf.to(BF16), one_dx=one, bound_dx=bound,
                           max_cells=int(ncell.max().item()), shape=(N, H, W, C), out=(OH, OW))


# ----------------------------------------------------------------------------- reports
def pointwise_report(got, want, C, rpi=None, limit=8):
    """mismatches by row mod 4 rpi, channel mod 8 / 16 / 64 and row slot (row mod rpi)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    g, w = got.reshape(-1, got.shape[-1]).double(), want.reshape(-1, want.shape[-1]).double()
    bad = (g != w) | (torch.isnan(g) != torch.isnan(w))
    per = max(1, C // got.shape[-1])  # mask bytes: 8 channels per column
    idx = bad.nonzero()
    rpi = rpi or rpi_of(C)
    lines = [f"{idx.shape[0]} of {g.numel()} elements differ (rows {g.shape[0]}, C {C}, rpi {rpi})"]
    for r, c in idx[:limit].tolist():
        lines.append(f"  row {r} col {c * per}: got {g[r, c].item():g} want {w[r, c].item():g}")

    def hist(v, m):
        cnt = torch.bincount(v % m, minlength=m)
        top = torch.argsort(cnt, descending=True)[:8]
        return ", ".join(f"{int(k)}:{int(cnt[k])}" for k in top if cnt[k] > 0)

    row, ch = idx[:, 0], idx[:, 1] * per
    lines.append(f"  by row mod 4 rpi ({4 * rpi}): {hist(row, 4 * rpi)}")
    lines.append(f"  by row slot (row mod {rpi}): {hist(row, rpi)}")
    for m in (8, 16, 64):
        lines.append(f"  by channel mod {m}: {hist(ch, m)}")
    return "\n".join(lines)


def assert_pointwise(got, want, C, what="", rpi=None):
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} vs {want.dtype}"
    if want.device != got.device:
        want = want.to(got.device)
    if torch.equal(got, want):
        return
    raise AssertionError(f"{what}: not bit-exact\n" + pointwise_report(got, want, C, rpi))


def relerr(a, b):
    """the whole-tensor criterion of tests/test_kernels_gpu.py"""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
