"""fp64 oracle for the fused stem backward (csrc/stem.hip stem_bwd_kernel, stem_bwd_dw) and the stem
weight's index maps (csrc/misc.hip s2d_weight / s2d_weight_bwd) -- helper module, not collected.

Written from the definitions, not from ops/_ref.py and not from the kernel's phases:

  g    = bf16(3x3 / 2 / pad 1 max-pool backward of dy through idx)      the gathered window sum, rounded once
  g'   = g where z scale + shift > 0, else 0 (act == 1);  g (act == 0)
  zc   = bf16(z - mean)
  X[px][(ty, tx, c)] = x16[n][y + ty - 2][x + tx - 2][c], zero outside the image    (k = ty 64 + tx 16 + c)
  G1 = g'^T X,  G2 = zc^T X,  G3 = sum_px X,  s1 = sum g',  s2raw = sum g' zc
  tot  = [G1 (64 x 256) | G2 (64 x 256) | G3 (256) | s1 (64) | s2raw (64)],  sums = [s1, s2raw invstd]
  dW   = scale (G1 - a3 G2 - a2 G3),  a2 = s1 / count,  a3 = s2raw invstd^2 / count           (``dw_algebra``)
  dW   = sum_px dz X,  dz = scale (g' - a2 - a3 zc): the training-mode BN backward of g'       (``dw_textbook``)

``z`` and ``x16`` are independent inputs of the kernel and are drawn independently.

Lattice (``problem``): x16, z, dy, shift and mean are small integers, scale and invstd powers of two, so
every product and every partial sum, in any order and under any FMA contraction, is an integer; the
builder asserts on the reference alone that the sum of ABSOLUTE values behind every entry of ``tot`` is
below 2^24, and then fp32 holds every partial sum of any summation order: ``tot`` and ``sums`` are
compared with ``torch.equal``.  z sits on five even levels (most pooling windows tied, as pool_problem)
and every channel's shift puts one level exactly on the ReLU boundary z scale + shift == 0.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests.exact_oracle import (BF16, F32, TWO24, _seed, assert_exact, int_vector, lattice, pow2_scales,  # noqa: F401
                                rounded)
from tests.pointwise_oracle import maxpool_bwd_exact, maxpool_first, need_fp32

CO, KC = 64, 256  # output channels; patch columns k = (ty, tx, c) = 4 x 4 x 16
TOT = 2 * CO * KC + KC + 2 * CO
WIDTHS = (16, 32, 48, 56, 64, 80, 96, 112)  # the stem_bwd_kernel<W> instantiations
KTAIL16 = (16, 48, 80, 112)  # last k-step of 32 pixels holds <= 16: the 16-deep MFMA path
DW_DIMS = ("co", "ty", "tx", "c")


def launch_geometry(N, H, cu):
    """(workgroups, rows per workgroup) of the launcher: min(N H, CUs) and the ceiling of the ratio"""
    nb = min(N * H, cu)
    return nb, -(-(N * H) // nb)


# ----------------------------------------------------------------------------- definitions (fp64)
def patches(x16):
    """[n,H,W,16] -> [n,H,W,256]: X[..., ty 64 + tx 16 + c] = x16[n][y + ty - 2][x + tx - 2][c]"""
    n, H, W, _ = x16.shape
    xp = F.pad(x16.double(), (0, 0, 2, 1, 2, 1))  # W by (2, 1), H by (2, 1)
    return torch.cat([xp[:, ty:ty + H, tx:tx + W] for ty in range(4) for tx in range(4)], -1)


def pixel_terms(z, dy, idx, scale, shift, mean, act, bf16=True):
    """-> (g' [N,H,W,64], zc [N,H,W,64], the unrounded gathered sum); ``bf16=False`` leaves out the two
    roundings (inputs that are not bf16 numbers: the autograd comparison)"""
    N, H, W, _ = z.shape
    raw = maxpool_bwd_exact(dy, idx, H, W, 3, 2, 1)
    g = rounded(raw, BF16).double() if bf16 else raw
    zd = z.double()
    if act == 1:
        g = torch.where(zd * scale.double() + shift.double() > 0, g, torch.zeros_like(g))
    zc = zd - mean.double()
    if bf16:
        zc = rounded(zc, BF16).double()
    return g, zc, raw


def _chunks(N, rows_per_image, limit=8192):
    step = max(1, limit // rows_per_image)
    return [(a, min(N, a + step)) for a in range(0, N, step)]


def reference(z, x16, dy, idx, scale, shift, mean, invstd, act, bf16=True):
    """The five sums in fp64, image chunk by image chunk, and the largest sum of absolute values behind
    an entry of each (``absmax``: the lattice condition)."""
    N, H, W, _ = z.shape
    g, zc, raw = pixel_terms(z, dy, idx, scale, shift, mean, act, bf16)
    G1, G3 = torch.zeros(CO, KC, dtype=torch.float64), torch.zeros(KC, dtype=torch.float64)
    G2, A1, A2, A3 = torch.zeros_like(G1), torch.zeros_like(G1), torch.zeros_like(G1), torch.zeros_like(G3)
    for a, b in _chunks(N, H * W):
        X = patches(x16[a:b]).reshape(-1, KC)
        gc, zcc = g[a:b].reshape(-1, CO), zc[a:b].reshape(-1, CO)
        G1 += gc.t() @ X
        G2 += zcc.t() @ X
        G3 += X.sum(0)
        Xa = X.abs()
        A1 += gc.abs().t() @ Xa
        A2 += zcc.abs().t() @ Xa
        A3 += Xa.sum(0)
    gf, zf = g.reshape(-1, CO), zc.reshape(-1, CO)
    s1, s2raw = gf.sum(0), (gf * zf).sum(0)
    absmax = max(A1.max().item(), A2.max().item(), A3.max().item(), gf.abs().sum(0).max().item(),
                 (gf * zf).abs().sum(0).max().item())
    tot = torch.cat([G1.reshape(-1), G2.reshape(-1), G3, s1, s2raw])
    sums = torch.stack([s1, s2raw * invstd.double()])
    return SimpleNamespace(g=g, zc=zc, raw=raw, G1=G1, G2=G2, G3=G3, s1=s1, s2raw=s2raw, tot=tot, sums=sums,
                           absmax=absmax)


def split_tot(tot):
    """-> {name: (view, dims)} of a [TOT] tensor, for comparisons that name the (ty, tx, c) column"""
    n = CO * KC
    return {"G1": (tot[:n].reshape(CO, 4, 4, 16), DW_DIMS), "G2": (tot[n:2 * n].reshape(CO, 4, 4, 16), DW_DIMS),
            "G3": (tot[2 * n:2 * n + KC].reshape(4, 4, 16), DW_DIMS[1:]),
            "s1": (tot[2 * n + KC:2 * n + KC + CO], ("co",)), "s2raw": (tot[2 * n + KC + CO:], ("co",))}


def dw_terms(G1, G2, G3, s1, s2raw, scale, invstd, count):
    """the three terms of the algebraic form and the coefficients (fp64)"""
    a2 = s1.double() / count
    a3 = s2raw.double() * invstd.double() ** 2 / count
    return G1.double(), a3[:, None] * G2.double(), a2[:, None] * G3.double()[None, :], a2, a3


def dw_algebra(G1, G2, G3, s1, s2raw, scale, invstd, count):
    """-> (dW [64,4,4,16], mag = |scale| (|G1| + |a3 G2| + |a2 G3|) per element)"""
    t1, t2, t3, _, _ = dw_terms(G1, G2, G3, s1, s2raw, scale, invstd, count)
    sc = scale.double()[:, None]
    mag = sc.abs() * (t1.abs() + t2.abs() + t3.abs())
    return (sc * (t1 - t2 - t3)).reshape(CO, 4, 4, 16), mag.reshape(CO, 4, 4, 16)


def dw_textbook(ref, x16, scale, invstd, count):
    """sum_px dz X with dz the training-mode BN backward of g' over ``count`` rows"""
    a2 = ref.s1 / count
    a3 = ref.s2raw * invstd.double() ** 2 / count
    dz = scale.double() * (ref.g - a2 - a3 * ref.zc)
    N, H, W, _ = dz.shape
    dw = torch.zeros(CO, KC, dtype=torch.float64)
    for a, b in _chunks(N, H * W):
        dw += dz[a:b].reshape(-1, CO).t() @ patches(x16[a:b]).reshape(-1, KC)
    return dw.reshape(CO, 4, 4, 16)


def dw_bound(mag, pow2_count):
    """|fp32 dW - exact dW| per element, from the formula scale (G1 - a3 G2 - a2 G3) itself: a2 = fl(s1 ic)
    carries one rounding, a3 = fl(fl(s2 ic) invstd) two, each product one more, then two subtractions and
    the multiply by scale -- the G1 term passes 3 roundings, a2 G3 passes 5, a3 G2 passes 6; (1 + u)^6 - 1
    <= 8 u with the higher orders, u = 2^-24.  ic = float(1 / count) is exact for a power of two and within
    u of 1 / count otherwise: one more u."""
    return (8.0 if pow2_count else 9.0) * 2.0 ** -24 * mag


# ----------------------------------------------------------------------------- stem weight index maps
def s2d_weight_ref(w7):
    """[Co,7,7,C<=4] -> [Co,4,4,16]: w16[co][ta][tb][(py 2 + px) 4 + c] = w7[co][2 ta + py - 1][2 tb + px - 1][c]"""
    Co, _, _, C = w7.shape
    w16 = torch.zeros(Co, 4, 4, 16, dtype=w7.dtype)
    for ta in range(4):
        for tb in range(4):
            for py in range(2):
                for px in range(2):
                    kh, kw = 2 * ta + py - 1, 2 * tb + px - 1
                    if 0 <= kh < 7 and 0 <= kw < 7:
                        q = (py * 2 + px) * 4
                        w16[:, ta, tb, q:q + C] = w7[:, kh, kw, :]
    return w16


def s2d_weight_bwd_ref(g16, C):
    """the transpose: gather back onto [Co,7,7,C], dropping the padded row / column and channels"""
    Co = g16.shape[0]
    g7 = torch.zeros(Co, 7, 7, C, dtype=g16.dtype)
    for kh in range(7):
        for kw in range(7):
            ta, py, tb, px = (kh + 1) // 2, (kh + 1) % 2, (kw + 1) // 2, (kw + 1) % 2
            q = (py * 2 + px) * 4
            g7[:, kh, kw, :] = g16[:, ta, tb, q:q + C]
    return g7


# ----------------------------------------------------------------------------- lattice problems
FAMILIES = ("plain", "bigdy", "corner", "four", "bigfour", "xrow", "grow")


@functools.lru_cache(maxsize=None)
def problem(N, H, W, act, family="plain", row=None):
    """One lattice problem and its exact ``tot`` / ``sums``.

    plain      idx = the first-maximum argmax of act(z scale + shift), |dy| <= 28 (four windows sum within 256)
    bigdy      |dy| <= 200: the gathered sum passes 256 and its bf16 rounding, ties included, matters
    corner     every window points at its bottom-right tap: pixel (2 ho + 1, 2 wo + 1) gets that one window,
               pixels on an even row or column get nothing
    four       the four windows around pixel (2 ho + 1, 2 wo + 1), ho and wo even, all point at it (taps 8, 6,
               2, 0 by window parity): those pixels sum four terms, every other pixel gets nothing
    bigfour    four with |dy| <= 200: the four-term sums pass 256
    xrow       plain, x16 nonzero in the image row ``row`` = (n, y) alone
    grow       dy nonzero in one pooled row alone, argmax on the window's centre row: g' nonzero in the
               image row (n, y) alone, y even
    """
    assert family in FAMILIES and H % 2 == 0 and W % 2 == 0
    key = ("stem_bwd", N, H, W, act, family, row)
    Ho, Wo = H // 2, W // 2
    x16 = lattice((N, H, W, 16), -7, 7, _seed("x", key))
    z = lattice((N, H, W, CO), -2, 2, _seed("z", key)) * 2
    scale = pow2_scales(CO, _seed("sc", key))
    level = int_vector(CO, -1, 1, _seed("lv", key)) * 2  # an inner level: both signs of z scale + shift occur
    shift = -scale * level + 0.0  # the level of z that lands on z scale + shift == 0; an integer
    mean = int_vector(CO, -2, 2, _seed("mu", key))
    invstd = pow2_scales(CO, _seed("is", key)).abs()
    big = family in ("bigdy", "bigfour")
    dy = lattice((N, Ho, Wo, CO), -200 if big else -28, 200 if big else 28, _seed("dy", key))
    zs = z.double() * scale.double() + shift.double()
    pooled = torch.where(zs > 0, zs, torch.zeros_like(zs)) if act == 1 else zs
    _, idx, tied = maxpool_first(pooled, 3, 2, 1)
    if family == "corner":
        idx = torch.full_like(idx, 8)
    if family in ("four", "bigfour"):
        ho, wo = torch.arange(Ho)[:, None] % 2, torch.arange(Wo)[None, :] % 2
        tap = torch.tensor([[8, 6], [2, 0]], dtype=torch.uint8)[ho, wo]  # [Ho,Wo]: kh = 2 (1 - ho), kw = 2 (1 - wo)
        idx = tap[None, :, :, None].expand_as(idx).contiguous()
    if family == "xrow":
        n0, y0 = row
        keep = torch.zeros((N, H, 1, 1), dtype=torch.bool)
        keep[n0, y0] = True
        x16 = torch.where(keep, x16, torch.zeros_like(x16))
    if family == "grow":
        n0, y0 = row
        assert y0 % 2 == 0
        keep = torch.zeros((N, Ho, 1, 1), dtype=torch.bool)
        keep[n0, y0 // 2] = True
        dy = torch.where(keep, dy, torch.zeros_like(dy))
        g = torch.Generator().manual_seed(_seed("kw", key))
        kw = torch.randint(0, 3, idx.shape, generator=g)
        kw[:, :, 0] = kw[:, :, 0].clamp_min(1)  # tap column -1 of the first window is outside the image
        idx = (3 + kw).to(torch.uint8)  # kh = 1: pixel row 2 ho
    ref = reference(z, x16, dy, idx, scale, shift, mean, invstd, act)
    # ---- preconditions, on the reference alone
    for t in (x16, z, dy, shift, mean, ref.g, ref.zc):
        assert bool((t.double() == t.double().round()).all()), "lattice values must be integers"
    assert ref.absmax < TWO24, f"partial sums may leave the fp32 integers: {ref.absmax:.3g} >= 2^24"
    need_fp32(tot=ref.tot, sums=ref.sums)
    z0 = (zs == 0).double().mean().item()
    assert z0 >= 0.05, f"only {z0:.1%} of z scale + shift sit at 0"
    if family in ("plain", "bigdy", "xrow"):
        assert tied >= 0.20, f"only {tied:.1%} of the windows hold a tied maximum"
    assert bool((ref.g.reshape(-1, CO) != 0).any(0).all()), "a channel of g' is all zero"
    off = (ref.raw != rounded(ref.raw, BF16).double()).double().mean().item()  # share of gathered sums bf16 rounds
    if big:
        assert off >= (0.005 if family == "bigfour" else 0.002), f"only {off:.2%} of the gathered sums are rounded"
    if family == "grow":
        rows = (ref.g != 0).any(3).any(2).nonzero().tolist()
        assert rows == [list(row)], rows
    return SimpleNamespace(N=N, H=H, W=W, act=act, family=family, x16=x16, z=z, dy=dy, idx=idx, scale=scale,
                           shift=shift, mean=mean, invstd=invstd, ref=ref, tied=tied, z0=z0, rounded_share=off,
                           want_tot=rounded(ref.tot, F32), want_sums=rounded(ref.sums, F32))
