"""The BN / pooling / channel-scale oracle (tests/pointwise_oracle.py) checked on the CPU alone.

* Preconditions: for every problem tests/test_bn_exact_gpu.py and tests/test_pool_exact_gpu.py use,
  the reference alone shows that every intermediate is an fp32 number (asserted inside the
  builders), that >= 5 % of the bf16 outputs need rounding and >= 1 % are ties, that >= 5 % of the
  elements sit at z == 0 (some at -0.0) and that >= 20 % of the pooling windows hold a tied maximum.
* The oracle agrees with torch's own fp64 operators where torch has one (batch_norm autograd,
  max_pool2d on tie-free data, adaptive_avg_pool2d), so the definitions are the usual ones.
* Sensitivity: each defect of the list below, planted in a small torch emulation of the kernel,
  passes the whole-tensor criterion of tests/test_kernels_gpu.py (Gaussian inputs, ``relerr < 1e-2``,
  the compile-time 3x3/2 pool) and fails the new check.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_oracle as P

BF16, F32 = P.BF16, P.F32
SLOPE = P.LEAKY_SLOPE


# ----------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("C", P.BN_C)
def test_bn_forward_preconditions(C):
    """every (act, residual) combination over the row counts of one channel count: z, y fp32 numbers
    (asserted by bn_case), shares of rounded / tied outputs and of z == 0 over the channel count's cases"""
    for act in P.ACTS:
        for res, two in ((False, False), (True, False), (True, True)):
            cases = [P.bn_case(P.bn_base(C, M), act, res, two=two) for M in P.bn_rows(C)]
            norep, ties, z0, zneg = P.check_bn_shares(cases)
            if not res:
                assert zneg > 0, "no element reaches z == -0.0"


@pytest.mark.parametrize("C", P.BN_C)
def test_bn_backward_preconditions(C):
    for M in P.bwd_rows(C):
        b = P.bn_base(C, M, small=True)
        for act in P.ACTS:
            for res in (False, True):
                c = P.bn_case(b, act, res, count=float(M))
                P.check_bn_shares([c], "dx")
        for act in (0, 2):  # InplaceABN: from the output
            c = P.bn_case(b, act, False, count=float(M), inv=True)
            P.check_bn_shares([c], "dx")
        two = P.bn2_case(b)
        for v in (two.dx, two.dr):
            norep, ties = P.lattice_shares(v)
            assert norep >= 0.05 and ties >= 0.01, (norep, ties)


def test_bn_backward_matches_torch_autograd():
    """the textbook backward of the oracle == autograd of torch's fp64 batch_norm + relu"""
    M, C = 64, 24
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 0.5
    w, bias = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    xt = x.clone().requires_grad_(True)
    y = torch.relu(F.batch_norm(xt, None, None, w, bias, training=True, eps=1e-5))
    y.backward(dy)
    n, mu, m2 = P.stats64(x)
    invstd = 1 / (m2 / n + 1e-5).sqrt()
    scale, shift = w * invstd, bias - mu * w * invstd
    z = P.bn_z(x, scale, shift)
    assert torch.allclose(P.act_f(z, 1, 0.0), y.detach(), rtol=1e-12, atol=1e-12)
    _, _, _, dx = P.bn_bwd_textbook(dy, x, z, mu, invstd, scale, 1, 0.0, float(M))
    assert torch.allclose(dx, xt.grad, rtol=1e-10, atol=1e-12)


def _pool_cases(C=8):
    for k, s, p in P.POOL_GEOS:
        for H, W in P.POOL_SIZES:
            if P.pool_valid(H, W, k, s, p):
                yield P.pool_problem(2, H, W, C, k, s, p)


def test_pool_preconditions_and_torch_agreement():
    for pr in _pool_cases():
        k, s, p = pr.geo
        N, H, W, C = pr.shape
        if H * W >= 35 and k * k > 1:
            assert pr.tied >= 0.20, f"{pr.shape} {pr.geo}: only {pr.tied:.1%} of the windows hold a tied maximum"
        yt = F.max_pool2d(pr.x.double().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
        assert torch.equal(yt, pr.y)
        # the argmax points at a pixel that holds the maximum, and no earlier tap of the window does
        for n_, ho, wo, c in [(0, 0, 0, 0), (1, pr.y.shape[1] - 1, pr.y.shape[2] - 1, C - 1)]:
            t = int(pr.idx[n_, ho, wo, c])
            vals = []
            for kh in range(k):
                for kw in range(k):
                    hi, wi = ho * s - p + kh, wo * s - p + kw
                    vals.append(pr.x[n_, hi, wi, c].item() if 0 <= hi < H and 0 <= wi < W else -math.inf)
            assert vals[t] == max(vals) and all(v < vals[t] for v in vals[:t])
        assert pr.dx.abs().max() <= 100 * math.ceil(k / s) ** 2  # at most ceil(k/s)^2 windows per pixel
        assert torch.equal(pr.dx.sum((1, 2)), pr.dy.double().sum((1, 2)))


def test_bn_pool_preconditions():
    for C in (8, 64, 256):
        for geo in ((3, 2, 1), (2, 2, 0)):
            pr = P.bn_pool_problem(4, 8, 8, C, *geo, 1)
            assert pr.count == 256.0 and pr.tied >= 0.20
            assert (pr.z == 0).double().mean() >= 0.05
            norep, ties = P.lattice_shares(pr.dx)
            assert norep >= 0.05 and ties >= 0.01, (norep, ties)


@pytest.mark.parametrize("hw,ohw", P.ADAPTIVE)
def test_adaptive_oracle_matches_torch(hw, ohw):
    pr = P.adaptive_problem(2, *hw, 8, *ohw)
    yt = F.adaptive_avg_pool2d(pr.x.double().permute(0, 3, 1, 2), ohw).permute(0, 2, 3, 1)
    assert torch.allclose(pr.one_y, yt, rtol=1e-13, atol=1e-13)
    xt = pr.x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.adaptive_avg_pool2d(xt, ohw).backward(pr.dy.double().permute(0, 3, 1, 2))
    assert torch.allclose(pr.one_dx, xt.grad.permute(0, 2, 3, 1), rtol=1e-13, atol=1e-13)
    # the two-rounding model stays inside its own bound against the one-rounding value
    assert bool(((pr.want_y.double() - pr.one_y).abs() <= pr.bound_y).all())
    assert bool(((pr.want_dx.double() - pr.one_dx).abs() <= pr.bound_dx).all())
    assert bool(((pr.want_dx_fma.double() - pr.one_dx).abs() <= pr.bound_dx).all())


def test_gap_and_chan_scale_preconditions():
    for N, HW, C in ((3, 49, 24), (1, 64, 72)):
        g = P.gap_problem(N, HW, C)
        want, one, bound = P.two_roundings(g.sum, HW)
        assert bool(((want.double() - one).abs() <= bound).all())
        cs = P.chan_scale_problem(N, HW, C)
        for (relu, has_res), c in cs.cases.items():
            assert (c.z == 0).double().mean() >= 0.05
            if has_res:
                norep, ties = P.lattice_shares(c.y)
                assert norep >= 0.05 and ties >= 0.01


# ----------------------------------------------------------------------------- emulations with planted defects
def gauss(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF16)


def emu_bn_act(x, sc, sh, res, act, slope, defect=None):
    z = x.float() * sc + sh
    if res is not None:
        z = z + res.float()
    y = P.act_f(z, act, slope)
    mask = P.mask_bytes(z >= 0 if defect == "mask_ge" else z > 0)
    yb = y.to(BF16)
    if defect == "tail":  # bn_act_rows' tail loop stops one row early: the last row is never written
        yb[-1] = 0
    return y, yb, mask


def emu_bn_bwd(dy, x, res, sc, sh, mu, is_, act, slope, count, defect=None):
    z = x.float() * sc + sh
    if res is not None:
        z = z + res.float()
    d = P.act_d(z, act, slope)
    if defect == "relu_ge" and act == 1:
        d = (z >= 0).float()
    dz = dy.float() * d
    s1, s2 = dz.sum(0), (dz * (x.float() - mu)).sum(0) * is_
    a2, a3 = s1 / count, s2 / count * is_
    dx = sc * dz + (-sc * a3) * x.float() + (-sc * a2 + sc * a3 * mu)
    return dx, (P.bf16_trunc(dx) if defect == "trunc" else dx.to(BF16)), dz.to(BF16)


def _merge(a, nb, mb, m2b):
    n, mean, m2 = a
    live = nb > 0
    nt = n + nb
    d = mb - mean
    f = nb / nt.clamp_min(1e-30)
    return (torch.where(live, nt, n), torch.where(live, mean + d * f, mean),
            torch.where(live, m2 + (m2b + d * d * n * f), m2))


def emu_merge_partials(part, NW=16, defect=None):
    P_, _, C = part.shape
    zero = lambda: (torch.zeros(C), torch.zeros(C), torch.zeros(C))  # noqa: E731
    waves = []
    for w in range(NW):
        a = zero()
        for p in range(w, P_, NW):
            a = _merge(a, part[p, 0], part[p, 1], part[p, 2])
        waves.append(a)
    a = waves[0]
    for k in range(1, NW - 1 if defect == "drop_wave" else NW):
        a = _merge(a, *waves[k])
    return a


def emu_merge_slabs(slabs, M, defect=None):
    R, _, C = slabs.shape
    nrow = lambda r: torch.full((C,), float(min(128, M - 128 * r)))  # noqa: E731
    streams = []
    for rs in range(64):
        a = (torch.zeros(C), torch.zeros(C), torch.zeros(C))
        r = rs
        while r + 7 * 64 < R:
            for u in range(8):
                q = r + u * 64
                src = min(q + 1, R - 1) if defect == "slab_plus1" else q
                a = _merge(a, nrow(q), slabs[src, 0], slabs[src, 1])
            r += 8 * 64
        while r < R:
            a = _merge(a, nrow(r), slabs[r, 0], slabs[r, 1])
            r += 64
        streams.append(a)
    lvl = []
    for rs in range(8):
        b = (torch.zeros(C), torch.zeros(C), torch.zeros(C))
        for k in range(8):
            b = _merge(b, *streams[rs + 8 * k])
        lvl.append(b)
    b = (torch.zeros(C), torch.zeros(C), torch.zeros(C))
    for k in range(8):
        b = _merge(b, *lvl[k])
    return b


def emu_partial_sum(part, defect=None):
    P_, K = part.shape
    tot = torch.zeros(K)
    for w in range(4):
        s = [torch.zeros(K) for _ in range(4)]
        p = w
        while p + 60 < P_:
            for u in range(16):
                s[u % 4] = s[u % 4] + part[p + 4 * u]
            p += 64
        while p + 12 < P_:
            for u in range(3 if defect == "drop_term" else 4):
                s[u] = s[u] + part[p + 4 * u]
            p += 16
        while p < P_:
            s[0] = s[0] + part[p]
            p += 4
        tot = tot + ((s[0] + s[1]) + (s[2] + s[3]))
    return tot


def emu_maxpool(x, k, s, p, defect=None):
    N, H, W, C = x.shape
    Ho, Wo = P.out_hw(H, W, k, s, p)
    v = x.float()
    best = torch.full((N, Ho, Wo, C), -math.inf)
    idx = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8)
    for ho in range(Ho):
        for wo in range(Wo):
            for kh in range(k):
                for kw in range(k):
                    hi, wi = ho * s - p + kh, wo * s - p + kw
                    if not (0 <= hi < H and 0 <= wi < W):
                        continue
                    f = v[:, hi, wi]
                    take = f >= best[:, ho, wo] if defect == "ge" else f > best[:, ho, wo]
                    best[:, ho, wo] = torch.where(take, f, best[:, ho, wo])
                    idx[:, ho, wo] = torch.where(take, torch.full_like(idx[:, ho, wo], kh * k + kw), idx[:, ho, wo])
    return best.to(BF16), idx


def emu_pool_gather(dy, idx, H, W, k, s, p, defect=None):
    """gather_pool_grad: the 3x3/2/1 instantiation scans its 2 x 2 candidates, every other geometry
    takes the generic ho_lo .. ho_hi scan (where the defect sits)"""
    N, Ho, Wo, C = dy.shape
    dx = torch.zeros((N, H, W, C))
    generic = (k, s, p) != (3, 2, 1)
    for hi in range(H):
        for wi in range(W):
            ho_lo, ho_hi = max(0, (hi + p - k + s) // s), min(Ho - 1, (hi + p) // s)
            wo_lo, wo_hi = max(0, (wi + p - k + s) // s), min(Wo - 1, (wi + p) // s)
            if generic and defect == "ho_hi_short":
                ho_hi -= 1
            for ho in range(ho_lo, ho_hi + 1):
                kh = hi - (ho * s - p)
                if kh < 0 or kh >= k:
                    continue
                for wo in range(wo_lo, wo_hi + 1):
                    kw = wi - (wo * s - p)
                    if kw < 0 or kw >= k:
                        continue
                    dx[:, hi, wi] += torch.where(idx[:, ho, wo] == kh * k + kw, dy[:, ho, wo].float(),
                                                 torch.zeros(()))
    return dx.to(BF16)


def emu_chan_scale_bwd(dy, x, g, res, defect=None):
    z = x.float() * g.float()[:, None, :] + res.float()
    dz = torch.where(z > 0, dy.float(), torch.zeros(()))
    dres = dz * g.float()[:, None, :] if defect == "dres_g" else dz
    return (dz * g.float()[:, None, :]).to(BF16), dres.to(BF16)


def emu_adaptive_bwd(dy, H, W, defect=None):
    N, OH, OW, C = dy.shape
    dx = torch.zeros((N, H, W, C))
    plus = 0 if defect == "no_plus1" else 1
    for h in range(H):
        for w in range(W):
            oh_lo, oh_hi = max(0, (h * OH) // H - 1), min(OH - 1, ((h + 1) * OH) // H + plus)
            ow_lo, ow_hi = max(0, (w * OW) // W - 1), min(OW - 1, ((w + 1) * OW) // W + plus)
            for oh in range(oh_lo, oh_hi + 1):
                h0, h1 = P.ad_cell(oh, H, OH)
                if h < h0 or h >= h1:
                    continue
                for ow in range(ow_lo, ow_hi + 1):
                    w0, w1 = P.ad_cell(ow, W, OW)
                    if w < w0 or w >= w1:
                        continue
                    inv = torch.tensor(1.0) / float((h1 - h0) * (w1 - w0))
                    dx[:, h, w] += dy[:, oh, ow].float() * inv
    return dx.to(BF16)


OLD = 1e-2  # the widest whole-tensor tolerance of this family in tests/test_kernels_gpu.py


def test_defect_1_tail_row():
    M, C = 20000, 8  # one lost row of 20,000 moves the norm by 0.7 %
    x, sc, sh = gauss(M, C, scale=2.0, shift=0.5), torch.rand(C) + 0.5, torch.randn(C) * 0.1
    ref, _, _ = emu_bn_act(x, sc, sh, None, 1, 0.0)
    _, bad, _ = emu_bn_act(x, sc, sh, None, 1, 0.0, "tail")
    assert P.relerr(bad, ref) < OLD
    c = P.bn_case(P.bn_base(8, 1027), 1, False)
    _, good, _ = emu_bn_act(c.x, c.b.scale, c.b.shift, None, 1, 0.0)
    _, bad, _ = emu_bn_act(c.x, c.b.scale, c.b.shift, None, 1, 0.0, "tail")
    assert torch.equal(good, c.want_y) and not torch.equal(bad, c.want_y)


@pytest.mark.parametrize("defect", ["relu_ge", "trunc"])
def test_defects_2_7_backward(defect):
    M, C = 256, 24
    x, dy = gauss(M, C, scale=2.0, shift=0.5), gauss(M, C, seed=1)
    sc, sh, mu, is_ = torch.rand(C) + 0.5, torch.randn(C) * 0.1, torch.randn(C) * 0.1, torch.rand(C) + 0.5
    ref, _, refd = emu_bn_bwd(dy, x, None, sc, sh, mu, is_, 1, 0.0, M)
    _, bad, badd = emu_bn_bwd(dy, x, None, sc, sh, mu, is_, 1, 0.0, M, defect)
    assert P.relerr(bad, ref) < OLD and P.relerr(badd, refd) < OLD
    c = P.bn_case(P.bn_base(C, M, small=True), 1, False, count=float(M))
    b = c.b
    args = (b.dy, c.x, None, b.scale, b.shift, b.mean, b.invstd, 1, 0.0, M)
    _, good, goodd = emu_bn_bwd(*args)
    _, bad, badd = emu_bn_bwd(*args, defect)
    assert torch.equal(good, c.want_dx) and torch.equal(goodd, c.want_dres)
    assert not (torch.equal(bad, c.want_dx) and torch.equal(badd, c.want_dres))


def test_defect_3_mask_bit():
    M, C = 300, 24
    x, r, sc, sh = gauss(M, C), gauss(M, C, seed=1), torch.rand(C) + 0.5, torch.randn(C) * 0.1
    _, _, m0 = emu_bn_act(x, sc, sh, r, 1, 0.0)
    _, _, m1 = emu_bn_act(x, sc, sh, r, 1, 0.0, "mask_ge")
    assert torch.equal(m0, m1)  # Gaussian inputs: no element at z == 0, the old test cannot tell
    c = P.bn_case(P.bn_base(C, 99), 1, True)
    _, _, good = emu_bn_act(c.x, c.b.scale, c.b.shift, c.res, 1, 0.0)
    _, _, bad = emu_bn_act(c.x, c.b.scale, c.b.shift, c.res, 1, 0.0, "mask_ge")
    assert torch.equal(good, c.want_mask) and not torch.equal(bad, c.want_mask)


def _stat_check(got, x, D):
    n, mu, m2, bm, b2 = P.stat_bounds(x, D)
    ok_n = bool((got[0].double() == n).all())
    ok = bool(((got[1].double() - mu).abs() <= bm).all()) and bool(((got[2].double() - m2).abs() <= b2).all())
    return ok_n, ok


def test_defect_4_merge_partials_drops_a_wave():
    M, C, P_ = 4096, 24, 64
    xg = gauss(M, C, scale=1.0, shift=4.0)
    clean = emu_merge_partials(P.partials_of(xg, P_))
    bad = emu_merge_partials(P.partials_of(xg, P_), defect="drop_wave")
    inv = lambda a: 1 / (a[2] / a[0] + 1e-5).sqrt()  # noqa: E731
    assert P.relerr(bad[1], clean[1]) < OLD and P.relerr(inv(bad), inv(clean)) < OLD  # mean, invstd: what was compared
    x = P.stat_rows(M, C)
    part = P.partials_of(x, P_)
    D = P.stat_chain("given", P=P_)
    assert _stat_check(emu_merge_partials(part), x, D) == (True, True)
    assert _stat_check(emu_merge_partials(part, defect="drop_wave"), x, D)[0] is False  # n is exact or wrong


def test_defect_5_merge_slabs_reads_the_next_slab():
    C, R = 8, 513
    M = 128 * R - 127
    xg = gauss(M, C, scale=1.0, shift=4.0)
    clean, bad = emu_merge_slabs(P.slabs_of(xg), M), emu_merge_slabs(P.slabs_of(xg), M, "slab_plus1")
    inv = lambda a: 1 / (a[2] / a[0] + 1e-5).sqrt()  # noqa: E731
    assert P.relerr(bad[1], clean[1]) < OLD and P.relerr(inv(bad), inv(clean)) < OLD
    x = P.stat_rows(M, C)
    D = P.stat_chain("direct", R=R)
    assert _stat_check(emu_merge_slabs(P.slabs_of(x), M), x, D) == (True, True)
    assert _stat_check(emu_merge_slabs(P.slabs_of(x), M, "slab_plus1"), x, D)[1] is False


def test_defect_6_partial_sum_drops_a_term():
    P_, K = 64 * 40 + 16, 48  # the 16-wide loop runs once per wave: 4 rows of 2,576
    part = torch.rand(P_, K, generator=torch.Generator().manual_seed(0)) + 0.5
    assert P.relerr(emu_partial_sum(part, "drop_term"), emu_partial_sum(part)) < OLD
    lat = P.lattice((17, K), -100, 100, 5).float()
    assert torch.equal(emu_partial_sum(lat), lat.double().sum(0).float())
    assert not torch.equal(emu_partial_sum(lat, "drop_term"), lat.double().sum(0).float())


def test_defect_8_last_maximum():
    x = gauss(2, 17, 15, 8)
    y0, i0 = emu_maxpool(x, 3, 2, 1)
    y1, i1 = emu_maxpool(x, 3, 2, 1, "ge")
    assert P.relerr(y1, y0) < 1e-6 and (i0 == i1).float().mean() > 0.99  # the old test's two criteria
    pr = P.pool_problem(2, 7, 5, 8, 3, 2, 1)
    y0, i0 = emu_maxpool(pr.x, 3, 2, 1)
    y1, i1 = emu_maxpool(pr.x, 3, 2, 1, "ge")
    assert torch.equal(y0, pr.want_y) and torch.equal(i0, pr.idx)
    assert torch.equal(y1, pr.want_y) and not torch.equal(i1, pr.idx)  # the values cannot tell, the argmax does


def test_defect_9_generic_gather_range():
    x, dy = gauss(2, 17, 15, 8), gauss(2, 9, 8, 8, seed=1)
    _, idx = emu_maxpool(x, 3, 2, 1)
    # the old tests call 3x3/2/1 only: the compile-time instantiation, which the defect does not touch
    assert torch.equal(emu_pool_gather(dy, idx, 17, 15, 3, 2, 1, "ho_hi_short"), emu_pool_gather(dy, idx, 17, 15, 3, 2, 1))
    for geo in ((2, 2, 0), (3, 1, 1)):
        pr = P.pool_problem(2, 7, 5, 8, *geo)
        assert torch.equal(emu_pool_gather(pr.dy, pr.idx, 7, 5, *geo), pr.want_dx)
        assert not torch.equal(emu_pool_gather(pr.dy, pr.idx, 7, 5, *geo, "ho_hi_short"), pr.want_dx)


def test_defect_10_dres_scaled_by_the_gate():
    """dres = dz g is far outside the old tolerance wherever the gate is not 1: the old test does catch
    this one (recorded here so the list is complete); the exact check catches it too"""
    N, HW, C = 2, 49, 24
    x, g, r, dy = gauss(N, HW, C), gauss(N, C, seed=1), gauss(N, HW, C, seed=2), gauss(N, HW, C, seed=3)
    _, ref = emu_chan_scale_bwd(dy, x, g, r)
    _, bad = emu_chan_scale_bwd(dy, x, g, r, "dres_g")
    assert P.relerr(bad, ref) > OLD
    cs = P.chan_scale_problem(3, 49, 24)
    c = cs.cases[(True, True)]
    dx, dres = emu_chan_scale_bwd(cs.dy, c.x, cs.gate, c.res)
    assert torch.equal(dx, c.want_dx) and torch.equal(dres, c.want_dres)
    assert not torch.equal(emu_chan_scale_bwd(cs.dy, c.x, cs.gate, c.res, "dres_g")[1], c.want_dres)


@pytest.mark.parametrize("hw,ohw", P.ADAPTIVE)
def test_defect_11_is_an_equivalent_mutant(hw, ohw):
    """Row h lies in cell oh iff floor(oh H / OH) <= h < ceil((oh + 1) H / OH), i.e. iff
    h OH / H - 1 < oh < (h + 1) OH / H: the largest such oh is ceil((h + 1) OH / H) - 1 <=
    floor((h + 1) OH / H).  The ``+ 1`` of ``oh_hi`` (and the ``- 1`` of ``oh_lo``) only widen a scan
    whose extra candidates fail the window test, so dropping it changes no output -- for any H, OH, not
    only these.  No test can fail on it; the exact test pins the result either way."""
    pr = P.adaptive_problem(2, *hw, 8, *ohw)
    a = emu_adaptive_bwd(pr.dy, *hw)
    assert torch.equal(a, emu_adaptive_bwd(pr.dy, *hw, "no_plus1"))
    assert bool(((a == pr.want_dx) | (a == pr.want_dx_fma)).all())
    for H in range(1, 20):
        for OH in range(1, 20):
            for h in range(H):
                top = max(oh for oh in range(OH) if P.ad_cell(oh, H, OH)[0] <= h < P.ad_cell(oh, H, OH)[1])
                assert top <= ((h + 1) * OH) // H
