"""Per-element and per-channel checks of the BatchNorm kernels (csrc/bn.hip, act_bwd of misc.hip).

Elementwise kernels run on the exact problems of tests/pointwise_oracle.py (power-of-two scales,
integer shifts, small-integer activations): every intermediate is an fp32 number, the only correct
output is one bf16 rounding of the exact value, and the comparison is ``torch.equal`` -- at channel
counts whose C/8 does not divide 256 (idle row slots), at row counts around the row-slot count and
around the 4-deep unroll, with >= 5 % of the elements exactly at z == 0.

Statistics are compared per channel with fp64 against bounds derived from the length of each
route's chain of fp32 operations (``pointwise_oracle.stat_chain`` / ``stat_bounds``); the measured
maxima are printed at the end of the module.

The mask bits of bn_act_mask / bn2_act_mask are the ReLU mask ``z > 0`` for every activation (only
ReLU layers ask for them); the boundary test ties them to the backward kernels' own decision.
"""
import collections
import math

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from tests import pointwise_oracle as P
from tests.test_exact_lattice_gpu import d, slots

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = P.BF16, P.F32
SLOPE = P.LEAKY_SLOPE
TALLY = collections.Counter()
ROOM = {}  # route -> [max |mean err| / bound, max |M2 err| / bound]


@pytest.fixture(scope="module")
def K():
    ops = _ext.hip_ops()
    yield ops
    print("\n[bn-exact] bit-exact comparisons per kernel:")
    for fam, n in sorted(TALLY.items()):
        print(f"[bn-exact]   {fam}: {n}")
    print("[bn-exact] statistics: largest measured error as a share of the derived bound, per route")
    for route, (a, b, D) in sorted(ROOM.items()):
        print(f"[bn-exact]   {route}: mean {a:.3%}  M2 {b:.3%}  (longest chain D = {D})")


def exact(fam, got, want, C, what):
    P.assert_pointwise(got, want, C, f"{fam} {what}")
    TALLY[fam] += 1


def _plan(C):
    """(rows, tuning slots): the default grid at every row count; one workgroup / three workgroups at
    4 rpi g + 3 rows (the 4-deep loop once, then the tail loop for three row slots); one row per thread"""
    r = P.rpi_of(C)
    out = [(M, ()) for M in P.bn_rows(C)]
    out += [(4 * r + 3, (("ew_grid_cap", 1), ("bn_bwd_cap", 1))), (12 * r + 3, (("ew_grid_cap", 3),)),
            (12 * r + 3, (("ew_grid_cap", 1), ("bn_bwd_cap", 1))), (r + 1, (("ew_rows", 1),))]
    return out


def _dev(b):
    return {k: d(getattr(b, k)) for k in ("x", "x_res", "dy", "res", "res2", "scale", "shift", "rscale", "rshift",
                                          "mean", "invstd")}


def _forward_and_eval_backward(K, b, g, act, res, what):
    C = b.C
    c = P.bn_case(b, act, res)
    x, r = g["x_res" if res else "x"], g["res"] if res else None
    y = K.bn_act(x, r, g["scale"], g["shift"], act, SLOPE)
    exact("bn_act", y, c.want_y, C, what)
    y2, mask = K.bn_act_mask(x, r, g["scale"], g["shift"], act, SLOPE)
    exact("bn_act_mask.y", y2, c.want_y, C, what)
    exact("bn_act_mask.mask", mask, c.want_mask, C, what)
    sums = K.bn_bwd_reduce(g["dy"], x, r, g["scale"], g["shift"], g["mean"], g["invstd"], act, SLOPE, False)
    exact("bn_bwd_reduce", sums, c.want_sums, C, what)
    dx, dres = K.bn_bwd_elemt(g["dy"], x, r, g["scale"], g["shift"], g["mean"], g["invstd"], None, 1.0, act, SLOPE,
                              True, False, None)
    exact("bn_bwd_elemt.eval.dx", dx, c.want_dx, C, what)
    exact("bn_bwd_elemt.eval.dres", dres, c.want_dres, C, what)
    if res:
        c2 = P.bn_case(b, act, True, two=True)
        y3, m3 = K.bn2_act_mask(x, g["res2"], g["scale"], g["shift"], g["rscale"], g["rshift"], act, SLOPE)
        exact("bn2_act_mask.y", y3, c2.want_y, C, what)
        exact("bn2_act_mask.mask", m3, c2.want_mask, C, what)


@pytest.mark.parametrize("C", P.BN_C)
def test_elementwise_forward_and_eval_backward(K, C):
    for M, cfg in _plan(C):
        b = P.bn_base(C, M)
        g = _dev(b)
        with slots(K, cfg):
            for act in P.ACTS:
                for res in (False, True):
                    _forward_and_eval_backward(K, b, g, act, res, f"C={C} M={M} act={act} res={res} {dict(cfg)}")


@pytest.mark.parametrize("M,rows", [(8192 + 5, 4), (4096 + 5, 2)])
def test_default_grids(K, M, rows):
    """the two default elementwise grids at C = 2048 (one row slot): 4 rows per thread from 2,048
    workgroups up (8,197 rows: 2,050 workgroups, the 4-deep loop and the tail loop), 2 rows below"""
    C = 2048
    g4 = math.ceil(M / 4)  # ew_grid (bn.hip): 4 rows per thread where that leaves >= 2,048 workgroups; the library
    assert (g4 >= 2048) == (rows == 4)  # does not report the launched grid, so a change of that rule must change this
    b = P.bn_base(C, M)
    _forward_and_eval_backward(K, b, _dev(b), 1, True, f"C={C} M={M} default grid")


@pytest.mark.parametrize("C", P.BN_C)
def test_training_backward_exact(K, C):
    """bn_bwd_reduce + bn_bwd_elemt (dx, dres), bn2_bwd_elemt and the InplaceABN ``inv`` forms with a
    power-of-two row count: dx = ca dz + cb x + cc is one bf16 rounding of an exact number"""
    for M in P.bwd_rows(C):
        b = P.bn_base(C, M, small=True)
        g = _dev(b)
        for cfg in ((), (("ew_grid_cap", 1), ("bn_bwd_cap", 1))):
            with slots(K, cfg):
                for act in P.ACTS:
                    for res in (False, True):
                        what = f"C={C} M={M} act={act} res={res} {dict(cfg)}"
                        c = P.bn_case(b, act, res, count=float(M))
                        x, r = g["x_res" if res else "x"], g["res"] if res else None
                        sums = K.bn_bwd_reduce(g["dy"], x, r, g["scale"], g["shift"], g["mean"], g["invstd"], act,
                                               SLOPE, False)
                        exact("bn_bwd_reduce", sums, c.want_sums, C, what)
                        dx, dres = K.bn_bwd_elemt(g["dy"], x, r, g["scale"], g["shift"], g["mean"], g["invstd"], sums,
                                                  float(M), act, SLOPE, True, False, None)
                        exact("bn_bwd_elemt.dx", dx, c.want_dx, C, what)
                        exact("bn_bwd_elemt.dres", dres, c.want_dres, C, what)
                for act in (0, 2):
                    what = f"C={C} M={M} act={act} inv {dict(cfg)}"
                    c = P.bn_case(b, act, False, count=float(M), inv=True)
                    sums = K.bn_bwd_reduce(g["dy"], g["x"], None, g["scale"], g["shift"], g["mean"], g["invstd"], act,
                                           SLOPE, True)
                    exact("bn_bwd_reduce.inv", sums, c.want_sums, C, what)
                    graw = P.int_vector(C, -1, 1, 7)
                    dx, dg = K.bn_bwd_elemt(g["dy"], g["x"], None, g["scale"], g["shift"], g["mean"], g["invstd"],
                                            sums, float(M), act, SLOPE, False, True, d(graw))
                    exact("bn_bwd_elemt.inv.dx", dx, c.want_dx, C, what)
                    exact("bn_bwd_elemt.inv.dg", dg, c.want_sums[1] * torch.sign(graw), C, what)
                two = P.bn2_case(b)
                dx, dr = K.bn2_bwd_elemt(g["dy"], g["x"], d(two.r), g["scale"], g["mean"], g["invstd"], d(two.sums),
                                         d(two.rscale), d(two.rmean), d(two.rinvstd), d(two.rsums), float(M))
                exact("bn2_bwd_elemt.dx", dx, two.want_dx, C, f"C={C} M={M} {dict(cfg)}")
                exact("bn2_bwd_elemt.dr", dr, two.want_dr, C, f"C={C} M={M} {dict(cfg)}")


@pytest.mark.parametrize("C", [8, 64, 2048])
def test_act_scale_bwd_and_act_bwd(K, C):
    """backward from the stored OUTPUT y (its zeros, +0.0 and -0.0, are the boundary): ReLU passes the
    gradient where y > 0, leaky where y >= 0"""
    for M, cfg in _plan(C):
        b = P.bn_base(C, M)
        for act in P.ACTS:
            c = P.bn_case(b, act, False)
            y, dy = c.want_y, b.dy
            yd = y.double()
            rule = {0: torch.ones_like(yd), 1: (yd > 0).double(), 2: torch.where(yd >= 0, 1.0, SLOPE)}[act]
            gk = dy.double() * rule
            with slots(K, cfg):
                for want_g in (False, True):
                    dc, g = K.act_scale_bwd(d(dy), d(y), d(b.scale), act, SLOPE, want_g)
                    exact("act_scale_bwd.dc", dc, P.rounded(gk * b.scale.double(), BF16), C, f"C={C} M={M} act={act}")
                    if want_g:
                        exact("act_scale_bwd.g", g, P.rounded(gk, BF16), C, f"C={C} M={M} act={act}")
                if act == 1:
                    exact("act_bwd", K.act_bwd(d(dy), d(y), 1), P.rounded(gk, BF16), C, f"C={C} M={M}")


@pytest.mark.parametrize("C", [8, 72, 1000])
def test_activation_boundary_agreement(K, C):
    """One exact problem, five deciders: the oracle's z, the forward's mask bits, the stored output y
    (the rule act_scale_bwd applies), and the elements bn_bwd_elemt treats as active (read off dres).
    ReLU: active iff z > 0; leaky: full slope iff z >= 0 -- z == -0.0 included."""
    M = 4 * P.rpi_of(C) + 3
    b = P.bn_base(C, M)
    g = _dev(b)
    dy1 = torch.ones_like(b.dy)  # dres = act'(z) itself
    for res in (False, True):
        x, r = g["x_res" if res else "x"], g["res"] if res else None
        for act in (1, 2):
            c = P.bn_case(b, act, res)
            want = (c.z > 0) if act == 1 else (c.z >= 0)
            assert (c.z == 0).double().mean() >= 0.05
            y, mask = K.bn_act_mask(x, r, g["scale"], g["shift"], act, SLOPE)
            _, dres = K.bn_bwd_elemt(d(dy1), x, r, g["scale"], g["shift"], g["mean"], g["invstd"], None, 1.0, act,
                                     SLOPE, True, False, None)
            active = (dres.cpu().double() == 1.0)
            assert torch.equal(active, want), f"backward's active set != oracle (C={C} act={act} res={res})"
            yc = y.cpu().double()
            assert torch.equal((yc > 0) if act == 1 else (yc >= 0), want), "rule on the stored output != oracle"
            if act == 1:
                assert torch.equal(mask.cpu(), P.mask_bytes(active)), "mask bits != backward's active set"
            TALLY["boundary"] += 1


@pytest.mark.parametrize("C", P.BN_C)
def test_bn_fin_act_every_act_and_residual(K, C):
    """bn_fin_act (finalize + apply in one launch of 1024-thread workgroups, four virtual row tiles each)
    for every act x residual, with and without mask bits, at every channel count -- idle row slots in each
    virtual tile, coefficients staged through LDS -- from synthesised slabs and from given partials:
    bit for bit its two launches, bn_stats_finalize + bn_act_mask / bn_act (pinned exactly above), the
    running statistics too, and no spin timeout."""
    r = P.rpi_of(C)
    gamma, beta = d(P.pow2_scales(C, 13, exps=(-1, 0, 1))), d(P.int_vector(C, -3, 3, 14))
    rm0, rv0 = P.int_vector(C, -2, 2, 15), P.int_vector(C, 1, 3, 16)
    for M, kind in ((12 * r + 3, "slabs"), (4 * r + 3, "partials"), (max(1, r - 1), "slabs"), (16 * r + 1, "partials")):
        x = P.stat_rows(M, C)
        res = d(P.lattice((M, C), -100, 100, P._seed("finres", M, C)))
        src = d(P.slabs_of(x)) if kind == "slabs" else d(P.partials_of(x, 5, (1,)))
        xd = d(x)
        for act in P.ACTS:
            for rd in (None, res):
                for want_mask in (True, False):
                    what = f"C={C} M={M} {kind} act={act} res={rd is not None} mask={want_mask}"
                    before = K.bn_fin_act_timeouts(xd)
                    rm, rv = d(rm0.clone()), d(rv0.clone())
                    y, mask, *coef = K.bn_fin_act(xd, src, rd, gamma, beta, rm, rv, 0.1, 1e-5, act, SLOPE, want_mask)
                    assert K.bn_fin_act_timeouts(xd) == before, f"{what}: spin timeout"
                    rm2, rv2 = d(rm0.clone()), d(rv0.clone())
                    ref = K.bn_stats_finalize(xd, src, gamma, beta, rm2, rv2, 0.1, 1e-5)
                    for name, a, b in zip(("mean", "invstd", "scale", "shift"), coef, ref):
                        assert torch.equal(a, b), f"{what}: {name} differs from bn_stats_finalize"
                    assert torch.equal(rm, rm2) and torch.equal(rv, rv2), f"{what}: running statistics"
                    if want_mask:
                        y2, mask2 = K.bn_act_mask(xd, rd, ref[2], ref[3], act, SLOPE)
                        exact("bn_fin_act.mask", mask, mask2, C, what)
                    else:
                        y2 = K.bn_act(xd, rd, ref[2], ref[3], act, SLOPE)
                        assert mask.numel() == 0
                    exact("bn_fin_act.y", y, y2, C, what)


# ----------------------------------------------------------------------------- statistics
def _check_stats(route, st, x, D, what):
    """st [3, C] (n, mean, M2) against fp64, per channel"""
    n, mu, m2, bm, b2 = P.stat_bounds(x, D)
    st = st.detach().cpu().double().reshape(3, -1)
    assert bool((st[0] == n).all()), f"{what}: n {st[0].unique().tolist()} != {n}"
    assert not torch.isnan(st).any(), f"{what}: NaN"
    em, e2 = (st[1] - mu).abs(), (st[2] - m2).abs()
    # |mean - mu| <= Km u (|mu| + sigma), |M2 - M2*| <= K2 u M2* (stat_bounds: Km = 2 D T,
    # K2 = 2 D (4 T^2 + 4 T (|mu| / sigma + T)), D = stat_chain(route): derived, not measured)
    bad_m, bad_2 = (em > bm).nonzero().flatten().tolist(), (e2 > b2).nonzero().flatten().tolist()
    assert not bad_m, f"{what}: mean outside its bound in channels {bad_m[:8]}: {em[bad_m[:8]].tolist()} > {bm[bad_m[:8]].tolist()}"
    assert not bad_2, f"{what}: M2 outside its bound in channels {bad_2[:8]}: {e2[bad_2[:8]].tolist()} > {b2[bad_2[:8]].tolist()}"
    live = b2 > 0
    room = ROOM.setdefault(route, [0.0, 0.0, 0])
    room[0] = max(room[0], (em[bm > 0] / bm[bm > 0]).max().item() if (bm > 0).any() else 0.0)
    room[1] = max(room[1], (e2[live] / b2[live]).max().item() if live.any() else 0.0)
    room[2] = max(room[2], D)
    TALLY["stats." + route] += 1
    return n, mu, m2, b2


def _ulps(got, want64):
    """|got - want| in units of the fp32 spacing at want"""
    w = want64.double()
    ulp = torch.exp2(torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -126))) - 23)
    return ((got.detach().cpu().double() - w).abs() / ulp).max().item()


def _finalize_agreement(K, x, src, st, what, eps=1e-5, fin_act=True):
    """bn_finalize(bn_stats(.)), bn_stats_finalize and bn_fin_act (one launch, and as its two launches)
    on the same source: the same merge order and the same finalize code -- bit for bit, running
    statistics included.  Then invstd / scale / shift against fp64 from the kernel's own (mean, M2)."""
    C = x.shape[-1]
    gamma, beta = d(P.pow2_scales(C, 3, exps=(-1, 0, 1))), d(P.int_vector(C, -3, 3, 4))
    rm0, rv0 = P.int_vector(C, -2, 2, 5), P.int_vector(C, 1, 3, 6)
    outs = []
    run = []
    rm, rv = d(rm0.clone()), d(rv0.clone())
    outs.append(K.bn_finalize(st, gamma, beta, rm, rv, 0.1, eps))
    run.append((rm, rv))
    rm, rv = d(rm0.clone()), d(rv0.clone())
    outs.append(K.bn_stats_finalize(x, src, gamma, beta, rm, rv, 0.1, eps))
    run.append((rm, rv))
    if fin_act and src is not None:
        before = K.bn_fin_act_timeouts(x)
        ys = []
        for mode in (0, 2):
            rm, rv = d(rm0.clone()), d(rv0.clone())
            with slots(K, (("bn_fin_act", mode),) if mode else ()):
                y, mask, *coef = K.bn_fin_act(x, src, None, gamma, beta, rm, rv, 0.1, eps, 1, 0.0, True, -1.0, None)
            outs.append(tuple(coef))
            run.append((rm, rv))
            ys.append((y, mask))
        assert K.bn_fin_act_timeouts(x) == before, f"{what}: bn_fin_act spin timeout"
        assert torch.equal(ys[0][0], ys[1][0]) and torch.equal(ys[0][1], ys[1][1]), f"{what}: bn_fin_act y / mask"
        # y against fp64 from the kernel's own coefficients: one fp32 rounding of x scale (or none, fused),
        # one of the sum, then half a bf16 ulp
        sc, sh = outs[-1][2].cpu().double(), outs[-1][3].cpu().double()
        z = x.cpu().double().reshape(-1, C) * sc + sh
        e32 = 2 * P.U32 * ((x.cpu().double().reshape(-1, C) * sc).abs() + sh.abs())
        yw = torch.relu(z)
        err = (ys[0][0].cpu().double().reshape(-1, C) - yw).abs()
        assert bool((err <= e32 + 0.5 * P.bf16_ulp(yw + e32)).all()), f"{what}: bn_fin_act y outside half a bf16 ulp"
        zc = z.abs() > e32  # the mask bit is decided where z is clear of zero
        mb = P.mask_bytes(z > 0)
        got_bits = ys[0][1].cpu().reshape(-1, C // 8)
        same = ((got_bits[..., None] >> torch.arange(8)) & 1) == ((mb[..., None] >> torch.arange(8)) & 1)
        assert bool((same.reshape(-1, C) | ~zc).all()), f"{what}: bn_fin_act mask bits"
        TALLY["bn_fin_act"] += 1
    for i, (o, r) in enumerate(zip(outs[1:], run[1:]), 1):
        for j, name in enumerate(("mean", "invstd", "scale", "shift")):
            assert torch.equal(o[j], outs[0][j]), f"{what}: {name} of path {i} differs from bn_finalize(bn_stats)"
        assert torch.equal(r[0], run[0][0]) and torch.equal(r[1], run[0][1]), f"{what}: running stats of path {i}"
    TALLY["finalize.agree"] += 1
    n, mean, m2 = (t.cpu().double() for t in st.reshape(-1, 3, C)[0]) if st.shape[0] == 1 else (None, None, None)
    if n is not None:
        var = m2 / n
        want_is = 1 / (var + float(torch.tensor(eps, dtype=F32))).sqrt()
        assert _ulps(outs[0][1], want_is) <= 4, f"{what}: invstd"  # /, +, rsqrt (about 1 ulp) and its input's rounding
        unb = torch.where(n > 1, m2 / (n - 1).clamp_min(1), var)
        assert torch.allclose(run[0][1].cpu().double(), 0.9 * rv0.double() + 0.1 * unb, rtol=4 * P.U32, atol=1e-30)
        assert torch.allclose(run[0][0].cpu().double(), 0.9 * rm0.double() + 0.1 * mean, rtol=4 * P.U32,
                              atol=4 * P.U32 * float(mean.abs().max()) + 1e-30)
    return outs[0]


RAW = [(8, 1), (24, 1), (24, 50), (72, 896), (320, 100), (1000, 300), (1032, 77), (2040, 33), (2048, 8200)]


@pytest.mark.parametrize("C,M", RAW)
def test_stats_raw_route(K, C, M):
    """one row, fewer rows than row slots, a single partial, several partials, the 256-partial cap"""
    x = P.stat_rows(M, C)
    rpi = P.rpi_of(C)
    Pn = min(256, max(1, math.ceil(M / (rpi * 32))))
    D = P.stat_chain("raw", L=math.ceil(M / (Pn * rpi)), rpi=rpi, P=Pn)
    st = K.bn_stats(d(x), None)
    _check_stats("raw", st[0], x, D, f"raw C={C} M={M}")
    sc = st[0].cpu()
    assert sc[2, 0] == 0 and sc[2, 1] == 0 and sc[1, 1] == 0, "constant / all-zero channel: M2 must be exactly 0"
    assert sc[1, 0] == 37.0
    mean, invstd, scale, shift = _finalize_agreement(K, d(x), None, st, f"raw C={C} M={M}")
    eps32 = torch.tensor(1e-5, dtype=F32).double()
    assert _ulps(invstd[:2], (1 / eps32.sqrt()).expand(2)) <= 1, "constant channel: invstd != rsqrt(eps) to 1 ulp"
    assert not any(torch.isnan(t).any() for t in (mean, invstd, scale, shift))


SLAB_R = (1, 63, 64, 65, 511, 512, 513, 1024, 1025, 1089)


@pytest.mark.parametrize("R", SLAB_R)
def test_stats_slab_routes(K, R):
    """slabs synthesised per 128 rows in fp64 (no conv needed): the one-level merge up to 1,024 slabs,
    64 slabs per split above; last slab of 128, 1 and 127 rows; 8 and 24 channels (ragged 16-channel
    finalize groups)"""
    for tail, C in ((128, 8), (1, 24), (127, 8)):
        M = 128 * (R - 1) + tail
        x = P.stat_rows(M, C)
        slabs = d(P.slabs_of(x))
        xd = d(x)
        if R <= 1024:
            route, D = "slab.direct", P.stat_chain("direct", R=R)
        else:
            Pn = math.ceil(R / 64)
            route, D = "slab.split", P.stat_chain("split", tps=math.ceil(R / Pn), P=Pn)
        st = K.bn_stats(xd, slabs)
        _check_stats(route, st[0], x, D, f"{route} R={R} M={M} C={C}")
        assert st[0, 2, 0] == 0 and st[0, 2, 1] == 0, "constant channel: equal slab means, M2 stays 0"
        _finalize_agreement(K, xd, slabs, st, f"{route} R={R} M={M} C={C}", fin_act=R in (1, 65, 513, 1025))


@pytest.mark.parametrize("Pn", [1, 15, 16, 17, 48, 49, 64, 65, 256, 257, 385])
def test_stats_given_partials(K, Pn):
    C, M = 24, 3 * Pn + 40
    x = P.stat_rows(M, C)
    empty = () if Pn < 15 else (0, 7, Pn - 1)
    part = d(P.partials_of(x, Pn, empty))
    xd = d(x)
    st = K.bn_stats(xd, part)
    _check_stats("given", st[0], x, P.stat_chain("given", P=Pn), f"given P={Pn}")
    _finalize_agreement(K, xd, part, st, f"given P={Pn}", fin_act=Pn in (17, 65, 257))


@pytest.mark.parametrize("W", [1, 2, 8])
def test_bn_finalize_ranks(K, W):
    """bn_finalize over W ranks, one of them empty: (mean, invstd) of the union of the rows"""
    C, M = 24, 200
    x = P.stat_rows(M, C)
    st = P.partials_of(x, W, (1,) if W > 1 else ())
    mean, invstd, scale, shift = K.bn_finalize(d(st), None, None, None, None, 0.1, 1e-5)
    n, mu, m2, bm, b2 = P.stat_bounds(x, P.stat_chain("ranks", W=W))
    assert bool(((mean.cpu().double() - mu).abs() <= bm).all())
    var_lo, var_hi = (m2 - b2) / n, (m2 + b2) / n
    e = float(torch.tensor(1e-5, dtype=F32))
    lo, hi = 1 / (var_hi + e).sqrt(), 1 / (var_lo + e).sqrt()
    got = invstd.cpu().double()
    assert bool(((got >= lo * (1 - 4 * P.U32)) & (got <= hi * (1 + 4 * P.U32))).all())
    assert torch.equal(scale, invstd) and not torch.isnan(shift).any()
    TALLY["bn_finalize.ranks"] += 1


def test_running_stats_single_row_and_iabn_gamma(K):
    """n = 1: the unbiased variance falls back to the biased one (0), no division by zero;
    iabn_eps >= 0: effective weight |gamma| + eps for negative and zero gamma, reciprocal finite"""
    C = 24
    x = P.stat_rows(1, C)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    gamma = P.int_vector(C, -2, 2, 11)
    gamma[:3] = torch.tensor([0.0, -1.0, -0.0])
    rg = torch.empty(C, device=DEV)
    ie = 2.0 ** -10
    mean, invstd, scale, shift = K.bn_stats_finalize(d(x), None, d(gamma), None, rm, rv, 0.5, 1e-5, ie, rg)
    assert torch.equal(mean.cpu(), x[0].float())
    assert torch.equal(rv.cpu(), torch.full((C,), 0.5)) and torch.equal(rm.cpu(), 0.5 * x[0].float())
    geff = gamma.abs().double() + ie
    assert torch.equal(rg.cpu().double(), (1 / geff).float().double()) and bool((rg > 0).all())
    assert _ulps(scale, geff * invstd.cpu().double()) <= 1 and bool((scale > 0).all())
    assert not torch.isnan(shift).any()
    TALLY["iabn_gamma"] += 1


# ----------------------------------------------------------------------------- reductions exact on the lattice
PART_P = (1, 3, 4, 13, 16, 17, 61, 64, 65, 128)


@pytest.mark.parametrize("Pn", PART_P)
def test_colsum_exact(K, Pn):
    """colsum -> partial_sum over Pn = ceil(M / 16) partials: integer sums, exact in any order"""
    M = 16 * Pn - 5
    for C in (8, 24, 1000, 2056):
        x = P.lattice((M, C), -127, 127, P._seed("colsum", M, C))
        want = x.double().sum(0)
        P.need_fp32(colsum=want)
        exact("colsum", K.colsum(d(x)), want.float(), C, f"M={M} C={C} P={Pn}")


@pytest.mark.parametrize("Pn", PART_P + (512,))
def test_bn_bwd_reduce_partials_exact(K, Pn):
    """bn_bwd_reduce -> partial_sum over Pn workgroup partials of 2 C columns (C = 1000: two row slots,
    250 live threads); Pn = 512 through a lowered bn_bwd_cap, the branch the 512-workgroup cap takes"""
    C = 1000
    cfg = ()
    if Pn == 512:
        Pn, cfg, M = 5, (("bn_bwd_cap", 5),), 2 * 32 * 6 + 1
    else:
        M = 8 * Pn - 3
    b = P.bn_base(C, M)
    c = P.bn_case(b, 1, True)
    with slots(K, cfg):
        sums = K.bn_bwd_reduce(d(b.dy), d(b.x_res), d(b.res), d(b.scale), d(b.shift), d(b.mean), d(b.invstd), 1, 0.0,
                               False)
    exact("bn_bwd_reduce.partials", sums, c.want_sums, C, f"M={M} P={Pn} {dict(cfg)}")
