"""Bit-exact checks of the pooling, channel-scale and layout kernels (csrc/pool.hip, pool_gather.cuh,
the SE half of csrc/extra.hip) against tests/pointwise_oracle.py.

* Max pool: values AND argmax with ``torch.equal`` against the first-maximum-in-window-order rule on
  lattices where most windows hold their maximum more than once; every runtime geometry (the
  ``<0,0,0>`` instantiations VGG's 2x2/2 pool takes) next to the compile-time 3x3/2/1; the backward as
  an exact sum of at most ceil(k/s)^2 lattice values.  The fused BN + ReLU + pool and both its
  backward passes at every channel count ``bn_pool_ok`` admits up to 512.
* Averages (GAP, adaptive): where the divisor is not a power of two the kernels multiply by
  fp32(1/n), so they are held bit for bit to ``bf16(fp32(sum) * fp32(1/n))`` and, per element, to
  the bound two roundings imply against the one-rounding value.
* Channel scale: exact with power-of-two gates, the ReLU boundary at z == 0 included.
"""
import collections

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from tests import pointwise_oracle as P
from tests.test_exact_lattice_gpu import d

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = P.BF16, P.F32
TALLY = collections.Counter()
OFF_ONE = collections.Counter()
NHWC = ("n", "h", "w", "c")


@pytest.fixture(scope="module")
def K():
    ops = _ext.hip_ops()
    yield ops
    print("\n[pool-exact] bit-exact comparisons per kernel:")
    for fam, n in sorted(TALLY.items()):
        print(f"[pool-exact]   {fam}: {n}")
    for fam in sorted(f for f in OFF_ONE if not f.endswith("#n")):
        print(f"[pool-exact]   {fam}: {OFF_ONE[fam]} of {OFF_ONE[fam + '#n']} outputs differ from the one-rounding "
              f"value, all inside the derived bound")


def exact(fam, got, want, what, dims=NHWC):
    P.assert_exact(got, want, dims if got.dim() == len(dims) else None, f"{fam} {what}")
    TALLY[fam] += 1


def two_rounded(fam, got, want, one, bound, what):
    """bit for bit the two-rounding arithmetic, and inside its bound against the one-rounding value"""
    exact(fam, got, want, what)
    g = got.cpu().double()
    assert bool(((g - one).abs() <= bound).all()), f"{fam} {what}: outside the two-rounding bound"
    OFF_ONE[fam] += int((got.cpu() != P.rounded(one.float().double(), BF16)).sum())
    OFF_ONE[fam + "#n"] += got.numel()


# ----------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("geo", P.POOL_GEOS, ids=str)
def test_maxpool_exact(K, geo):
    k, s, p = geo
    for H, W in P.POOL_SIZES:
        if not P.pool_valid(H, W, k, s, p):
            continue
        for C in ((8, 24, 64, 128, 256, 512) if (H, W) == (7, 5) else (8, 24)):
            pr = P.pool_problem(2, H, W, C, k, s, p)
            what = f"{H}x{W}x{C} k{k} s{s} p{p}"
            y, idx = K.maxpool_fwd(d(pr.x), k, s, p)
            exact("maxpool_fwd.y", y, pr.want_y, what)
            exact("maxpool_fwd.argmax", idx, pr.idx, what)
            dx = K.maxpool_bwd(d(pr.dy), d(pr.idx), H, W, k, s, p)
            exact("maxpool_bwd", dx, pr.want_dx, what)


def test_maxpool_grid_stride(K):
    """more than one workgroup per kernel and a row of output pixels that straddles them"""
    for geo in ((3, 2, 1), (2, 2, 0)):
        pr = P.pool_problem(3, 17, 15, 72, *geo)
        y, idx = K.maxpool_fwd(d(pr.x), *geo)
        exact("maxpool_fwd.y", y, pr.want_y, f"17x15x72 {geo}")
        exact("maxpool_fwd.argmax", idx, pr.idx, f"17x15x72 {geo}")
        exact("maxpool_bwd", K.maxpool_bwd(d(pr.dy), idx, 17, 15, *geo), pr.want_dx, f"17x15x72 {geo}")


BN_POOL_C = (8, 16, 32, 64, 128, 256, 512)  # C % 8 == 0 and 256 % (C / 8) == 0, up to 512


@pytest.mark.parametrize("C", BN_POOL_C)
def test_bn_act_maxpool_exact(K, C):
    """BN + ReLU + max pool fused, forward and both backward passes, 256 input rows (1 / count exact).
    From 256 channels on the reduction writes 2 C > 256 partial columns per workgroup."""
    for geo in ((3, 2, 1), (2, 2, 0), (3, 1, 1), (5, 2, 2)):
        for act in (1, 0):
            if act == 0 and geo != (2, 2, 0):
                continue
            N, H, W = 4, 8, 8
            pr = P.bn_pool_problem(N, H, W, C, *geo, act)
            what = f"{N}x{H}x{W}x{C} {geo} act={act}"
            g = [d(t) for t in (pr.scale, pr.shift, pr.mean, pr.invstd)]
            y, idx = K.bn_act_maxpool(d(pr.x), g[0], g[1], act, *geo)
            exact("bn_act_maxpool.y", y, pr.want_y, what)
            exact("bn_act_maxpool.argmax", idx, pr.idx, what)
            sums = K.maxpool_bn_bwd_reduce(d(pr.dy), idx, d(pr.x), *g, act, *geo)
            exact("maxpool_bn_bwd_reduce", sums, pr.want_sums, what, ("which", "c"))
            dx = K.maxpool_bn_bwd_elemt(d(pr.dy), idx, d(pr.x), *g, act, d(pr.want_sums), pr.count, *geo)
            exact("maxpool_bn_bwd_elemt", dx, pr.want_dx, what)


def test_bn_act_maxpool_odd_sizes(K):
    """non-square, odd and smaller-than-window images: the reduction is exact for any row count"""
    for (H, W), geo in (((7, 5), (3, 2, 1)), ((7, 5), (2, 2, 0)), ((17, 15), (3, 2, 1)), ((1, 1), (3, 2, 1)),
                        ((2, 2), (5, 2, 2)), ((17, 15), (2, 1, 0))):
        for C in (64, 256):
            pr = P.bn_pool_problem(3, H, W, C, *geo, 1)
            what = f"3x{H}x{W}x{C} {geo}"
            g = [d(t) for t in (pr.scale, pr.shift, pr.mean, pr.invstd)]
            y, idx = K.bn_act_maxpool(d(pr.x), g[0], g[1], 1, *geo)
            exact("bn_act_maxpool.y", y, pr.want_y, what)
            exact("bn_act_maxpool.argmax", idx, pr.idx, what)
            sums = K.maxpool_bn_bwd_reduce(d(pr.dy), idx, d(pr.x), *g, 1, *geo)
            exact("maxpool_bn_bwd_reduce", sums, pr.want_sums, what, ("which", "c"))


# ----------------------------------------------------------------------------- GAP / channel scale
GAP_SHAPES = [(1, 1, 8), (3, 4, 24), (16, 49, 72), (3, 64, 1000), (1, 3136, 24), (3, 3136, 64), (3, 49, 2040),
              (1, 64, 1032), (16, 49, 320), (1, 3136, 8), (1, 256, 2048)]


def _hw_splits(N, HW, C):
    rpp = 256 // (C // 8)
    S = min((2048 + N - 1) // N, max(1, HW // (4 * rpp)))
    return max(1, min(S, 64))


def test_hw_splits_cover_one_interior_and_64():
    got = {_hw_splits(N, HW, C) for N, HW, C in GAP_SHAPES}
    assert 1 in got and 64 in got and any(1 < s < 64 for s in got), got


@pytest.mark.parametrize("N,HW,C", GAP_SHAPES)
def test_gap_exact(K, N, HW, C):
    pr = P.gap_problem(N, HW, C)
    H, W = (HW // 7, 7) if HW % 7 == 0 else (HW, 1)
    what = f"N={N} HW={HW} C={C} splits={_hw_splits(N, HW, C)}"
    want, one, bound = P.two_roundings(pr.sum, float(HW))
    two_rounded("gap_fwd", K.gap_fwd(d(pr.x.reshape(N, H, W, C))), want, one, bound, what)
    # backward: bf16(fp32(dy * fp32(1/HW))), and with ``add`` one FMA: bf16(fp32(dy * fp32(1/HW) + add))
    dyb = pr.dy.double()[:, None, :].expand(N, HW, C)
    want, one, bound = P.two_roundings(dyb, float(HW))
    got = K.gap_bwd(d(pr.dy), H, W)
    two_rounded("gap_bwd", got.reshape(N, HW, C), want, one, bound, what)
    inv = P.f32_recip(HW)
    pre = (dyb * inv + pr.add.double()).float()  # the fp64 sum of an exact product and an integer: one rounding
    one = dyb / HW + pr.add.double()
    bound = P.U32 * (dyb / HW).abs() + P.U32 * one.abs() * (1 + 1e-6) + 0.5 * P.bf16_ulp(pre.double())
    got = K.gap_bwd(d(pr.dy), H, W, d(pr.add.reshape(N, H, W, C)))
    two_rounded("gap_bwd.add", got.reshape(N, HW, C), pre.to(BF16), one, bound, what)


@pytest.mark.parametrize("N,HW,C", GAP_SHAPES)
def test_chan_scale_exact(K, N, HW, C):
    """y = relu?(x g + res) and its backward (dx, dg in bf16, dres) with power-of-two gates: exact,
    with a share of the elements at z == 0 where relu' is 0"""
    cs = P.chan_scale_problem(N, HW, C)
    dims = ("n", "hw", "c")
    for (relu, has_res), c in cs.cases.items():
        what = f"N={N} HW={HW} C={C} relu={relu} res={has_res}"
        y = K.chan_scale_fwd(d(c.x), d(cs.gate), d(c.res), relu)
        exact("chan_scale_fwd", y, c.want_y, what, dims)
        dx, dg, dres = K.chan_scale_bwd(d(cs.dy), d(c.x), d(cs.gate), d(c.res), relu, has_res)
        exact("chan_scale_bwd.dx", dx, c.want_dx, what, dims)
        exact("chan_scale_bwd.dg", dg, c.want_dg, what, ("n", "c"))
        if has_res:
            exact("chan_scale_bwd.dres", dres, c.want_dres, what, dims)


@pytest.mark.parametrize("N,C,R", [(1, 32, 32), (3, 96, 32), (16, 256, 128), (32, 160, 64)])
def test_se_gate_hidden_exact(K, N, C, R):
    """The SE gate as far as it is exact: h = bf16(relu(p W1^T + b1)) on the lattice (integer sums below
    2^24, integer bias), about half of the sums negative.  The sigmoid half is not a lattice and keeps
    its tolerance test; here it only has to stay inside (0, 1)."""
    from tests import exact_oracle as X

    key = ("se", N, C, R)
    ma, mb = X.pick_ranges(C)
    p = P.lattice((N, C), -ma, ma, P._seed("p", key))
    w1 = P.lattice((R, C), -mb, mb, P._seed("w1", key))
    w2 = P.lattice((C, R), -1, 1, P._seed("w2", key))
    b1 = P.int_vector(R, -200, 200, P._seed("b1", key))
    pre = p.double() @ w1.double().t() + b1.double()
    X.check_lattice(p, w1, C, pre, BF16, bias=b1)
    h, g = K.se_gate_fwd(d(p), d(w1), d(b1), d(w2), None, R)
    exact("se_gate_fwd.h", h, P.rounded(torch.relu(pre), BF16), f"N={N} C={C} R={R}", ("n", "r"))
    assert bool(((g.float() >= 0) & (g.float() <= 1)).all()) and not torch.isnan(g.float()).any()


# ----------------------------------------------------------------------------- adaptive average pool
@pytest.mark.parametrize("hw,ohw", P.ADAPTIVE, ids=str)
def test_adaptive_avg_pool_exact(K, hw, ohw):
    for C in (8, 72):
        pr = P.adaptive_problem(2, *hw, C, *ohw)
        what = f"{hw}->{ohw} C={C}"
        two_rounded("adaptive_avg_pool", K.adaptive_avg_pool(d(pr.x), *ohw), pr.want_y, pr.one_y, pr.bound_y, what)
        dx = K.adaptive_avg_pool_bwd(d(pr.dy), *hw)
        g = dx.cpu()
        # a pixel in several cells with inexact 1 / cnt: the product rounded, or contracted into the sum --
        # the compiled kernel has ONE form, so the whole tensor must equal one of the two models
        if not (torch.equal(g, pr.want_dx) or torch.equal(g, pr.want_dx_fma)):
            raise AssertionError(f"adaptive_avg_pool_bwd {what}: equals neither model\nproduct rounded: "
                                 + P.mismatch_report(g, pr.want_dx, NHWC) + "\ncontracted: "
                                 + P.mismatch_report(g, pr.want_dx_fma, NHWC))
        assert bool(((g.double() - pr.one_dx).abs() <= pr.bound_dx).all()), f"adaptive_avg_pool_bwd {what}: bound"
        TALLY["adaptive_avg_pool_bwd"] += 1
        OFF_ONE["adaptive_avg_pool_bwd"] += int((g != P.rounded(pr.one_dx.float().double(), BF16)).sum())
        OFF_ONE["adaptive_avg_pool_bwd#n"] += g.numel()


# ----------------------------------------------------------------------------- space to depth
@pytest.mark.parametrize("b,shape", [(2, (2, 6, 10, 8)), (4, (1, 8, 12, 8)), (2, (3, 2, 2, 24))])
def test_space_to_depth_exact(K, b, shape):
    N, H, W, C = shape
    x = P.lattice(shape, -127, 127, P._seed("s2d", b, shape))
    want = x.reshape(N, H // b, b, W // b, b, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // b, W // b, b * b * C)
    y = K.space_to_depth(d(x), b, False)
    exact("space_to_depth", y, want.contiguous(), f"b={b} {shape}")
    exact("space_to_depth.inverse", K.space_to_depth(y, b, True), x, f"b={b} {shape}")
