"""Bit-exact checks of the fused stem backward (csrc/stem.hip: stem_bwd_kernel<W>, stem_bwd_sums, stem_bwd_dw)
and the stem weight's index maps (csrc/misc.hip: s2d_weight, s2d_weight_bwd) against tests/stem_bwd_oracle.py.

``tot`` and ``sums`` of every case are compared with ``torch.equal`` on the integer lattice of the oracle.
The launcher runs nb = min(N H, CUs) workgroups over rpb = ceil(N H / nb) consecutive rows (n, y) each, so the
batch of every case is derived from the device's CU count and the rows-per-workgroup it is meant to reach is
asserted, not assumed.  Per case family (R = N H rows; "ring" = steady-state loop with ring-slot reuse,
"cross" = workgroups that start mid-image or span images, "empty" = workgroups without rows, "g0 == g1" = a
workgroup that starts exactly at R; kTail16 widths are 16, 48, 80, 112, the others 32, 56, 64, 96; the half
tile is W = 56):

  test_one_row_per_workgroup   every W, N 1, H 4, act 0 / 1: rpb 1.  kTail16 and not, half tile; prologue and
                               epilogue intervals only, image top and bottom rows.
  test_steady_state            every W, H 2, N = CUs + 1, act 0 / 1: rpb 3.  ring (t + 3 loads), cross
                               (workgroups start on alternating row parity, every one spans two images),
                               empty (the last third), short last workgroup, kTail16, half tile; H 2 (Ho 1:
                               every odd row is the last row, h1 clamped) at W 112 and W 56 among them.
  test_ring_wraps              W 16, H 10, R > 8 CUs: rpb >= 9, H % rpb != 0.  ring through all 8 slots and
                               round again, cross, kTail16; called twice for run-to-run determinism.
  test_ring_wraps_min_height   W 16, H 2, R > 8 CUs: rpb >= 9.  ring, cross (4 to 5 images per workgroup).
  test_rows_per_group_near_H   W 32, H 6, rpb 5, 6, 7: rpb == H is the training alignment (every workgroup
                               one whole image), H - 1 and H + 1 drift through every starting row.  ring, cross.
  test_empty_and_short_groups  W 16, H 2, R = CUs + 2: rpb 2, about half the workgroups empty and one with
                               g0 == g1; the partial buffer is uninitialised memory, so they must write zeros.
  test_gather_families         W 32, H 4, rpb 3: |dy| <= 200 (the gathered sum passes 256 and is rounded to
                               bf16, ties included), every window on its bottom-right tap, four windows on
                               one pixel, and the last two combined.  ring, cross.
  test_localised_rows          W 16, H 10, rpb >= 9: x16 nonzero in ONE image row, g' nonzero in ONE image
                               row.  A stale or mis-slotted ring row then is a named (ty, tx, c) column.

stem_bwd_dw is compared bit for bit where every intermediate of its formula is an fp32 number, and otherwise
held per element to the bound that follows from the formula (``S.dw_bound``), against both the algebraic form
and the independent textbook sum over dz X (which pins the (ty, tx, c) layout of the output).
"""
import collections
import math

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import stem_bwd_oracle as S
from tests.exact_oracle import BF16, F32, assert_exact, lattice, int_vector, pow2_scales, rounded, _seed
from tests.pointwise_oracle import need_fp32

pytestmark = pytest.mark.gpu

DEV = "cuda"
TALLY = collections.Counter()


def d(t):
    return t.to(DEV)


@pytest.fixture(scope="module")
def K():
    ops = _ext.hip_ops()
    yield ops
    print("\n[stem-bwd-exact] bit-exact comparisons per kernel:")
    for fam, n in sorted(TALLY.items()):
        print(f"[stem-bwd-exact]   {fam}: {n}")


@pytest.fixture(scope="module")
def cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run(K, pr):
    return K.stem_bn_pool_bwd(d(pr.dy), d(pr.idx), d(pr.z), d(pr.x16), d(pr.scale), d(pr.shift), d(pr.mean),
                              d(pr.invstd), pr.act)


def check(K, pr, what):
    """tot piece by piece (a mismatch names its (co, ty, tx, c)), then as a whole, and sums"""
    tot, sums = run(K, pr)
    what = f"W={pr.W} H={pr.H} N={pr.N} act={pr.act} {pr.family} {what}"
    got, want = S.split_tot(tot), S.split_tot(pr.want_tot)
    for name in got:
        assert_exact(got[name][0], want[name][0], got[name][1], f"stem_bwd_kernel<{pr.W}> {name} {what}")
    assert_exact(tot, pr.want_tot, None, f"stem_bwd_kernel<{pr.W}> tot {what}")
    assert_exact(sums, pr.want_sums, ("which", "co"), f"stem_bwd_sums {what}")
    TALLY[f"stem_bwd_kernel<{pr.W}>"] += 1
    TALLY["stem_bwd_sums"] += 1
    return tot, sums


def geometry(N, H, cu, want_rpb=None, min_rpb=None):
    nb, rpb = S.launch_geometry(N, H, cu)
    if want_rpb is not None:
        assert rpb == want_rpb, f"N={N} H={H} on {cu} CUs: rpb {rpb}, the case is meant for {want_rpb}"
    if min_rpb is not None:
        assert rpb >= min_rpb, f"N={N} H={H} on {cu} CUs: rpb {rpb}, the case is meant for >= {min_rpb}"
    return nb, rpb


# ----------------------------------------------------------------------------- stem_bwd_kernel
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("W", S.WIDTHS)
def test_one_row_per_workgroup(K, cu, W, act):
    assert cu >= 4
    geometry(1, 4, cu, want_rpb=1)
    check(K, S.problem(1, 4, W, act), "rpb=1")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("W", S.WIDTHS)
def test_steady_state(K, cu, W, act):
    N, H = cu + 1, 2
    nb, rpb = geometry(N, H, cu, want_rpb=3)
    assert -(-(N * H) // rpb) < nb  # trailing workgroups without rows
    check(K, S.problem(N, H, W, act), "rpb=3")


def _ring_shape(cu):
    N, H = 8 * cu // 10 + 1, 10
    nb, rpb = geometry(N, H, cu, min_rpb=9)
    assert N * H > 8 * cu and H % rpb != 0
    return N, H, nb, rpb


def test_ring_wraps(K, cu):
    N, H, nb, rpb = _ring_shape(cu)
    pr = S.problem(N, H, 16, 1)
    tot, _ = check(K, pr, f"rpb={rpb}")
    again, _ = run(K, pr)
    assert torch.equal(again, tot), "two calls on the same inputs differ"


def test_ring_wraps_min_height(K, cu):
    N, H = 4 * cu + 1, 2
    nb, rpb = geometry(N, H, cu, min_rpb=9)
    check(K, S.problem(N, H, 16, 1), f"rpb={rpb}")


@pytest.mark.parametrize("rpb", [5, 6, 7])
def test_rows_per_group_near_H(K, cu, rpb):
    H = 6
    N = rpb * cu // H
    geometry(N, H, cu, want_rpb=rpb)
    check(K, S.problem(N, H, 32, 1), f"rpb={rpb}")


def test_empty_and_short_groups(K, cu):
    assert cu % 2 == 0 and cu > 2
    N, H = cu // 2 + 1, 2
    nb, rpb = geometry(N, H, cu, want_rpb=2)
    R = N * H
    starts = [b * rpb for b in range(nb)]
    assert R in starts, "no workgroup with g0 == g1"
    assert sum(g0 > R for g0 in starts) >= nb // 2 - 2, "about half the workgroups are meant to be empty"
    check(K, S.problem(N, H, 16, 1), "rpb=2")
    check(K, S.problem(N, H, 16, 0), "rpb=2")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("family", ["bigdy", "corner", "four", "bigfour"])
def test_gather_families(K, cu, family, act):
    N, H = cu // 2 + 1, 4
    geometry(N, H, cu, want_rpb=3)
    check(K, S.problem(N, H, 32, act, family), "rpb=3")


@pytest.mark.parametrize("family,act", [("xrow", 1), ("xrow", 0), ("grow", 0)])
def test_localised_rows(K, cu, family, act):
    """the one row sits in the middle of a workgroup's range of a middle workgroup; "grow" runs without the
    ReLU mask (masked, a channel can lose the whole row and the builder refuses the problem)"""
    N, H, nb, rpb = _ring_shape(cu)
    n0, y0 = divmod(rpb * (nb // 2) + rpb // 2, H)
    if family == "grow":
        y0 -= y0 % 2
    check(K, S.problem(N, H, 16, act, family, (n0, y0)), f"rpb={rpb} row=({n0},{y0})")


# ----------------------------------------------------------------------------- stem_bwd_dw
def _dw(K, tot, sums, scale, invstd, count):
    return K.stem_bwd_dw(d(tot), d(sums), d(scale), d(invstd), float(count))


def test_stem_bwd_dw_exact(K):
    """tot and sums are plain inputs of the op: lattice G1 / G2 / G3 and sums that are small multiples of the
    power-of-two count make a2, a3, both products, both differences and the scaled result fp32 numbers
    (asserted), so one rounding-free evaluation is the only correct output, with or without FMA contraction"""
    count = 1024.0
    key = ("dw-exact",)
    G1 = lattice((64, 256), -256, 256, _seed("g1", key)).double() * 16
    G2 = lattice((64, 256), -256, 256, _seed("g2", key)).double()
    G3 = lattice((256,), -256, 256, _seed("g3", key)).double()
    s1 = int_vector(64, -64, 64, _seed("s1", key)).double() * count
    s2raw = int_vector(64, -64, 64, _seed("s2", key)).double() * count
    scale = pow2_scales(64, _seed("sc", key))
    invstd = pow2_scales(64, _seed("is", key)).abs()
    t1, t2, t3, a2, a3 = S.dw_terms(G1, G2, G3, s1, s2raw, scale, invstd, count)
    sums = torch.stack([s1, s2raw * invstd.double()])
    need_fp32(a2=a2, a3=a3, s2ic=sums[1] / count, t2=t2, t3=t3, d1=t1 - t2, d2=t1 - t2 - t3, fma2=t1 - t2 - t3,
              out=scale.double()[:, None] * (t1 - t2 - t3))
    want, _ = S.dw_algebra(G1, G2, G3, s1, s2raw, scale, invstd, count)
    tot = rounded(torch.cat([G1.reshape(-1), G2.reshape(-1), G3, s1, s2raw]), F32)
    got = _dw(K, tot, rounded(sums, F32), scale, invstd, count)
    assert_exact(got, rounded(want, F32), S.DW_DIMS, "stem_bwd_dw exact")
    TALLY["stem_bwd_dw"] += 1


@pytest.mark.parametrize("W,act,count", [(32, 1, 4096.0), (48, 1, None), (56, 0, 3000.0), (112, 1, 65536.0)])
def test_stem_bwd_dw_bound(K, cu, W, act, count):
    """dW from the kernel's own tot / sums (bit-exact, checked first) inside ``S.dw_bound`` of the fp64
    algebraic form, and of the textbook sum over dz X: 8 u |scale| (|G1| + |a3 G2| + |a2 G3|) per element for a
    power-of-two count (six roundings on the longest path, see the oracle), 9 u otherwise for float(1 / count).
    ``count`` is free (the global row count under DDP); None = this problem's own N H W, not a power of two."""
    N, H = 5, 4
    pr = S.problem(N, H, W, act)
    count = float(N * H * W) if count is None else count
    pow2 = math.frexp(count)[0] == 0.5
    tot, sums = check(K, pr, "dw")
    got = _dw(K, tot, sums, pr.scale, pr.invstd, count).cpu().double()
    ref = pr.ref
    want, mag = S.dw_algebra(ref.G1, ref.G2, ref.G3, ref.s1, ref.s2raw, pr.scale, pr.invstd, count)
    text = S.dw_textbook(ref, pr.x16, pr.scale, pr.invstd, count)
    assert bool(((want - text).abs() <= 1e-12 * mag).all())
    bound = S.dw_bound(mag, pow2)
    err = (got - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max()
    print(f"\n[stem-bwd-exact] stem_bwd_dw W={W} count={count:g}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"stem_bwd_dw outside the derived bound: {(err / bound).max():.3f} x"
    assert bool(((got - text).abs() <= bound + 1e-12 * mag).all()), "stem_bwd_dw against the textbook sum over dz X"
    assert float(want.abs().max()) > 0


# ----------------------------------------------------------------------------- s2d_weight / s2d_weight_bwd
@pytest.mark.parametrize("Co", [1, 64, 65])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_s2d_weight_maps(K, C, Co):
    """pure index maps: torch.equal.  w16 starts as NaN, so every element, the zero taps included, must be
    written; Co 65 with C 3 leaves a ragged last workgroup in the backward launch"""
    g = torch.Generator().manual_seed(1000 * Co + C)
    w7 = torch.randn((Co, 7, 7, C), generator=g)
    w16 = torch.full((Co, 4, 4, 16), float("nan"), device=DEV)
    K.s2d_weight(d(w7), w16)
    assert_exact(w16, Fn.stem_s2d_weight(w7), S.DW_DIMS, f"s2d_weight Co={Co} C={C}")
    assert_exact(w16, S.s2d_weight_ref(w7), S.DW_DIMS, f"s2d_weight Co={Co} C={C} (definition)")
    g16 = torch.randn((Co, 4, 4, 16), generator=g)
    g7 = K.s2d_weight_bwd(d(g16), C)
    assert_exact(g7, S.s2d_weight_bwd_ref(g16, C), ("co", "kh", "kw", "c"), f"s2d_weight_bwd Co={Co} C={C}")
    TALLY["s2d_weight"] += 2
    TALLY["s2d_weight_bwd"] += 1


# ----------------------------------------------------------------------------- refusals
def _args(N, H, W, dy_hw=None, idx_dtype=torch.uint8):
    Ho, Wo = dy_hw or (H // 2, W // 2)
    z = torch.zeros((N, H, W, 64), dtype=BF16, device=DEV)
    x16 = torch.zeros((N, H, W, 16), dtype=BF16, device=DEV)
    dy = torch.zeros((N, Ho, Wo, 64), dtype=BF16, device=DEV)
    idx = torch.full((N, Ho, Wo, 64), 4, dtype=idx_dtype, device=DEV)
    v = torch.ones(64, device=DEV)
    return z, (dy, idx, z, x16, v, v, v, v, 1)


@pytest.mark.parametrize("case", ["W=24", "odd H", "dy size", "idx dtype"])
def test_refusals(K, case):
    if case == "W=24":
        z, args = _args(1, 4, 24)
        assert not K.stem_bwd_fusable(z)
    elif case == "odd H":
        z, args = _args(1, 3, 16, dy_hw=(1, 8))
        assert not K.stem_bwd_fusable(z)
    elif case == "dy size":
        z, args = _args(1, 4, 16, dy_hw=(2, 9))
        assert K.stem_bwd_fusable(z)
    else:
        z, args = _args(1, 4, 16, idx_dtype=torch.int32)
        assert K.stem_bwd_fusable(z)
    with pytest.raises(RuntimeError):
        K.stem_bn_pool_bwd(*args)
