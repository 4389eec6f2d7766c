"""The fused ArcFace head's coverage rule (every D <= 512, every batch size) and, on the CPU, the
sensitivity of the gradient bound that test_arcface_fused_wide_gpu.py asserts.

Sensitivity: the GPU test caps the dX / dW relative error at 1e-3.  Here the fp64 head of
tests/head_ref.py runs on the GPU test's own inputs (operands normalised and rounded to bf16 as
arc_l2norm_t_kernel does), once whole and once with one staged tile of the bf16 dcos zeroed before
the second GEMM -- what a backward kernel that skips, mis-stages or mis-addresses a tile computes.
The tile is as wide as the kernel's at that shape (32 at Dp = 512, else 64): for dX the first and the
last class tile that holds a class, for dW the second and the last row tile that holds a row.  Every
such defect moves the gradient by >= 1e-2, ten times the cap (smallest here: 9.9e-2, a 64-row tile
of dW at (6208, 70, 100); the last 32-class tile of (70, 130, 512), which holds two classes, moves
dX by 1.8e-1)."""
import pytest
import torch

from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import arcface_wide_cases as W
from tests import head_ref as R


def test_fused_dp_picks_the_padded_width():
    assert [Fn.arcface_fused_dp(D) for D in (1, 128, 129, 256, 257, 512)] == [128, 128, 256, 256, 512, 512]
    with pytest.raises(ValueError):
        Fn.arcface_fused_dp(513)


def test_fused_supported_every_batch_up_to_d512():
    for B, D in ((64, 512), (2112, 256), (8192, 256), (6208, 100), (16384, 512)):
        assert Fn.arcface_fused_supported(B, D), (B, D)
    assert not Fn.arcface_fused_supported(64, 513)


def _operands(x, Wt):
    """Normalised bf16 rows and fp32 inverse norms, as the normalisation kernel forms them."""
    out = []
    for t in (x, Wt):
        t = t.float()
        inv = 1.0 / t.norm(dim=1).clamp_min(1e-12)
        out += [(t * inv[:, None]).bfloat16(), inv]
    return out


@pytest.mark.parametrize("B,C,D", W.WIDE_SHAPES)
def test_dropped_tile_exceeds_the_gradient_cap(B, C, D):
    x, Wt, lab = W.inputs(B, C, D, torch.float32, W.seed_of(B, C, D))
    xn, inv_x, wn, inv_w = _operands(x, Wt)
    g = R.f32(W.GO) * R.f32(1.0 / B)
    xn64, wn64 = R.f64(xn), R.f64(wn)
    r = R.arcface_rows(xn64 @ wn64.t(), lab, C, W.S, W.M, True, g)
    dcos = r["dcos"].float().bfloat16().to(R.F64)
    dx = R.l2norm_grad(dcos @ wn64, xn64, inv_x, D)
    dw = R.l2norm_grad(dcos.t() @ xn64, wn64, inv_w, D)
    T = W.bwd_tile(Fn.arcface_fused_dp(D))
    for tile in (0, (C - 1) // T):  # dX: a class tile
        d = dcos.clone()
        d[:, tile * T:(tile + 1) * T] = 0
        e = R.relerr(R.l2norm_grad(d @ wn64, xn64, inv_x, D), dx)
        print(f"B{B} C{C} D{D} tile {T}: dX without class tile {tile}: relerr {e:.3e}")
        assert e >= 1e-2, (tile, e)
    for tile in (1, (B - 1) // T):  # dW: a row tile
        d = dcos.clone()
        d[tile * T:(tile + 1) * T] = 0
        e = R.relerr(R.l2norm_grad(d.t() @ xn64, wn64, inv_w, D), dw)
        print(f"B{B} C{C} D{D} tile {T}: dW without row tile {tile}: relerr {e:.3e}")
        assert e >= 1e-2, (tile, e)
