"""The fused ArcFace head (csrc/arcface.hip) at the widths and batch sizes it did not cover before:
Dp = 512 (D up to 512) and padded batches past the old LDS limit of the dW kernel (2048 rows at
Dp = 256, 6144 at Dp = 128).

1. Matched operands: arcface_l2norm_t -> arcface_fused_fwd / _dx / _dw against the fp64 head of
   tests/head_ref.py on the operands the normalisation kernel returned.  Shapes (B, C, D):
     (70, 130, 512)    Dp = 512: 64-class forward tiles, 32-class / 32-row backward tiles
     (64, 700, 300)    D padded to 512: the columns 300.. of xn, wn and the rows 300.. of their
                       transposes are exactly zero; dX / dW are [., 300]
     (130, 1100, 512)  three row blocks, 16 class splits through the XCD remap
     (2112, 130, 256)  33 row tiles: the first padded batch past the old limit, dW row splits 9/9/9/6
     (2112, 130, 512)  66 32-row tiles at Dp = 512 over 4 splits (17/17/17/15)
     (6208, 70, 100)   Dp = 128 past its old limit: 97 row tiles over 4 dW splits (25/25/25/22)
   Bounds: operands one bf16 rounding + 1e-7, nT == n.t() exactly, zero padding; loss and lse rows
   |err| <= s Dp 2^-24 + 2e-5 max(1, s) (the fp32 dot of Dp products of unit-vector entries, as the
   rank band; then the project's loss tolerance); invalid-label rows exactly zero; rank within the
   near-ties of the band 2 s Dp 2^-24.
   dX, dW: bf16 roundings of dcos flip where the fp32 and the fp64 value straddle a rounding
   boundary, so there is no derivable bound.  Measured on an MI355X against the fp64 reference on the
   kernel's own operands (relative error; fp32-feature cases easy / hard margin, then the dW of the
   bf16-feature cases, whose dX is held to its output rounding element by element):
     shape              fp32 features: dX / dW easy, dX / dW hard     bf16 features: dW easy, dW hard
     (70, 130, 512)     7.7e-8 / 7.4e-8, 7.8e-8 / 7.6e-8              7.4e-8, 7.5e-8
     (64, 700, 300)     6.3e-6 / 5.6e-6, 1.7e-6 / 1.5e-6              1.27e-5, 1.39e-5
     (130, 1100, 512)   1.1e-6 / 1.0e-6, 1.5e-6 / 1.5e-6              2.6e-6, 2.9e-6
     (2112, 130, 256)   1.71e-5 / 1.67e-5, 9.0e-6 / 9.0e-6            2.4e-6, 2.0e-6
     (2112, 130, 512)   3.7e-6 / 3.6e-6, 1.7e-6 / 1.7e-6              6.1e-6, 9.2e-7
     (6208, 70, 100)    8.0e-7 / 8.6e-7, 1.9e-6 / 1.9e-6              1.77e-5, 1.41e-5
   largest: dX with an fp32 output 1.713e-5, dW 1.770e-5 (a bf16 dX is 1.64e-3 .. 1.69e-3: its output
   rounding).  The figures repeat: fixed summation order, seeded CPU inputs.
   The assertions are 4x the largest value, rounded up to one digit (WIDE_DX_TOL, WIDE_DW_TOL), and
   never above 1e-3: test_arcface_fused_wide_cpu.py shows that a dropped staged tile costs >= 1e-2
   at exactly these shapes and inputs.
2. Dispatch and autograd: Fn.arcface_loss runs _ArcFaceFused at (48, 700, 512) and (2112, 300, 256)
   and agrees with an fp32 autograd rendering of the reference head and with the unfused kernel path.
3. Copies: a 4224-row batch made of two copies of a 2112-row batch gives bit-identical halves (row
   block indexing across 66 blocks, no tolerance).
4. HIP-graph capture at D = 512: replay equals eager bit for bit.
5. Memory: no [B, C] tensor at (1024, 100000, 512) and at (8192, 10000, 256).
"""
import math
import os

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import arcface_wide_cases as W
from tests import head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, M, GO = W.S, W.M, W.GO
GRAD_CAP = 1e-3      # no measurement may raise a gradient bound above this (see the module docstring)
WIDE_DX_TOL = 7e-5   # 4 x the measured 1.713e-5
WIDE_DW_TOL = 8e-5   # 4 x the measured 1.770e-5
assert WIDE_DX_TOL <= GRAD_CAP and WIDE_DW_TOL <= GRAD_CAP


@pytest.fixture(scope="module")
def K():
    return _ext.hip_ops()


def _run_ops(K, x, Wt, lab, B, C, D, easy):
    """The bound ops on CPU inputs -> every output plus the operands, still on the GPU."""
    Dp = Fn.arcface_fused_dp(D)
    Bp, Cp = Fn.round_up(B, 64), Fn.round_up(C, 64)
    xd, Wd, labd = x.to(DEV), Wt.to(DEV), lab.to(DEV)
    xn, xnT, inv_x = K.arcface_l2norm_t(xd, Bp, Dp, 1e-12)
    wn, wnT, inv_w = K.arcface_l2norm_t(Wd, Cp, Dp, 1e-12)
    go = torch.tensor([GO], device=DEV)
    loss, rank, lse, labt = K.arcface_fused_fwd(xn, wn, labd, B, C, S, M, easy)
    dx = K.arcface_fused_dx(xn, wn, wnT, labd, lse, labt, go, 1.0 / B, inv_x, B, C, D, S, x.dtype == torch.bfloat16)
    dw = K.arcface_fused_dw(xn, xnT, wn, labd, lse, labt, go, 1.0 / B, inv_w, B, C, D, S)
    torch.cuda.synchronize()
    return dict(xn=xn, xnT=xnT, inv_x=inv_x, wn=wn, wnT=wnT, inv_w=inv_w, loss=loss, rank=rank, lse=lse, dx=dx,
                dw=dw, Dp=Dp, Bp=Bp, Cp=Cp)


@pytest.mark.parametrize("easy", [True, False], ids=["easy", "hard"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C,D", W.WIDE_SHAPES)
def test_wide_head_matched_operands(K, B, C, D, dtype, easy):
    x, Wt, lab = W.inputs(B, C, D, dtype, W.seed_of(B, C, D))
    o = _run_ops(K, x, Wt, lab, B, C, D, easy)
    Dp, Bp, Cp = o["Dp"], o["Bp"], o["Cp"]
    # the operands: normalised rows, exact transposes, zero padding in both dimensions, inverse norm 0
    for src, n, nT, inv, rows, Rp in ((x, o["xn"], o["xnT"], o["inv_x"], B, Bp), (Wt, o["wn"], o["wnT"], o["inv_w"], C, Cp)):
        assert n.shape == (Rp, Dp) and nT.shape == (Dp, Rp) and inv.shape == (Rp,)
        yr, ir = R.l2norm_rows(src, 1e-12)
        assert R.bf16_excess(n[:rows, :D], yr, 1e-7) <= 0
        assert ((R.f64(inv)[:rows] - ir).abs() / ir).max().item() <= 1e-6
        assert torch.equal(nT, n.t().contiguous())
        if Rp > rows:
            assert n[rows:].abs().max().item() == 0 and inv[rows:].abs().max().item() == 0
        if Dp > D:
            assert n[:, D:].abs().max().item() == 0 and nT[D:].abs().max().item() == 0
    g = R.f32(GO) * R.f32(1.0 / B)
    ref = R.arcface_head(o["xn"], o["wn"], o["inv_x"], o["inv_w"], lab, B, C, D, S, M, easy, g)
    valid = ref["valid"]
    assert o["loss"].shape == (B,) and o["lse"].shape == (Bp,) and o["rank"].shape == (B,)
    assert o["dx"].shape == (B, D) and o["dw"].shape == (C, D)
    assert o["dx"].dtype == dtype and o["dw"].dtype == torch.float32
    tol = S * Dp * 2.0 ** -24 + 2e-5 * max(1.0, S)
    el = (R.f64(o["loss"]) - ref["loss"]).abs()
    es = (R.f64(o["lse"])[:B] - ref["lse"]).abs()
    print(f"wide head B{B} C{C} D{D}: loss / lse err over tol {(el / tol).max().item():.3f} {(es / tol).max().item():.3f}")
    assert (el <= tol).all() and (es <= tol).all(), (el.max(), es.max())
    assert (R.f64(o["loss"])[~valid] == 0).all()
    band = 2.0 * S * Dp * 2.0 ** -24
    ties = R.near_ties(ref["x"], ref["t"], ref["onehot"], band)
    assert ((o["rank"].cpu().long() - ref["rank"]).abs() <= ties)[valid].all(), (o["rank"].cpu(), ref["rank"], ties)
    assert (~valid).sum().item() == 2 and R.f64(o["dx"])[~valid].abs().max().item() == 0
    assert torch.isfinite(o["dx"]).all() and torch.isfinite(o["dw"]).all()
    ex, ew = R.relerr(o["dx"], ref["dx"]), R.relerr(o["dw"], ref["dw"])
    print(f"wide head B{B} C{C} D{D} {dtype} easy{int(easy)}: dX relerr {ex:.3e} dW relerr {ew:.3e}")
    if dtype == torch.bfloat16:
        # the bf16 store of dX, element by element: one rounding of the reference, plus the fp32 path's
        # error vector, whose norm is <= WIDE_DX_TOL |dX|
        elem = R.bf16_excess(o["dx"], ref["dx"], WIDE_DX_TOL * ref["dx"].norm().item())
        print("wide bf16 dX element rule excess", elem)
        assert elem <= 0, elem
    else:
        assert ex <= WIDE_DX_TOL, ex
    assert ew <= WIDE_DW_TOL, ew


# ----------------------------------------------------------------------------- dispatch and autograd
def _relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ref_head_fp32(x, Wt, lab, s, m, easy):
    """fp32 autograd ArcMarginProduct + mean cross-entropy on the CPU -> (loss, dx, dW)."""
    xt, Wr = x.float().clone().requires_grad_(True), Wt.float().clone().requires_grad_(True)
    cos = torch.nn.functional.linear(torch.nn.functional.normalize(xt), torch.nn.functional.normalize(Wr))
    sine = torch.sqrt((1.0 - cos.pow(2)).clamp(0, 1))
    phi = cos * math.cos(m) - sine * math.sin(m)
    if easy:
        phi = torch.where(cos > 0, phi, cos)
    else:
        phi = torch.where(cos > math.cos(math.pi - m), phi, cos - math.sin(math.pi - m) * m)
    oh = torch.zeros_like(cos).scatter_(1, lab.view(-1, 1), 1)
    loss = torch.nn.functional.cross_entropy((oh * phi + (1 - oh) * cos) * s, lab)
    loss.backward()
    return loss.detach(), xt.grad, Wr.grad


def _run_loss(x, Wt, lab, s, m, easy, fused):
    old = os.environ.get("DCP_ARCFACE_FUSED")
    os.environ["DCP_ARCFACE_FUSED"] = "1" if fused else "0"
    try:
        xd, Wd = x.to(DEV).requires_grad_(True), Wt.to(DEV).requires_grad_(True)
        loss, rank, _ = Fn.arcface_loss(xd, Wd, lab.to(DEV), s, m, easy)
        name = type(loss.grad_fn).__name__
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), xd.grad, Wd.grad, name
    finally:
        if old is None:
            os.environ.pop("DCP_ARCFACE_FUSED", None)
        else:
            os.environ["DCP_ARCFACE_FUSED"] = old


@pytest.mark.parametrize("B,C,D,easy", [(48, 700, 512, False), (2112, 300, 256, True)])
def test_wide_head_dispatch_and_autograd(B, C, D, easy):
    torch.manual_seed(B + C + D)
    x = torch.randn(B, D)
    Wt = torch.randn(C, D) * 0.05
    lab = torch.randint(0, C, (B,))
    x[:3] = Wt[lab[:3]]  # cos ~ 1: the reference's sqrt has an infinite derivative there (NaN rows)
    lr, dxr, dwr = _ref_head_fp32(x, Wt, lab, S, M, easy)
    lf, dxf, dwf, name = _run_loss(x, Wt, lab, S, M, easy, fused=True)
    assert "_ArcFaceFused" in name, name
    assert abs(lf.item() - lr.item()) / max(abs(lr.item()), 1e-6) < 1e-2, (lf.item(), lr.item())
    assert torch.isfinite(dxf).all() and torch.isfinite(dwf).all()
    assert dxf.shape == (B, D) and dwf.shape == (C, D)
    rx, rw = torch.isfinite(dxr).all(1), torch.isfinite(dwr).all(1)
    assert rx.sum() >= B - 3 and rw.sum() >= C - 3
    assert _relerr(dxf[rx.to(DEV)], dxr[rx]) < 3e-2, _relerr(dxf[rx.to(DEV)], dxr[rx])
    assert _relerr(dwf[rw.to(DEV)], dwr[rw]) < 3e-2, _relerr(dwf[rw.to(DEV)], dwr[rw])
    lu, dxu, dwu, uname = _run_loss(x, Wt, lab, S, M, easy, fused=False)
    assert "_ArcFaceFused" not in uname, uname
    assert abs(lf.item() - lu.item()) / abs(lu.item()) < 5e-3, (lf.item(), lu.item())
    assert _relerr(dxf, dxu) < 3e-2 and _relerr(dwf, dwu) < 3e-2, (_relerr(dxf, dxu), _relerr(dwf, dwu))


# ----------------------------------------------------------------------------- copies
@pytest.mark.parametrize("D", [256, 512])
def test_wide_head_two_copies_are_bit_identical(K, D):
    B1, C = 2112, 130
    x, Wt, lab = W.inputs(B1, C, D, torch.float32, 77 + D)
    o = _run_ops(K, torch.cat([x, x]), Wt, torch.cat([lab, lab]), 2 * B1, C, D, True)
    assert o["Bp"] == 4224
    for name in ("loss", "rank", "dx"):
        t = o[name]
        assert t.shape[0] == 2 * B1 and torch.equal(t[:B1], t[B1:]), name
    assert torch.isfinite(o["dx"]).all() and o["dx"].abs().max().item() > 0


# ----------------------------------------------------------------------------- graph capture
def test_wide_head_invalid_labels_and_graph_capture():
    torch.manual_seed(2)
    B, C, D = 70, 500, 512
    x = torch.randn(B, D, device=DEV)
    Wt = (torch.randn(C, D) * 0.05).to(DEV)
    lab = torch.randint(0, C, (B,), device=DEV)
    lab[5] = -1
    lab[6] = C + 3
    xd, Wd = x.clone().requires_grad_(True), Wt.clone().requires_grad_(True)
    loss, rank, _ = Fn.arcface_loss(xd, Wd, lab, S, M, True)
    assert "_ArcFaceFused" in type(loss.grad_fn).__name__
    loss.backward()
    assert torch.isfinite(loss) and xd.grad[5].abs().max().item() == 0.0 and xd.grad[6].abs().max().item() == 0.0
    g_ref = (loss.detach().clone(), xd.grad.clone(), Wd.grad.clone())
    xs, Ws = x.clone().requires_grad_(True), Wt.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs.grad = Ws.grad = None
            l2, _, _ = Fn.arcface_loss(xs, Ws, lab, S, M, True)
            l2.backward()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    xs.grad = Ws.grad = None
    with torch.cuda.graph(graph):
        l3, _, _ = Fn.arcface_loss(xs, Ws, lab, S, M, True)
        l3.backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(l3, g_ref[0]) and torch.equal(xs.grad, g_ref[1]) and torch.equal(Ws.grad, g_ref[2])


# ----------------------------------------------------------------------------- memory
def _step_peak(x, Wt, lab, fused):
    old = os.environ.get("DCP_ARCFACE_FUSED")
    os.environ["DCP_ARCFACE_FUSED"] = "1" if fused else "0"
    try:
        xd, Wd = x.clone().requires_grad_(True), Wt.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, _, _ = Fn.arcface_loss(xd, Wd, lab, S, M, True)
        name = type(loss.grad_fn).__name__
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert torch.isfinite(loss) and torch.isfinite(Wd.grad).all() and torch.isfinite(xd.grad).all()
        return peak, name
    finally:
        if old is None:
            os.environ.pop("DCP_ARCFACE_FUSED", None)
        else:
            os.environ["DCP_ARCFACE_FUSED"] = old


def _mem_inputs(B, C, D, seed):
    torch.manual_seed(seed)
    return (torch.randn(B, D, device=DEV), (torch.randn(C, D) * 0.05).to(DEV), torch.randint(0, C, (B,), device=DEV))


def test_wide_head_100k_classes_d512_memory():
    """100k classes, batch 1024, D = 512: the fused step's extra memory is O((B + C) D) -- the
    bounds of the 100k-class test at D = 256."""
    B, C, D = 1024, 100000, 512
    x, Wt, lab = _mem_inputs(B, C, D, 3)
    pf, name = _step_peak(x, Wt, lab, True)
    assert "_ArcFaceFused" in name, name
    pu, _ = _step_peak(x, Wt, lab, False)
    bc = B * C * 2  # one bf16 [B, C] tensor
    cd = C * D * 4  # one fp32 [C, D] tensor
    print(f"D 512 100k classes: fused peak {pf / 2**20:.1f} MB, unfused {pu / 2**20:.1f} MB")
    assert pf < 3 * cd + bc // 4, (pf, pu, bc, cd)
    assert pu - pf > bc, (pf, pu, bc)


def test_wide_head_batch_8192_memory():
    """Batch 8192, 10000 classes, D = 256 (the ArcFace benchmark's head): the fused step's extra memory
    stays below ONE bf16 [B, C] tensor (164 MB); the unfused path holds two."""
    B, C, D = 8192, 10000, 256
    x, Wt, lab = _mem_inputs(B, C, D, 4)
    pf, name = _step_peak(x, Wt, lab, True)
    assert "_ArcFaceFused" in name, name
    print(f"batch 8192: fused peak {pf / 2**20:.1f} MB")
    assert pf < B * C * 2, (pf, B * C * 2)
