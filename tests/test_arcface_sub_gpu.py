"""The fused Sub-center ArcFace head (csrc/arcface_sub.hip): K centres per class, weight [C, K, D].

1. Lattice (tests/arcface_sub_ref.py ``lattice_inputs``): normalised entries exactly +-1/8, cosines
   exact multiples of 1/64, so cbar and the first maximum have no rounding at all and exact ties between
   sub-centres are everywhere.  Operands and sub_idx are compared with torch.equal; loss / lse within the
   K = 1 head's bound s Dp 2^-24 + 2e-5 max(1, s); rank within the near-ties of the band 2 s Dp 2^-24;
   invalid rows exactly zero.  dX / dW against the fp64 reference with dcos rounded to bf16: the bf16
   roundings of dcos flip at boundaries, so the bound is measured (MI355X, relative error, easy / hard):
     shape               dX easy / hard           dW easy / hard
     (70, 37, 2, 128)    7.42e-8 / 7.72e-8        3.77e-8 / 3.66e-8
     (64, 130, 3, 256)   1.59e-8 / 1.70e-8        9.59e-9 / 1.06e-8
     (130, 700, 4, 200)  4.876e-5 / 5.107e-5      1.559e-6 / 1.645e-6
     (200, 50, 3, 128)   3.36e-8 / 3.42e-8        4.25e-8 / 4.37e-8
   largest: dX 5.107e-5, dW 1.645e-6.  The figures repeat: fixed summation order, seeded CPU inputs.
   The assertions are 4x the largest value rounded up to one digit, never above 1e-3.  That cap is a
   property of the inputs: with the reference alone, on the CPU, two deliberate errors move dX / dW by
     shape               last maximum instead of first     dcos routed to all K planes
     (70, 37, 2, 128)    0.014 / 0.77                      1.02 / 0.80
     (64, 130, 3, 256)   0.031 / 1.15                      1.84 / 1.39
     (130, 700, 4, 200)  0.154 / 1.26                      2.44 / 1.63
     (200, 50, 3, 128)   0.116 / 1.40                      1.81 / 1.73
   (the smaller of easy / hard), each >= 1e-2.
2. Dispatch and autograd on random inputs against an fp32 CPU autograd rendering of the insightface
   formula (``view(-1, C, K).max(2)``), with the K = 1 dispatch test's tolerances (bf16 operands).
3. K = 1 is untouched: ArcMarginProduct(sub_centers=1) and a 2-D weight equal _ArcFaceFused bit for bit.
4. HIP-graph capture: replays equal eager bit for bit.
5. Memory: no [B, C K] tensor at (1024, 20000, 3, 256).
"""
import math

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.models.heads import ArcMarginProduct
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import arcface_sub_ref as SR
from tests import head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, M, GO = 30.0, 0.5, 1.0
SUB_DX_TOL = 3e-4  # 4 x the measured 5.107e-5
SUB_DW_TOL = 7e-6  # 4 x the measured 1.645e-6
assert SUB_DX_TOL <= 1e-3 and SUB_DW_TOL <= 1e-3

LATTICE = [(70, 37, 2, 128),    # two row blocks with padding; class tail inside the first tile
           (64, 130, 3, 256),   # odd K (one zero plane); several class tiles; class tail
           (130, 700, 4, 200),  # D padded to 256; three row blocks; >= 8 class splits through the XCD remap
           (200, 50, 3, 128)]   # four dW row splits (four class blocks)


@pytest.fixture(scope="module")
def lattice_cases():
    """(B, C, K, D) -> CPU inputs and the exact operands, made once."""
    out = {}
    for B, C, K, D in LATTICE:
        x, W, lab = SR.lattice_inputs(B, C, K, D, 1000 + B + C + K + D)
        (xn, ix), (wn, iw) = R.l2norm_rows(x, 1e-12), R.l2norm_rows(W.reshape(C * K, D), 1e-12)
        out[B, C, K, D] = (x, W, lab, xn, ix, wn.reshape(C, K, D), iw.reshape(C, K))
    return out


@pytest.mark.parametrize("easy", [True, False], ids=["easy", "hard"])
@pytest.mark.parametrize("B,C,K,D", LATTICE)
def test_sub_head_lattice(lattice_cases, B, C, K, D, easy):
    ops = _ext.hip_ops()
    x, W, lab, xn_e, ix_e, wn_e, iw_e = lattice_cases[B, C, K, D]
    Dp, Bp = Fn.arcface_sub_check(K, D), Fn.round_up(B, 64)
    rows, Wp = SR.operand_rows(C, K)
    labd, go = lab.to(DEV), torch.tensor([GO], device=DEV)
    xn, xnT, inv_x = ops.arcface_l2norm_t(x.to(DEV), Bp, Dp, 1e-12)
    wn, wnT, inv_w = ops.arcface_sub_l2norm_t(W.to(DEV), Dp, 1e-12)
    loss, rank, lse, labt, sub = ops.arcface_sub_fwd(xn, wn, labd, B, C, K, S, M, easy)
    dx = ops.arcface_sub_dx(xn, wn, wnT, labd, lse, labt, sub, go, 1.0 / B, inv_x, B, C, K, D, S, False)
    dw = ops.arcface_sub_dw(xn, xnT, wn, labd, lse, labt, sub, go, 1.0 / B, inv_w, B, C, K, D, S)
    torch.cuda.synchronize()
    # operands: exact values in the planar row order, exact transposes, zero padding in both dimensions
    assert wn.shape == (Wp, Dp) and wnT.shape == (Dp, Wp) and inv_w.shape == (Wp,)
    want_w, want_i = torch.zeros(Wp, Dp, dtype=R.F64), torch.zeros(Wp, dtype=R.F64)
    want_w[rows.reshape(-1), :D], want_i[rows.reshape(-1)] = wn_e.reshape(C * K, D), iw_e.reshape(-1)
    assert torch.equal(R.f64(wn), want_w) and torch.equal(R.f64(inv_w), want_i)
    assert torch.equal(wnT, wn.t().contiguous())
    assert torch.equal(R.f64(xn)[:B, :D], xn_e) and xn[B:].abs().sum().item() == 0 and xn[:, D:].abs().sum().item() == 0
    g = R.f32(GO) * R.f32(1.0 / B)
    ref = SR.sub_head(xn_e, wn_e, ix_e, iw_e, lab, D, S, M, easy, g)
    valid = ref["valid"]
    safe = lab.clamp(0, C - 1)
    assert sub.dtype == torch.int32 and sub.shape == (Bp,)
    assert torch.equal(sub[:B].cpu().long()[valid], ref["sub_idx"][torch.arange(B), safe][valid])
    tol = S * Dp * 2.0 ** -24 + 2e-5 * max(1.0, S)
    el, es = (R.f64(loss) - ref["loss"]).abs(), (R.f64(lse)[:B] - ref["lse"]).abs()
    assert (el <= tol).all() and (es <= tol).all(), (el.max(), es.max())
    assert (~valid).sum().item() == 2 and (R.f64(loss)[~valid] == 0).all() and R.f64(dx)[~valid].abs().max().item() == 0
    ties = R.near_ties(ref["x"], ref["t"], ref["onehot"], 2.0 * S * Dp * 2.0 ** -24)
    assert ((rank.cpu().long() - ref["rank"]).abs() <= ties)[valid].all(), (rank.cpu(), ref["rank"], ties)
    assert dx.shape == (B, D) and dw.shape == (C, K, D) and dw.dtype == torch.float32
    ex, ew = R.relerr(dx, ref["dx"]), R.relerr(dw, ref["dw"])
    print(f"sub head {(B, C, K, D)} easy{int(easy)}: dX relerr {ex:.3e} dW relerr {ew:.3e}")
    assert ex <= SUB_DX_TOL and ew <= SUB_DW_TOL, (ex, ew)


def test_sub_head_label_past_int32_is_invalid(lattice_cases):
    """A label whose low 32 bits name a class (2^32 + 5) is invalid to every kernel of the head, the
    shared finalize kernel included: the same outputs as for -1, a zero loss and a zero dX row."""
    ops = _ext.hip_ops()
    B, C, K, D = LATTICE[0]
    x, W, lab = lattice_cases[B, C, K, D][:3]
    Dp, Bp = Fn.arcface_sub_check(K, D), Fn.round_up(B, 64)
    go = torch.tensor([GO], device=DEV)
    xn, xnT, inv_x = ops.arcface_l2norm_t(x.to(DEV), Bp, Dp, 1e-12)
    wn, wnT, inv_w = ops.arcface_sub_l2norm_t(W.to(DEV), Dp, 1e-12)
    assert lab[1].item() == -1
    outs = []
    for bad in (-1, 2 ** 32 + 5):
        labd = lab.clone()
        labd[1] = bad
        labd = labd.to(DEV)
        loss, rank, lse, labt, sub = ops.arcface_sub_fwd(xn, wn, labd, B, C, K, S, M, True)
        dx = ops.arcface_sub_dx(xn, wn, wnT, labd, lse, labt, sub, go, 1.0 / B, inv_x, B, C, K, D, S, False)
        outs.append((loss, rank, lse, labt, sub, dx))
    assert outs[1][0][1].item() == 0 and outs[1][5][1].abs().max().item() == 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def _relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _insightface_fp32(x, W, lab, s, m, easy):
    """fp32 autograd on the CPU: cos [B, C K] -> view(-1, C, K).max(2) -> margin -> mean cross-entropy."""
    C, K, D = W.shape
    xt, Wr = x.float().clone().requires_grad_(True), W.clone().requires_grad_(True)
    cos = torch.nn.functional.linear(torch.nn.functional.normalize(xt), torch.nn.functional.normalize(Wr.view(C * K, D)))
    cos = cos.view(-1, C, K).max(2)[0]
    phi = cos * math.cos(m) - torch.sqrt((1.0 - cos.pow(2)).clamp(0, 1)) * math.sin(m)
    phi = torch.where(cos > 0, phi, cos) if easy else torch.where(cos > math.cos(math.pi - m), phi,
                                                                  cos - math.sin(math.pi - m) * m)
    oh = torch.zeros_like(cos).scatter_(1, lab.view(-1, 1), 1)
    loss = torch.nn.functional.cross_entropy((oh * phi + (1 - oh) * cos) * s, lab)
    loss.backward()
    return loss.detach(), xt.grad, Wr.grad


@pytest.mark.parametrize("B,C,K,D,dtype,easy", [(48, 300, 3, 256, torch.bfloat16, False),
                                                (130, 90, 2, 100, torch.float32, True)])
def test_sub_head_dispatch_and_autograd(B, C, K, D, dtype, easy):
    torch.manual_seed(B + C + K + D)
    x, W, lab = torch.randn(B, D).to(dtype), torch.randn(C, K, D) * 0.05, torch.randint(0, C, (B,))
    lr, dxr, dwr = _insightface_fp32(x, W, lab, S, M, easy)
    xd, Wd = x.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
    loss, rank, _, sub = Fn.arcface_loss(xd, Wd, lab.to(DEV), S, M, easy, return_sub_idx=True)
    assert "_ArcFaceSubFused" in type(loss.grad_fn).__name__
    loss.backward()
    assert abs(loss.item() - lr.item()) / abs(lr.item()) < 1e-2, (loss.item(), lr.item())
    assert xd.grad.shape == (B, D) and xd.grad.dtype == dtype and Wd.grad.shape == (C, K, D)
    assert rank.shape == (B,) and sub.shape == (B,) and 0 <= sub.min().item() and sub.max().item() < K
    assert _relerr(xd.grad, dxr) < 3e-2 and _relerr(Wd.grad, dwr) < 3e-2, (_relerr(xd.grad, dxr), _relerr(Wd.grad, dwr))
    # evaluation runs the fused forward alone: the same rows with the margin, plain cosines with m = 0
    le, re = Fn.arcface_rows(xd.detach(), Wd.detach(), lab.to(DEV), S, M, easy)
    assert torch.equal(re, rank) and torch.equal(le.mean(), loss.detach())
    lp, _ = Fn.arcface_rows(xd.detach(), Wd.detach(), lab.to(DEV), S, M, easy, with_margin=False)
    lp_ref = _insightface_fp32(x, W, lab, S, 0.0, True)[0]
    assert abs(lp.mean().item() - lp_ref.item()) / lp_ref.item() < 1e-2


def test_sub_centers_1_is_todays_head():
    torch.manual_seed(5)
    B, C, D = 70, 130, 256
    x, lab = torch.randn(B, D, device=DEV), torch.randint(0, C, (B,), device=DEV)
    head = ArcMarginProduct(D, C, S, M, True, sub_centers=1).to(DEV)
    assert head.weight.shape == (C, D)
    outs = []
    for fn in (lambda a, w: head(a, lab)[:2], lambda a, w: Fn.arcface_loss(a, w, lab, S, M, True)[:2],
               lambda a, w: Fn._ArcFaceFused.apply(a, w, lab, S, M, True)):
        xd, Wd = x.clone().requires_grad_(True), head.weight
        Wd.grad = None
        loss, rank = fn(xd, Wd)
        loss.backward()
        outs.append((loss.detach(), rank, xd.grad, Wd.grad.clone()))
    for o in outs[:2]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[2]))


def test_sub_head_graph_capture():
    torch.manual_seed(2)
    B, C, K, D = 70, 130, 3, 256
    x, W = torch.randn(B, D, device=DEV), (torch.randn(C, K, D) * 0.05).to(DEV)
    lab = torch.randint(0, C, (B,), device=DEV)
    xd, Wd = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    loss, _, _ = Fn.arcface_loss(xd, Wd, lab, S, M, True)
    loss.backward()
    xs, Ws = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs.grad = Ws.grad = None
            Fn.arcface_loss(xs, Ws, lab, S, M, True)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    xs.grad = Ws.grad = None
    with torch.cuda.graph(graph):
        l3, _, _ = Fn.arcface_loss(xs, Ws, lab, S, M, True)
        l3.backward()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(l3, loss.detach()) and torch.equal(xs.grad, xd.grad) and torch.equal(Ws.grad, Wd.grad)


def test_sub_head_memory():
    """No [B, C K] tensor: the 100k-class bound of the K = 1 head with C K rows."""
    torch.manual_seed(3)
    B, C, K, D = 1024, 20000, 3, 256
    x, W = torch.randn(B, D, device=DEV), (torch.randn(C, K, D) * 0.05).to(DEV)
    lab = torch.randint(0, C, (B,), device=DEV)
    xd, Wd = x.requires_grad_(True), W.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, _, _ = Fn.arcface_loss(xd, Wd, lab, S, M, True)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.isfinite(loss) and torch.isfinite(Wd.grad).all() and torch.isfinite(xd.grad).all()
    assert peak < 3 * (C * K * D * 4) + (B * C * K * 2) // 4, peak
