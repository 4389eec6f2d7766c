"""The fused supervised contrastive loss (csrc/supcon.hip) on the GPU.

1. The ops on the kernel's own operands (``arcface_l2norm_t``) against the fp64 reference (tests/supcon_ref.py),
   at the heuristic splits and at a forced 2.  lse and loss_i per row within (1 / tau) Dp 2^-24 +
   2e-5 max(1, 1 / tau) (the K = 1 ArcFace head's bound with s = 1 / tau); 1 / |P|, the anchor count, the zero
   losses of invalid rows and non-anchors and the zero dx rows of invalid rows exactly (a valid non-anchor is
   still a negative of the other rows: its dx row is the transpose term alone).  dx against the reference with
   G rounded to bf16: the roundings flip at boundaries, so the bound is measured (MI355X, relative error,
   splits heuristic / 2):
     (4, 24, 2, 0.1)        3.657e-8 / 3.657e-8        (65, 512, 64, 0.07)    6.611e-8 / 6.611e-8
     (70, 37, 9, 0.1)       7.795e-8 / 7.795e-8        (130, 200, 40, 0.1)    7.231e-8 / 8.452e-8
     (64, 128, 5, 0.07)     6.291e-8 / 6.291e-8        (530, 128, 20, 0.1)    3.128e-6 / 2.275e-6
   largest: 3.128e-6; the figures repeat (fixed summation order, seeded CPU inputs).  The assertion is 4x that,
   rounded up to one digit, never above 1e-3: the cap separates the kernel from the four deliberate errors
   of test_supcon_cpu.py, each >= 1e-2 on these inputs.
2. Degenerate batches.  3. Autograd through ``Fn.supcon_loss`` against fp32 CPU autograd from the raw rows (the
   K = 1 dispatch test's tolerances: bf16 operands).  4. HIP-graph replays on three batches equal eager.
"""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import head_ref as R
from tests import supcon_ref as SR
from tests.supcon_ref import CASES, case_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GO = 1.0
DX_TOL = 2e-5  # 4 x the measured 3.128e-6
assert DX_TOL <= 1e-3


def run_ops(x, y, tau, splits):  # the two ops on the kernel's own operands
    ops = _ext.hip_ops()
    B, D = x.shape
    zn, znT, inv = ops.arcface_l2norm_t(x.to(DEV), Fn.round_up(B, 64), Fn.arcface_fused_dp(D), 1e-12)
    rec, stat, nanch = ops.supcon_fwd(zn, y.to(DEV), B, tau, splits)
    dx = ops.supcon_dz(zn, znT, inv, rec, stat, torch.tensor([GO], device=DEV), B, D, tau, splits, False)
    torch.cuda.synchronize()
    return zn, inv, rec.cpu(), stat.cpu(), nanch.item(), dx


def check(x, y, tau, splits, tag):
    B, D = x.shape
    zn, inv, rec, stat, nanch, dx = run_ops(x, y, tau, splits)
    ref = SR.supcon(zn, inv, y, D, tau, g=GO)
    valid, anchor = ref["valid"], ref["anchor"]
    tol = (1.0 / tau) * zn.shape[1] * 2.0 ** -24 + 2e-5 * max(1.0, 1.0 / tau)
    el = (R.f64(rec[:B, 0]) - ref["lse"]).abs()[valid]
    er = (R.f64(rec[:B, 3]) - ref["rows"]).abs()
    assert (el <= tol).all() and (er <= tol).all() and abs(stat[0].item() - ref["loss"].item()) <= tol, (el.max(), er.max())
    want_invp = torch.where(anchor, 1.0 / ref["cnt"].clamp(min=1).float(), torch.zeros(B))
    assert torch.equal(rec[:B, 1], want_invp) and nanch == ref["n"] and stat[1].item() == R.f32(1.0 / max(1, ref["n"]))
    assert (rec[:B, 3][~anchor] == 0).all() and (rec[B:, 1] == 0).all()
    assert torch.isfinite(dx).all() and dx.shape == (B, D) and dx[~valid.to(DEV)].abs().sum().item() == 0
    e = R.relerr(dx, ref["dx"])
    print(f"supcon {tag} splits {splits}: dx relerr {e:.3e}")
    assert e <= DX_TOL, e
    return ref, dx


@pytest.mark.parametrize("splits", [0, 2], ids=["auto", "split2"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_supcon_kernels_against_fp64(case, splits):
    x, y = case_inputs(case)
    check(x, y, CASES[case][3], splits, CASES[case])


def test_supcon_degenerate_batches():
    torch.manual_seed(7)
    x = torch.randn(70, 37)
    ref, dx = check(x, torch.arange(70), 0.1, 0, "all distinct")
    assert ref["loss"].item() == 0 and torch.equal(dx, torch.zeros_like(dx))
    ref, _ = check(x, torch.zeros(70, dtype=torch.int64), 0.1, 0, "all equal")
    assert ref["n"] == 70
    # B = 2, equal labels: lse_i = s_01, loss exactly 0.  The backward's exp(s - lse) takes s as an unrounded FMA: G is
    # within gs (e^u - 1) of 0, u = an fp32 ulp of s <= (1 / tau) 2^-23, so |dx| <= inv gs (1 / tau) 2^-23, gs = g / (n tau)
    _, inv, rec, stat, nanch, dx = run_ops(x[:2], torch.tensor([3, 3]), 0.1, 0)
    assert nanch == 2 and stat[0].item() == 0 and (rec[:2, 3] == 0).all()
    assert dx.abs().max().item() <= inv.max().item() * (GO / 2 / 0.1) * (1 / 0.1) * 2.0 ** -23


@pytest.mark.parametrize("B,D,dtype,ntxent", [(70, 37, torch.float32, False), (130, 200, torch.bfloat16, False),
                                               (70, 37, torch.bfloat16, True)])
def test_supcon_autograd(B, D, dtype, ntxent):
    torch.manual_seed(B + D)
    x = torch.randn(B, D).to(dtype)
    y = torch.arange(B // 2).repeat(2) if ntxent else torch.randint(0, 9, (B,))
    xc = x.float().clone().requires_grad_(True)
    lr = Fn.supcon_loss(xc, y, 0.1)  # the CPU path: fp32 torch autograd of the definition
    lr.backward()
    grads = []
    for scale in (1.0, 2.5):
        xd = x.to(DEV).requires_grad_(True)
        loss = Fn.supcon_loss(xd, y.to(DEV), 0.1)
        assert "_SupCon" in type(loss.grad_fn).__name__ and loss.dtype == torch.float32 and loss.dim() == 0
        (scale * loss).backward()
        grads.append(xd.grad)
    assert abs(loss.item() - lr.item()) / abs(lr.item()) < 1e-2 and grads[0].shape == (B, D) and grads[0].dtype == dtype
    assert R.relerr(grads[0], xc.grad) < 3e-2, R.relerr(grads[0], xc.grad)
    # (G is rounded to bf16 after the upstream factor: the two gradients differ by those roundings, 2^-9 each)
    assert R.relerr(grads[1], 2.5 * grads[0].float()) < 2.0 ** -7


def test_supcon_graph_capture():
    torch.manual_seed(2)
    B, D = 70, 200
    batches = [(torch.randn(B, D, device=DEV), torch.randint(0, 9, (B,), device=DEV)),
               (torch.randn(B, D, device=DEV), torch.arange(B, device=DEV)),  # no positives
               (torch.randn(B, D, device=DEV), torch.randint(-1, 3, (B,), device=DEV))]
    eager = []
    for x, y in batches:
        xd = x.clone().requires_grad_(True)
        loss = Fn.supcon_loss(xd, y, 0.1)
        eager.append((loss.detach().clone(), torch.autograd.grad(loss, xd)[0]))
    xs, ys = batches[0][0].clone().requires_grad_(True), batches[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs.grad = None
            Fn.supcon_loss(xs, ys, 0.1).backward()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    xs.grad = None
    with torch.cuda.graph(graph):
        l3 = Fn.supcon_loss(xs, ys, 0.1)
        l3.backward()
    for (x, y), (le, ge) in zip(batches, eager):
        with torch.no_grad():
            xs.copy_(x)
            ys.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(l3, le) and torch.equal(xs.grad, ge)
    assert eager[1][0].item() == 0 and eager[1][1].abs().max().item() == 0
