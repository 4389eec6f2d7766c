"""The fp64 references of tests/head_ref.py checked on the CPU alone, against torch autograd and
torch.optim in fp64: the GPU head / optimizer / CDR tests stand on these formulas."""
import math

import pytest
import torch

from tests import head_ref as R

F64 = torch.float64


def _close(a, b, tol=1e-12):
    a, b = a.to(F64), b.to(F64)
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_xent_reference_matches_autograd(smoothing):
    torch.manual_seed(0)
    B, C, ld = 9, 33, 40
    x = (torch.randn(B, ld) * 3).bfloat16()
    lab = torch.randint(0, C, (B,))
    xt = x[:, :C].to(F64).requires_grad_(True)
    rows = torch.nn.functional.cross_entropy(xt, lab, reduction="none", label_smoothing=R.f32(smoothing))
    (0.37 * rows.sum()).backward()
    r = R.xent_rows(x, lab, C, smoothing)
    assert _close(r["loss"], rows.detach())
    assert _close(R.xent_grad(x, lab, C, 0.37, smoothing), xt.grad)
    xl = xt.detach().gather(1, lab[:, None])
    assert torch.equal(r["rank"], (xt.detach() > xl).sum(1))
    # invalid labels: loss 0, gradient row 0 (the project divides by B, so nothing else changes)
    lab2 = lab.clone()
    lab2[1], lab2[2] = -1, C
    r2 = R.xent_rows(x, lab2, C, smoothing)
    d2 = R.xent_grad(x, lab2, C, 0.37, smoothing)
    assert r2["loss"][1] == 0 and r2["loss"][2] == 0 and d2[1:3].abs().max() == 0
    keep = torch.tensor([0] + list(range(3, B)))
    assert torch.equal(r2["loss"][keep], r["loss"][keep]) and _close(d2[keep], xt.grad[keep])


def test_log_softmax_reference_matches_autograd():
    torch.manual_seed(1)
    x = torch.randn(7, 45)
    xt = x[:, :40].to(F64).requires_grad_(True)
    y = torch.log_softmax(xt, 1)
    dy = torch.randn(7, 40, dtype=F64) + 0.3
    y.backward(dy)
    assert _close(R.log_softmax_rows(x, 40), y.detach())
    assert _close(R.log_softmax_grad(y.detach(), dy), xt.grad)


def test_l2norm_reference_matches_autograd():
    torch.manual_seed(2)
    x = torch.randn(6, 20)
    x[3] = 0
    xt = x.to(F64).requires_grad_(True)
    y = xt / xt.norm(dim=1, keepdim=True).clamp_min(R.f32(1e-12))
    dy = torch.randn(6, 24, dtype=F64)
    y.backward(dy[:, :20])
    yr, inv = R.l2norm_rows(x, 1e-12)
    assert _close(yr, y.detach()) and yr[3].abs().max() == 0 and torch.isfinite(inv).all()
    nz = torch.tensor([0, 1, 2, 4, 5])  # (the zero row: the clamp's subgradient, not the formula)
    assert _close(R.l2norm_grad(dy, yr, inv, 20)[nz], xt.grad[nz])


def test_prefix_mask_reference():
    x = torch.arange(15.0).reshape(3, 5).bfloat16()
    assert torch.equal(R.prefix_mask(x, 2)[:, :2], x[:, :2]) and R.prefix_mask(x, 2)[:, 2:].abs().max() == 0
    assert torch.equal(R.prefix_mask(x, 12), x)


def _arc_autograd(xt, wt, lab, s, m, easy, g):
    cm, sm, th, mm = R.arc_consts(m)
    cos = torch.nn.functional.normalize(xt) @ torch.nn.functional.normalize(wt).t()
    sine = torch.sqrt((1.0 - cos.pow(2)).clamp(0, 1))
    phi = cos * cm - sine * sm
    phi = torch.where(cos > 0, phi, cos) if easy else torch.where(cos > th, phi, cos - mm)
    oh = torch.zeros_like(cos).scatter_(1, lab.view(-1, 1), 1)
    out = (oh * phi + (1 - oh) * cos) * R.f32(s)
    rows = torch.nn.functional.cross_entropy(out, lab, reduction="none")
    (g * rows.sum()).backward()
    return out.detach(), rows.detach()


@pytest.mark.parametrize("easy", [True, False])
def test_arcface_references_match_autograd(easy):
    """ArcMarginProduct + CE by autograd in fp64 against arcface_rows (from the cosines) and
    arcface_head (from normalised operands: exact here, because they are passed unrounded and dcos
    values are exactly representable only up to bf16 -- so dx / dw agree to the bf16 step)."""
    torch.manual_seed(3)
    B, C, D, s, m, g = 10, 37, 24, 30.0, 0.5, 0.37 / 10
    x, w = torch.randn(B, D, dtype=F64), torch.randn(C, D, dtype=F64)
    lab = torch.randint(0, C, (B,))
    xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out, rows = _arc_autograd(xt, wt, lab, s, m, easy, g)
    xn, inv_x = R.l2norm_rows(x, 1e-12)
    wn, inv_w = R.l2norm_rows(w, 1e-12)
    r = R.arcface_rows(xn @ wn.t(), lab, C, s, m, easy, g)
    assert _close(r["x"], out) and _close(r["loss"], rows)
    assert torch.equal(r["rank"], (out > out.gather(1, lab[:, None])).sum(1))
    # dcos through both GEMMs and normalisation backwards = autograd's dx, dw
    dx = R.l2norm_grad(r["dcos"] @ wn, xn, inv_x, D)
    dw = R.l2norm_grad(r["dcos"].t() @ xn, wn, inv_w, D)
    assert _close(dx, xt.grad, 1e-10) and _close(dw, wt.grad, 1e-10)
    h = R.arcface_head(xn, wn, inv_x, inv_w, lab, B, C, D, s, m, easy, g)
    assert R.relerr(h["dx"], xt.grad) < 2.0 ** -8 and R.relerr(h["dw"], wt.grad) < 2.0 ** -8
    # invalid labels: no loss, no gradient, the other rows unchanged
    lab2 = lab.clone()
    lab2[0], lab2[4] = -1, C
    r2 = R.arcface_rows(xn @ wn.t(), lab2, C, s, m, easy, g)
    assert r2["loss"][0] == 0 and r2["loss"][4] == 0 and r2["dcos"][0].abs().max() == 0
    assert torch.equal(r2["dcos"][1:4], r["dcos"][1:4]) and r2["dphi"][4] == 0


def test_arc_margin_branches_and_guards():
    cm, sm, th, mm = R.arc_consts(0.5)
    c = torch.tensor([1.0, -1.0, 0.0, 1e-30, -1e-30, th + 1e-9, th - 1e-9, 1.5], dtype=F64)
    phi, dphi = R.arc_margin(c, 0.5, True)
    assert torch.isfinite(phi).all() and torch.isfinite(dphi).all()
    assert dphi[0] == cm and dphi[1] == 1  # sin -> 0: the c / sin term is dropped; c = -1: no margin
    assert phi[2] == 0 and dphi[2] == 1 and abs(phi[3].item() + sm) < 1e-12 and phi[4] == c[4]
    assert phi[7] == phi[0]  # clamped
    phi_h, dphi_h = R.arc_margin(c, 0.5, False)
    assert abs(phi_h[5].item() - math.cos(math.acos(c[5].item()) + 0.5)) < 1e-7
    assert phi_h[6] == c[6] - mm and dphi_h[6] == 1
    assert R.near_ties(torch.tensor([[1.0, 2.0, 2.0 + 1e-6]], dtype=F64), torch.tensor([2.0], dtype=F64),
                       torch.tensor([[0.0, 1.0, 0.0]], dtype=F64), 1e-5).item() == 1


@pytest.mark.parametrize("kw", [dict(lr=0.125, momentum=0.0), dict(lr=0.25, momentum=0.875, dampening=0.125),
                                dict(lr=0.5, momentum=0.875, nesterov=True, weight_decay=0.0625)])
def test_sgd_reference_matches_torch_fp64(kw):
    # (dyadic hyper-parameters: no rounding anywhere in torch.optim either)
    torch.manual_seed(4)
    p = torch.randn(50, dtype=F64).requires_grad_(True)
    opt = torch.optim.SGD([p], **kw)
    q, buf = p.detach().clone(), None
    for step in range(4):
        g = torch.randn(50, dtype=F64)
        p.grad = g.clone()
        opt.step()
        q, buf = R.sgd_step(q, g, buf, step == 0, kw["lr"], kw["momentum"], kw.get("dampening", 0.0),
                            kw.get("weight_decay", 0.0), kw.get("nesterov", False))
        assert _close(q, p.detach())
        if kw["momentum"]:
            assert _close(buf, opt.state[p]["momentum_buffer"])
    q2, _ = R.sgd_step(q, g, None, True, 0.5, grad_scale=0.5)
    assert _close(q2, q - 0.25 * g)


@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_reference_matches_torch_fp64(decoupled):
    torch.manual_seed(5)
    kw = dict(lr=2.0 ** -7, betas=(0.75, 0.9375), eps=2.0 ** -10, weight_decay=0.125)
    p = torch.randn(50, dtype=F64).requires_grad_(True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], **kw)
    q, m, v = p.detach().clone(), torch.zeros(50, dtype=F64), torch.zeros(50, dtype=F64)
    for step in range(1, 6):
        g = torch.randn(50, dtype=F64)
        p.grad = g.clone()
        opt.step()
        q, m, v = R.adam_step(q, g, m, v, step, kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"], decoupled)
        assert _close(q, p.detach()) and _close(m, opt.state[p]["exp_avg"]) and _close(v, opt.state[p]["exp_avg_sq"])


def test_cdr_reference_cases():
    torch.manual_seed(6)
    ps = [torch.randn(8, 8), torch.randn(3, 3, 2, 2), torch.randn(7)]
    gs = [torch.randn_like(p) for p in ps]
    metric = torch.cat([(g * p).abs().reshape(-1) for p, g in zip(ps[:2], gs[:2])])
    n = metric.numel()
    thr, out = R.cdr_select(ps, gs, 0.5, 0.8)
    k = int(0.5 * n)
    assert thr == metric.sort(descending=True)[0][k - 1]
    assert sum(int((o != 0).sum()) for o in out[:2]) == k and torch.equal(out[2], gs[2])
    assert torch.equal(out[0][out[0] != 0], (gs[0] * torch.tensor(0.8))[out[0] != 0])
    thr1, out1 = R.cdr_select(ps, gs, 1.5 / n, 1.0)
    assert thr1 == metric.max() and sum(int((o != 0).sum()) for o in out1[:2]) == 1
    thrn, outn = R.cdr_select(ps, gs, 1.0, 1.0)
    assert thrn == metric.min() and torch.equal(outn[0], gs[0]) and torch.equal(outn[1], gs[1])
    thr0, out0 = R.cdr_select(ps, gs, 0.0, 1.0)
    assert math.isinf(float(thr0)) and out0[0].abs().max() == 0 and torch.equal(out0[2], gs[2])
    # ties at the threshold are all kept
    gt = [torch.ones(8, 8), torch.ones(3, 3, 2, 2) * 2, gs[2]]
    pt = [torch.ones(8, 8), torch.ones(3, 3, 2, 2), ps[2]]
    thrt, outt = R.cdr_select(pt, gt, 40 / n, 1.0)
    assert thrt == 1 and torch.equal(outt[0], gt[0]) and torch.equal(outt[1], gt[1])


def test_bf16_rule_and_row_relerr():
    ref = torch.tensor([[1.0, -3.0, 0.0]], dtype=F64)
    assert R.bf16_excess(ref.float().bfloat16(), ref, 0.0) <= 0
    assert R.bf16_excess(ref * (1 + 2.0 ** -7), ref, 0.0) > 0
    assert R.bf16_excess(ref + 1e-8, ref, 1e-7) <= 0
    assert R.row_relerr(torch.zeros(2, 3), torch.zeros(2, 3)).max() == 0
    assert abs(R.row_relerr(ref * 1.001, ref).item() - 1e-3) < 1e-9
