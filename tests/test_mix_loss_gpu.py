"""The two-label cross-entropy kernels (csrc/loss.hip, xent_mix_fwd / xent_mix_bwd) row by row
against the fp64 oracle of tests/mix_ref.py, and bit for bit against the one-label kernels where the
two coincide.

Rows and shapes are those of test_loss_rows_gpu.py, built afresh here: B = 12, the x40 row (3), the
constant row (4), the tie row (5), labels 0, C - 1 and the invalid -1 and C.  ``partner`` is the
flip, so the pairs are (0, 11), (1, 10), (2, 9), (3, 8), (4, 7), (5, 6): pair (0, 11) carries the
labels 0 and C - 1, pair (4, 7) the same label twice (a == b2), row 2 has an invalid own label and a
valid partner label, row 9 the converse, and rows 10 / 1 the same with the label C.
wlab cycles through {0, 1, 0.5, 0.3, 0.9}.

Tolerances: that file's rules.  rank exact (against the OWN label); loss within
2e-5 max(1, max|x|) -- a convex combination of two rows inside the rule is inside it, and the two
extra roundings add at most 2.4e-7 max|x|; fp32 gradient: row relative error <= 1e-5 and
|sum_j d_j| <= 1e-6 |g|; bf16 gradient: |got - ref| <= 2^-8 |ref| + 1e-7 |g|; rows with an invalid
label and the pad columns exactly 0.
"""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import head_ref as R
from tests import mix_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"

B = 12
GO = 0.37  # upstream gradient of the loss
XENT_SHAPES = [(1, 1), (10, 10), (64, 33), (257, 257), (520, 513), (2176, 2173)]
ROW_X40, ROW_CONST, ROW_TIE = 3, 4, 5
WLAB = [0.0, 1.0, 0.5, 0.3, 0.9]


@pytest.fixture(scope="module")
def K():
    return _ext.hip_ops()


def _rows(ld, C, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ld, generator=gen) * 2.0
    x[ROW_X40] *= 1.5 * 40.0
    x[ROW_CONST] = 1.5
    lab = torch.randint(0, C, (B,), generator=gen)
    x = x.to(dtype)
    if C > 1:
        lab[0], lab[11] = 0, C - 1
        lab[ROW_X40] = int(x[ROW_X40, :C].float().argmin())
        other = (int(lab[ROW_TIE]) + 1 + C // 2) % C
        if other == int(lab[ROW_TIE]):
            other = (other + 1) % C
        x[ROW_TIE, other] = x[ROW_TIE, lab[ROW_TIE]]
        lab[7] = lab[4]
        lab[2], lab[10] = -1, C
    partner = torch.arange(B - 1, -1, -1, dtype=torch.int32)
    wlab = torch.tensor([WLAB[b % len(WLAB)] for b in range(B)], dtype=torch.float32)
    return x, lab, partner, wlab


def _loss_tol(absmax):
    return 2e-5 * absmax.clamp_min(1.0)


def _check_grad(d, ref, valid, C, g, tag):
    dc = d.detach().cpu()
    assert dc.shape[0] == B and dc.shape[1] >= C, tag
    if dc.shape[1] > C:
        assert dc[:, C:].abs().max().item() == 0, tag
    if (~valid).any():
        assert dc[~valid].abs().max().item() == 0, tag
    if dc.dtype == torch.bfloat16:
        ex = R.bf16_excess(dc[:, :C], ref, 1e-7 * abs(g))
        assert ex <= 0, (tag, ex)
    else:
        assert dc.dtype == torch.float32
        rel = R.row_relerr(dc[:, :C], ref)
        print("xent_mix fp32 gradient row relerr / 1e-5", tag, rel.max().item() / 1e-5)
        assert rel.max().item() <= 1e-5, (tag, rel)
        assert R.f64(dc).sum(1).abs().max().item() <= 1e-6 * abs(g), (tag, R.f64(dc).sum(1))


def test_the_rows_are_the_ones_the_docstring_names():
    x, lab, partner, wlab = _rows(64, 33, torch.float32, 1)
    r = M.xent_mix_rows(x, lab, partner, wlab, 33)
    b2 = lab[partner.long()]
    assert lab[4] == b2[4] and r["valid"][4]
    assert not r["own_valid"][2] and 0 <= b2[2] < 33
    assert r["own_valid"][9] and b2[9] == -1
    assert lab[10] == 33 and r["own_valid"][1] and b2[1] == 33
    assert r["valid"].tolist() == [True, False, False, True, True, True, True, True, True, False, False, True]
    assert {lab[0].item(), b2[0].item()} == {0, 32}
    assert set(wlab.tolist()) == {0.0, 1.0, 0.5, float(torch.tensor(0.3)), float(torch.tensor(0.9))}


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ld,C", XENT_SHAPES)
def test_xent_mix_kernels_rows(K, ld, C, dtype, smoothing):
    x, lab, partner, wlab = _rows(ld, C, dtype, 100 + C)
    xd, labd, pd, wd = x.to(DEV), lab.to(DEV), partner.to(DEV), wlab.to(DEV)
    sm = R.f32(smoothing)
    ref = M.xent_mix_rows(x, lab, partner, wlab, C, sm)
    valid = ref["valid"]
    loss, rank = K.xent_mix_fwd(xd[:, :C], labd, pd, wd, C, smoothing)
    assert loss.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.equal(rank.cpu().long()[ref["own_valid"]], ref["rank"][ref["own_valid"]])
    err = (R.f64(loss) - ref["loss"]).abs()
    print("xent_mix loss err / tol", (err / _loss_tol(ref["absmax"])).max().item())
    assert (err <= _loss_tol(ref["absmax"])).all(), (err, ref["absmax"])
    assert (R.f64(loss)[~valid] == 0).all()
    # the padded buffer gives the same rows
    loss_p, rank_p = K.xent_mix_fwd(xd, labd, pd, wd, C, smoothing)
    assert torch.equal(loss_p, loss) and torch.equal(rank_p, rank)
    go = torch.tensor([GO], device=DEV)
    g = R.f32(GO) * R.f32(1.0 / B)
    dref = M.xent_mix_grad(x, lab, partner, wlab, C, g, sm)
    for out_bf16 in (False, True):
        d = K.xent_mix_bwd(xd[:, :C], labd, pd, wd, C, go, 1.0 / B, smoothing, out_bf16)
        assert d.shape == (B, C) and d.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
        _check_grad(d, dref, valid, C, g, ("slice", out_bf16))
        d = K.xent_mix_bwd(xd, labd, pd, wd, C, go, 1.0 / B, smoothing, out_bf16)
        assert d.shape == (B, ld)
        _check_grad(d, dref, valid, C, g, ("padded", out_bf16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ld,C", XENT_SHAPES)
def test_weight_one_and_zero_are_the_one_label_kernels_bit_for_bit(K, ld, C, dtype):
    """Smoothing 0, rows with both labels valid: wlab = 1 is xent_fwd / xent_bwd on labels, wlab = 0 on
    labels[partner] -- loss and gradient, torch.equal."""
    x, lab, partner, wlab = _rows(ld, C, dtype, 300 + C)
    xd, labd, pd = x.to(DEV), lab.to(DEV), partner.to(DEV)
    lab2 = lab[partner.long()]
    lab2d = lab2.to(DEV)
    valid = M.xent_mix_rows(x, lab, partner, wlab, C)["valid"]
    go = torch.tensor([GO], device=DEV)
    loss_a, rank_a = K.xent_fwd(xd[:, :C], labd, C, 0.0)
    loss_b, _ = K.xent_fwd(xd[:, :C], lab2d, C, 0.0)
    for w in (wlab, torch.ones(B), torch.zeros(B)):
        ones, zeros = valid & (w == 1), valid & (w == 0)
        assert (ones | zeros).sum() >= (4 if C > 1 else 1)
        loss, rank = K.xent_mix_fwd(xd[:, :C], labd, pd, w.to(DEV), C, 0.0)
        assert torch.equal(rank, rank_a)
        assert torch.equal(loss.cpu()[ones], loss_a.cpu()[ones])
        assert torch.equal(loss.cpu()[zeros], loss_b.cpu()[zeros])
        for out_bf16 in (False, True):
            for logits in (xd[:, :C], xd):
                d = K.xent_mix_bwd(logits, labd, pd, w.to(DEV), C, go, 1.0 / B, 0.0, out_bf16).cpu()
                da = K.xent_bwd(logits, labd, C, go, 1.0 / B, 0.0, out_bf16).cpu()
                db = K.xent_bwd(logits, lab2d, C, go, 1.0 / B, 0.0, out_bf16).cpu()
                assert torch.equal(d[ones], da[ones]) and torch.equal(d[zeros], db[zeros]), (out_bf16, logits.shape)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ld,C", XENT_SHAPES)
def test_cross_entropy_mix_autograd(ld, C, dtype, smoothing, reduction):
    """Fn.cross_entropy(mix=...) forward and backward on the slice and on the padded buffer."""
    x, lab, partner, wlab = _rows(ld, C, dtype, 200 + C)
    sm = R.f32(smoothing)
    ref = M.xent_mix_rows(x, lab, partner, wlab, C, sm)
    scale = 1.0 / B if reduction == "mean" else 1.0
    g = R.f32(GO) * R.f32(scale)
    dref = M.xent_mix_grad(x, lab, partner, wlab, C, g, sm)
    tol = _loss_tol(ref["absmax"]).sum().item() * scale
    for padded in (False, True):
        leaf = x.to(DEV).requires_grad_(True)
        logits = leaf if padded else leaf[:, :C]
        loss, rank = Fn.cross_entropy(logits, lab.to(DEV), C, smoothing=smoothing, reduction=reduction,
                                      return_rank=True, mix=(partner.to(DEV), wlab.to(DEV)))
        assert abs(loss.item() - ref["loss"].sum().item() * scale) <= tol, (loss.item(), ref["loss"].sum() * scale)
        assert torch.equal(rank.cpu().long()[ref["own_valid"]], ref["rank"][ref["own_valid"]])
        (loss * GO).backward()
        assert leaf.grad.dtype == dtype and leaf.grad.shape == (B, ld)
        _check_grad(leaf.grad, dref, ref["valid"], C, g, (padded, reduction))


def test_ops_check_their_plan(K):
    x, lab, partner, wlab = _rows(64, 33, torch.float32, 5)
    xd, labd, pd, wd = x.to(DEV), lab.to(DEV), partner.to(DEV), wlab.to(DEV)
    with pytest.raises(RuntimeError, match="partner int32"):
        K.xent_mix_fwd(xd, labd, pd.long(), wd, 33, 0.0)
    with pytest.raises(RuntimeError, match="wlab fp32"):
        K.xent_mix_fwd(xd, labd, pd, wd[:5], 33, 0.0)
    with pytest.raises(RuntimeError, match="partner int32"):
        K.xent_mix_bwd(xd, labd, partner, wd, 33, torch.ones(1, device=DEV), 1.0, 0.0, False)
