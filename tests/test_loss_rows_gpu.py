"""The row kernels every workload ends its step in -- softmax cross-entropy, log-softmax (csrc/loss.hip)
and the nested-dropout prefix mask (csrc/misc.hip) -- against fp64 references evaluated on exactly
the values the kernels read (tests/head_ref.py), row by row.

Tolerances (per row, never a norm over the batch):
  * rank: exact (there is no arithmetic between the inputs and the compare);
  * loss / log-probabilities: |err| <= 2e-5 max(1, max_j |x_j|): two fp32 roundings of magnitudes up
    to max |x| (2 * 2^-24 * 120 = 1.4e-5 on the x40 row) plus ~1e-6 for the fast exp / log;
  * fp32 gradient: row relative error <= 1e-5 and |sum_j d_j| <= 1e-6 |g| (softmax - target sums to 0);
  * bf16 gradient: |got - ref| <= 2^-8 |ref| + atol (one bf16 rounding of the exact value), atol the
    fp32 error of the quantity: 1e-7 |g| for the cross-entropy gradient (p <= 1 carries ~2^-24);
  * invalid-label rows (label outside [0, C)): loss and gradient row exactly 0 -- the mean still
    divides by B, so they are NOT compared with torch's ignore_index mean;
  * pad columns [C, size(1)): exactly 0.
"""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

B = 12
GO = 0.37  # upstream gradient of the loss

# one class; fewer than 256 classes; a padded buffer; one class past the 256-thread stride; ragged pads
XENT_SHAPES = [(1, 1), (10, 10), (64, 33), (257, 257), (520, 513), (2176, 2173)]
ROW_X40, ROW_CONST, ROW_TIE = 3, 4, 5


@pytest.fixture(scope="module")
def K():
    return _ext.hip_ops()


def _rows(ld, C, dtype, seed):
    """[B, ld] logits (rounded to dtype) and labels.  Row 3 is scaled x40 (|x| ~ 120: overflows
    without the max subtraction; its label is its smallest logit, so the gradient keeps two O(g)
    entries), row 4 is constant, row 5 has another class exactly equal to the label's logit (ties go
    to the label); labels include 0, C - 1 and the invalid -1 and C."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ld, generator=gen) * 2.0
    x[ROW_X40] *= 1.5 * 40.0  # 3 randn, x40
    x[ROW_CONST] = 1.5
    lab = torch.randint(0, C, (B,), generator=gen)
    lab[0], lab[1] = 0, C - 1
    x = x.to(dtype)
    if C > 1:
        lab[ROW_X40] = int(x[ROW_X40, :C].float().argmin())
        other = (int(lab[ROW_TIE]) + 1 + C // 2) % C
        if other == int(lab[ROW_TIE]):
            other = (other + 1) % C
        x[ROW_TIE, other] = x[ROW_TIE, lab[ROW_TIE]]
        lab[2], lab[6] = -1, C
    return x, lab


def _loss_tol(absmax):
    return 2e-5 * absmax.clamp_min(1.0)


def _check_grad(d, ref, valid, C, g, tag):
    """d [B, W] (fp32 or bf16) against ref [B, C]: pads and invalid rows exactly zero, then the fp32
    or the bf16 rule."""
    dc = d.detach().cpu()
    assert dc.shape[0] == B and dc.shape[1] >= C, tag
    assert dc[:, C:].abs().max().item() == 0 if dc.shape[1] > C else True, tag
    assert dc[~valid].abs().max().item() == 0 if (~valid).any() else True, tag
    if dc.dtype == torch.bfloat16:
        ex = R.bf16_excess(dc[:, :C], ref, 1e-7 * abs(g))
        assert ex <= 0, (tag, ex)
    else:
        assert dc.dtype == torch.float32
        rel = R.row_relerr(dc[:, :C], ref)
        print("fp32 gradient row relerr", tag, rel.max().item())
        assert rel.max().item() <= 1e-5, (tag, rel)
        assert R.f64(dc).sum(1).abs().max().item() <= 1e-6 * abs(g), (tag, R.f64(dc).sum(1))


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ld,C", XENT_SHAPES)
def test_xent_kernels_rows(K, ld, C, dtype, smoothing):
    x, lab = _rows(ld, C, dtype, 100 + C)
    xd, ld_ = x.to(DEV), lab.to(DEV)
    ref = R.xent_rows(x, lab, C, smoothing)
    valid = ref["valid"]
    loss, rank = K.xent_fwd(xd[:, :C], ld_, C, smoothing)
    assert torch.equal(rank.cpu().long()[valid], ref["rank"][valid])
    err = (R.f64(loss) - ref["loss"]).abs()
    print("xent loss err / tol", (err / _loss_tol(ref["absmax"])).max().item())
    assert (err <= _loss_tol(ref["absmax"])).all(), (err, ref["absmax"])
    assert (R.f64(loss)[~valid] == 0).all()
    go = torch.tensor([GO], device=DEV)
    g = R.f32(GO) * R.f32(1.0 / B)
    dref = R.xent_grad(x, lab, C, g, smoothing)
    for out_bf16 in (False, True):
        # on the [:, :C] slice of the padded buffer, and on the whole buffer with C < size(1)
        d = K.xent_bwd(xd[:, :C], ld_, C, go, 1.0 / B, smoothing, out_bf16)
        assert d.shape == (B, C) and d.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
        _check_grad(d, dref, valid, C, g, ("slice", out_bf16))
        d = K.xent_bwd(xd, ld_, C, go, 1.0 / B, smoothing, out_bf16)
        assert d.shape == (B, ld)
        _check_grad(d, dref, valid, C, g, ("padded", out_bf16))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ld,C", XENT_SHAPES)
def test_cross_entropy_autograd(ld, C, dtype, smoothing, reduction):
    """Fn.cross_entropy forward and backward (bf16 logits take the bf16 gradient branch), on the
    slice and on the padded buffer, mean and sum."""
    x, lab = _rows(ld, C, dtype, 200 + C)
    ref = R.xent_rows(x, lab, C, smoothing)
    scale = 1.0 / B if reduction == "mean" else 1.0
    g = R.f32(GO) * R.f32(scale)
    dref = R.xent_grad(x, lab, C, g, smoothing)
    # the sum of the B row bounds (the mean divides it by B)
    tol = _loss_tol(ref["absmax"]).sum().item() * scale
    for padded in (False, True):
        leaf = x.to(DEV).requires_grad_(True)
        logits = leaf if padded else leaf[:, :C]
        loss, rank = Fn.cross_entropy(logits, lab.to(DEV), C, smoothing=smoothing, reduction=reduction,
                                      return_rank=True)
        assert abs(loss.item() - ref["loss"].sum().item() * scale) <= tol, (loss.item(), ref["loss"].sum() * scale)
        assert torch.equal(rank.cpu().long()[ref["valid"]], ref["rank"][ref["valid"]])
        (loss * GO).backward()
        assert leaf.grad.dtype == dtype and leaf.grad.shape == (B, ld)
        _check_grad(leaf.grad, dref, ref["valid"], C, g, (padded, reduction))


# ----------------------------------------------------------------------------- log-softmax
LSM_C = [1, 33, 256, 257, 1000]


def _lsm_rows(C, ld, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ld, generator=gen) * 2.0
    x[ROW_X40] *= 1.5 * 40.0  # 3 randn, x40
    x[:, C:] = 50.0  # columns past C belong to the wider buffer: never read
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", LSM_C)
def test_log_softmax_kernels_rows(K, C, dtype):
    ld = C + 7
    x = _lsm_rows(C, ld, dtype, 300 + C)
    y = K.log_softmax_fwd(x.to(DEV)[:, :C], C)
    assert y.shape == (B, C) and y.dtype == torch.float32
    ref = R.log_softmax_rows(x, C)
    tol = _loss_tol(R.f64(x)[:, :C].abs().amax(1))
    err = (R.f64(y) - ref).abs().amax(1)
    print("log_softmax err / tol", (err / tol).max().item())
    assert (err <= tol).all(), (err, tol)
    # backward from the kernel's own y; dy has a non-zero row sum
    gen = torch.Generator().manual_seed(400 + C)
    dy = torch.randn(B, C, generator=gen) + 0.25
    dref = R.log_softmax_grad(y, dy)
    # fp32 error of dy_j - p_j S before the output rounding: both terms are bounded by
    # M = max |dy| + |S|; their roundings and the C-term fp32 sum S stay below 2^-20 M
    S = R.f64(dy).sum(1)
    atol = (2.0 ** -20) * (R.f64(dy).abs().amax(1) + S.abs())
    for ldo in (C, C + 5):
        for out_bf16 in (False, True):
            dx = K.log_softmax_bwd(y, dy.to(DEV), ldo, out_bf16).cpu()
            assert dx.shape == (B, ldo) and dx.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
            if ldo > C:
                assert dx[:, C:].abs().max().item() == 0
            if out_bf16:
                ex = R.bf16_excess(dx[:, :C], dref, atol[:, None])
                assert ex <= 0, (ldo, ex)
            else:
                rel = R.row_relerr(dx[:, :C], dref)
                assert rel.max().item() <= 1e-5, (ldo, rel)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", LSM_C)
def test_log_softmax_then_cross_entropy(C, dtype):
    """Fn.log_softmax -> Fn.cross_entropy as the CDR workload chains them, on a padded buffer.
    The reference is cross-entropy of the raw logits (log-softmax is idempotent under it), under the
    same rules as the cross-entropy kernels alone: the fp32 log-probabilities between the two kernels
    cost nothing visible -- an error of a row's lse is a common shift that the second softmax
    removes, and the rounding of lp_j moves p_j by at most p_j |lp_j| 2^-24 <= 2^-24 / e."""
    ld = C + 7
    x = _lsm_rows(C, ld, dtype, 500 + C)
    gen = torch.Generator().manual_seed(600 + C)
    lab = torch.randint(0, C, (B,), generator=gen)
    lab[0], lab[1] = 0, C - 1
    if C > 1:
        lab[2], lab[6] = -1, C
        lab[ROW_X40] = int(x[ROW_X40, :C].float().argmin())
    ref = R.xent_rows(x, lab, C)
    g = R.f32(GO) * R.f32(1.0 / B)
    dref = R.xent_grad(x, lab, C, g)
    leaf = x.to(DEV).requires_grad_(True)
    lp = Fn.log_softmax(leaf, C)
    assert lp.shape == (B, C) and lp.dtype == torch.float32
    loss = Fn.cross_entropy(lp, lab.to(DEV), C)
    rows, _ = Fn.cross_entropy_rows(lp.detach(), lab.to(DEV), C)
    err = (R.f64(rows) - ref["loss"]).abs()
    print("log_softmax -> xent loss err / tol", (err / _loss_tol(ref["absmax"])).max().item())
    assert (err <= _loss_tol(ref["absmax"])).all(), (err, ref["absmax"])
    assert abs(loss.item() - ref["loss"].sum().item() / B) <= _loss_tol(ref["absmax"]).sum().item() / B
    (loss * GO).backward()
    assert leaf.grad.dtype == dtype and leaf.grad.shape == (B, ld)
    _check_grad(leaf.grad, dref, ref["valid"], C, g, ("chain", C))


# ----------------------------------------------------------------------------- prefix mask
@pytest.mark.parametrize("Bm,D", [(3, 5), (37, 300)])
def test_prefix_mask_exact(K, Bm, D):
    """x * (arange(D) < keep), exactly; B * D is no multiple of the 256-thread block; keep past D
    keeps everything.  Directly and through Fn.nested_mask forward and backward."""
    gen = torch.Generator().manual_seed(700 + D)
    x = torch.randn(Bm, D, generator=gen).bfloat16()
    dy = torch.randn(Bm, D, generator=gen).bfloat16()
    for keep in (1, D - 1, D, D + 7):
        kt = torch.full((1,), keep, dtype=torch.int32, device=DEV)
        assert torch.equal(K.prefix_mask(x.to(DEV), kt).cpu(), R.prefix_mask(x, keep)), keep
        leaf = x.to(DEV).requires_grad_(True)
        y = Fn.nested_mask(leaf, keep - 1)
        y.backward(dy.to(DEV))
        assert torch.equal(y.detach().cpu(), R.prefix_mask(x, keep)), keep
        assert torch.equal(leaf.grad.cpu(), R.prefix_mask(dy, keep)), keep
