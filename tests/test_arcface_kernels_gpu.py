"""The ArcFace head's kernels one by one against fp64 references on exactly the values they read
(tests/head_ref.py): the L2 normalisation and its backward, the bf16 transpose, the unfused margin
kernels on a constructed cosine matrix that sits on every branch point, the evaluation path
(Fn.arcface_rows), and the fused head (csrc/arcface.hip) on the operands its own normalisation
kernel returned.

Rules: a bf16 output obeys |got - ref| <= 2^-8 |ref| + atol (one bf16 rounding; atol = the fp32
error of the quantity, derived at each use); loss / lse rows obey |err| <= 2e-5 max(1, max |x|)
with max |x| = s; a label rank may differ from the fp64 count by at most the number of classes
whose logit lies within a stated band of the target logit.

Fused head, dX and dW: bf16 rounding of dcos flips where the fp32 and the fp64 value straddle a
rounding boundary, so there is no derivable bound; measured on an MI355X against the fp64
reference on the kernel's own operands, over the 12 cases of test_fused_head_matched_operands
(per shape, fp32 / bf16 features, easy / hard margin: dX, dW relative error):
    (70, 130, 100)   fp32 9.0e-8 / 9.1e-8, 8.3e-8 / 8.4e-8    bf16 1.67e-3 / 1.67e-3, 8.4e-8 / 8.5e-8
    (64, 700, 256)   fp32 8.0e-7 / 4.4e-7, 8.0e-7 / 4.6e-7    bf16 1.68e-3 / 1.68e-3, 8.0e-7 / 1.8e-6
    (130, 1100, 128) fp32 5.3e-7 / 6.0e-7, 5.2e-7 / 5.8e-7    bf16 1.65e-3 / 1.67e-3, 1.1e-6 / 1.1e-6
    largest: dX with an fp32 output 8.04e-7, dW 1.82e-6 (the bf16 dX is its output rounding).
The assertions are 4x the largest value, rounded up to one digit: FUSED_DX_TOL = 4e-6,
FUSED_DW_TOL = 8e-6 -- four orders below the 3e-2 that the comparison with an fp32 reference on
unrounded operands needs (test_arcface_fused_gpu.py).  A bf16 dX is held element by element to one
bf16 rounding of the reference, with FUSED_DX_TOL |dX| as its absolute term.  The kernels are
deterministic (fixed summation order) and the inputs come from seeded CPU generators, so the figures
repeat; they are this small because at these seeds no flip lands on a label column, whose dcos
dominates its row (one such flip would cost ~5e-4).
"""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

S, M = 30.0, 0.5
GO = 0.37
FUSED_DX_TOL = 4e-6  # 4 x the measured 8.04e-7 (see the module docstring)
FUSED_DW_TOL = 8e-6  # 4 x the measured 1.82e-6


@pytest.fixture(scope="module")
def K():
    return _ext.hip_ops()


def _loss_tol(s):
    return 2e-5 * max(1.0, s)


# ----------------------------------------------------------------------------- l2norm_rows / l2norm_bwd
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Rr,D,ldo,rows_out",
                         [(1, 1, 8, -1), (5, 200, 200, -1), (5, 200, 208, 64), (70, 512, 512, 128)])
def test_l2norm_rows(K, Rr, D, ldo, rows_out, dtype):
    gen = torch.Generator().manual_seed(Rr * 1000 + D)
    x = (torch.randn(Rr, D, generator=gen) * 3.0).to(dtype)
    if Rr > 2:
        x[2] = 0  # an all-zero row: y = 0, inv = 1 / eps (finite)
    y, inv = K.l2norm_rows(x.to(DEV), ldo, 1e-12, rows_out)
    Ro = Rr if rows_out < 0 else rows_out
    assert y.shape == (Ro, ldo) and y.dtype == torch.bfloat16 and inv.shape == (Ro,) and inv.dtype == torch.float32
    y, inv = y.cpu(), inv.cpu()
    yr, ir = R.l2norm_rows(x, 1e-12)
    # |y| <= 1: the fp32 product x * inv carries ~2^-24 before the bf16 rounding
    ex = R.bf16_excess(y[:Rr, :D], yr, 1e-7)
    assert ex <= 0, ex
    rel = ((R.f64(inv[:Rr]) - ir).abs() / ir).max().item()
    assert rel <= 1e-6, rel
    assert torch.isfinite(inv).all()
    if Rr > 2:
        assert y[2].abs().max().item() == 0 and inv[2].item() > 1e11
    # padding columns and rows exactly zero, inverse norm 0
    assert y[:, D:].abs().max().item() == 0 if ldo > D else True
    if Ro > Rr:
        assert y[Rr:].abs().max().item() == 0 and inv[Rr:].abs().max().item() == 0


@pytest.mark.parametrize("out_bf16", [False, True], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16], ids=["dy_fp32", "dy_bf16"])
def test_l2norm_bwd(K, dy_dtype, out_bf16):
    """dx = inv (dy - y <dy, y>) with D = 200 inside 208-wide dy and y buffers (ldd, ldy > D) whose
    pad columns hold values that must not be read.  The dot product cancels (dy is made nearly
    parallel to y on two rows), so the tolerance is relative to the operand inv |dy_row|."""
    Rr, D, ld = 7, 200, 208
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(Rr, D, generator=gen) * 2.0
    y, inv = K.l2norm_rows(x.to(DEV), ld, 1e-12, -1)
    y = y.clone()
    y[:, D:] = 3.0
    dy = torch.randn(Rr, ld, generator=gen)
    dy[1, :D] = 5.0 * y[1, :D].float().cpu() + 1e-3 * dy[1, :D]
    dy[4, :D] = -2.0 * y[4, :D].float().cpu()
    dy[:, D:] = 100.0
    dy = dy.to(dy_dtype)
    dx = K.l2norm_bwd(dy.to(DEV), y, inv, D, out_bf16)
    assert dx.shape == (Rr, D) and dx.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    ref = R.l2norm_grad(dy, y, inv, D)
    opnd = R.f64(inv) * R.f64(dy)[:, :D].norm(dim=1)  # inv |dy_row|
    if out_bf16:
        ex = R.bf16_excess(dx, ref, (1e-5 * opnd)[:, None])
        assert ex <= 0, ex
    else:
        err = (R.f64(dx) - ref).norm(dim=1)
        assert (err <= 1e-5 * opnd).all(), (err / opnd)


@pytest.mark.parametrize("Rr,C", [(1, 1), (63, 65), (64, 64), (130, 70), (704, 208)])
def test_transpose2d_exact(K, Rr, C):
    gen = torch.Generator().manual_seed(Rr + C)
    x = torch.randn(Rr, C, generator=gen).bfloat16()
    yt = K.transpose2d(x.to(DEV))
    assert yt.shape == (C, Rr) and torch.equal(yt.cpu(), x.t().contiguous())


# ----------------------------------------------------------------------------- unfused margin kernels
def _bf16_step(v, up):
    """The bf16 neighbour of bf16 value v towards +inf (up) or -inf."""
    b = int(torch.tensor([v], dtype=torch.bfloat16).view(torch.int16).item()) & 0xFFFF
    if (b & 0x7FFF) == 0:
        b = 0x0001 if up else 0x8001
    else:
        neg, mag = b & 0x8000, b & 0x7FFF
        mag += 1 if up != bool(neg) else -1
        b = neg | mag
    return float(torch.tensor([b - 0x10000 if b >= 0x8000 else b], dtype=torch.int16).view(torch.bfloat16).item())


def _bf16_around(v):
    """(largest bf16 < v, smallest bf16 > v) for a v that is no bf16 value."""
    t = float(torch.tensor([v], dtype=torch.bfloat16).item())
    assert t != v
    return (_bf16_step(t, False), t) if t > v else (t, _bf16_step(t, True))


BM = 16
ROW_TIE, ROW_NEAR, ROW_NEG1, ROW_BIGC = 10, 11, 8, 9
COS_NEAR = 0.48046875  # bf16 next to sin(m): phi = cos(theta + m) ~ 0, where the bf16 grid is finer than 1e-5


def _cos_case(C, ld, seed):
    """A bf16 cosine matrix [16, ld] whose label column sits on the margin's branch points: +-1 (the
    sin -> 0 guard), 0 and its two bf16 neighbours (the easy margin's switch), the bf16 neighbours of
    cos(pi - m) (the hard margin's switch), 0.996 (255 / 256); rows 8 / 9 carry the labels -1 / C;
    row 10 has a second class at exactly the label's cosine (-0.5: an exact tie where no margin applies,
    i.e. under the easy margin); row 11 has its label at 0.4805, where both margins give phi ~ 0, and a
    second class at the bf16 value next to phi (a near-tie within 1e-5 under either margin).  Pad
    columns hold 0.99 (never read)."""
    gen = torch.Generator().manual_seed(seed)
    cos = (torch.rand(BM, ld, generator=gen) * 1.8 - 0.9).bfloat16()
    cos[:, C:] = 0.99
    lab = torch.randint(0, C, (BM,), generator=gen)
    lab[0], lab[1] = 0, C - 1
    th = R.arc_consts(M)[2]
    lo, hi = _bf16_around(th)
    assert lo < th < hi
    special = [1.0, -1.0, 0.0, _bf16_step(0.0, True), _bf16_step(0.0, False), lo, hi, 0.99609375]
    assert special[3] > 0 > special[4]
    for r, v in enumerate(special):
        cos[r, lab[r]] = v
        assert float(cos[r, lab[r]]) == v  # (the two subnormal neighbours of 0 included)
    cos[ROW_TIE, lab[ROW_TIE]] = -0.5
    cos[ROW_NEAR, lab[ROW_NEAR]] = COS_NEAR
    for r in range(BM):  # no accidental copy of a label's cosine among the random ones
        same = cos[r, :C] == cos[r, lab[r]]
        same[lab[r]] = False
        cos[r, :C][same] = 0.25
    cos[ROW_TIE, (int(lab[ROW_TIE]) + 7) % C] = -0.5
    phi_near = R.arc_margin(torch.tensor([COS_NEAR], dtype=torch.float64), M, True)[0].item()
    cos[ROW_NEAR, (int(lab[ROW_NEAR]) + 7) % C] = phi_near  # rounds to the bf16 neighbour of phi
    lab[ROW_NEG1], lab[ROW_BIGC] = -1, C
    return cos, lab


@pytest.mark.parametrize("want_logits", [False, True], ids=["nologits", "logits"])
@pytest.mark.parametrize("easy", [True, False], ids=["easy", "hard"])
@pytest.mark.parametrize("C,ld", [(70, 128), (300, 320)])
def test_arcface_margin_kernels_branch_points(K, C, ld, easy, want_logits):
    cos, lab = _cos_case(C, ld, 900 + C)
    cd, labd = cos.to(DEV), lab.to(DEV)
    loss, rank, dphi, logits = K.arcface_fwd(cd, labd, C, S, M, easy, want_logits)
    ref = R.arcface_rows(cos, lab, C, S, M, easy)
    valid = ref["valid"]
    # loss rows (max |x| = s), invalid rows exactly 0
    err = (R.f64(loss) - ref["loss"]).abs()
    print("arcface_fwd loss err / tol", (err / _loss_tol(S)).max().item())
    assert (err <= _loss_tol(S)).all(), err
    assert (R.f64(loss)[~valid] == 0).all() and (R.f64(dphi)[~valid] == 0).all()
    # d phi / d cos under the same sin > 1e-6 guard
    rel = ((R.f64(dphi) - ref["dphi"]).abs() / ref["dphi"].abs().clamp_min(1e-30))[valid]
    assert rel.max().item() <= 1e-5, rel
    # rank: s * phi is rounded in fp32, so classes within 1e-5 s of the target may fall either side;
    # by construction that happens only on the two tie rows (the exact tie only without a margin there)
    ties = R.near_ties(ref["x"], ref["t"], ref["onehot"], 1e-5 * S)
    assert ties[[r for r in range(BM) if r not in (ROW_TIE, ROW_NEAR)]].max().item() == 0
    assert ties[ROW_TIE].item() == (1 if easy else 0) and ties[ROW_NEAR].item() == 1
    assert ((rank.cpu().long() - ref["rank"]).abs() <= ties)[valid].all(), (rank.cpu(), ref["rank"])
    if want_logits:
        # s * cos: one fp32 rounding; s * phi: four (<= 4 * 2^-24 s)
        assert logits.shape == (BM, C) and (R.f64(logits) - ref["x"]).abs().max().item() <= 1e-6 * S
    else:
        assert logits.numel() == 0
    # backward, from the forward kernel's own dphi
    go = torch.tensor([GO], device=DEV)
    g = R.f32(GO) * R.f32(1.0 / BM)
    dcos = K.arcface_bwd(cd, labd, C, S, M, easy, dphi, go, 1.0 / BM).cpu()
    assert dcos.shape == (BM, ld) and dcos.dtype == torch.bfloat16
    rb = R.arcface_rows(cos, lab, C, S, M, easy, g, dphi=dphi)
    assert dcos[:, C:].abs().max().item() == 0 and dcos[~valid].abs().max().item() == 0
    # fp32 error of g s (p - onehot) mult before the rounding: the logits s cos carry 2^-24 s each, so
    # p = exp(x - lse) carries a relative 2 * 2^-23 s plus the fast exp / log (~2e-6); p <= 1
    mult = 1.0 + rb["onehot"] * (R.f64(dphi).abs()[:, None] - 1.0)
    atol = abs(g) * S * mult * ((2.0 ** -22) * S + 2e-6)
    ex = R.bf16_excess(dcos[:, :C], rb["dcos"], atol)
    assert ex <= 0, ex


@pytest.mark.parametrize("with_margin,easy", [(True, True), (True, False), (False, True)],
                         ids=["margin-easy", "margin-hard", "plain"])
def test_arcface_rows_eval_path(K, with_margin, easy):
    """Fn.arcface_rows (the ArcFace evaluation path): D = 200 -> Dp = 200, C = 130 -> Cp = 192.
    Checked link by link: the bf16 cosines of the project's GEMM against the fp64 product of the
    normalised operands the kernel produced, then loss and rank against the fp64 reference on those
    cosines.  ``with_margin=False`` is cross-entropy of the plain SCALED cosines s * cos."""
    Bm, C, D = 20, 130, 200
    gen = torch.Generator().manual_seed(321)
    x = torch.randn(Bm, D, generator=gen)
    W = torch.randn(C, D, generator=gen) * 0.05
    lab = torch.randint(0, C, (Bm,), generator=gen)
    lab[3], lab[4] = -1, C
    x[0] = W[lab[0]] * 3.0  # cos ~ 1
    xd, Wd, labd = x.to(DEV), W.to(DEV), lab.to(DEV)
    loss, rank = Fn.arcface_rows(xd, Wd, labd, S, M, easy, with_margin)
    xn, _ = K.l2norm_rows(xd, 200, 1e-12, -1)
    wn, _ = K.l2norm_rows(Wd, 200, 1e-12, 192)
    cos = K.linear_fwd(xn, wn, None, 0)
    assert cos.shape == (Bm, 192) and cos.dtype == torch.bfloat16
    exact = R.f64(xn) @ R.f64(wn)[:C].t()
    # an fp32-accumulated dot of 200 products of magnitude <= 1: <= 200 * 2^-24 before the rounding
    ex = R.bf16_excess(cos[:, :C], exact, 200 * 2.0 ** -24)
    assert ex <= 0, ex
    ref = R.arcface_rows(cos, lab, C, S, M if with_margin else 0.0, easy)
    valid = ref["valid"]
    err = (R.f64(loss) - ref["loss"]).abs()
    print("arcface_rows loss err / tol", (err / _loss_tol(S)).max().item())
    assert (err <= _loss_tol(S)).all(), (err, loss, ref["loss"])
    ties = R.near_ties(ref["x"], ref["t"], ref["onehot"], 1e-5 * S)
    assert ((rank.cpu().long() - ref["rank"]).abs() <= ties)[valid].all(), (rank.cpu(), ref["rank"], ties)


# ----------------------------------------------------------------------------- fused head
FUSED_SHAPES = [
    (70, 130, 100),    # Dp = 128, 3 class tiles -> 3 splits (not remapped), D padded, 2 dW row splits
    (64, 700, 256),    # 11 tiles -> 8 splits of 2 tiles, the last two empty; XCD remap, one row block
    (130, 1100, 128),  # 3 row blocks, 18 tiles -> 16 splits (7 empty), remap with RB = 3, 3 dW row splits
]


def _fused_case(K, B, C, D, dtype, easy, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=gen)
    W = torch.randn(C, D, generator=gen) * 0.05
    lab = torch.randint(0, C, (B,), generator=gen)
    lab[0], lab[1] = 0, C - 1
    x[:3] = W[lab[:3]]          # cos ~ 1: the margin's sin -> 0 guard
    lab[5], lab[6] = -1, C + 3  # invalid labels
    x = x.to(dtype)
    Dp = 128 if D <= 128 else 256
    Bp, Cp = Fn.round_up(B, 64), Fn.round_up(C, 64)
    xd, Wd, labd = x.to(DEV), W.to(DEV), lab.to(DEV)
    xn, xnT, inv_x = K.arcface_l2norm_t(xd, Bp, Dp, 1e-12)
    wn, wnT, inv_w = K.arcface_l2norm_t(Wd, Cp, Dp, 1e-12)
    # the operands themselves: normalised rows, exact transposes, zero padding, inverse norm 0 there
    for src, n, nT, inv, rows in ((x, xn, xnT, inv_x, B), (W, wn, wnT, inv_w, C)):
        yr, ir = R.l2norm_rows(src, 1e-12)
        assert R.bf16_excess(n[:rows, :D], yr, 1e-7) <= 0
        assert ((R.f64(inv)[:rows] - ir).abs() / ir).max().item() <= 1e-6
        assert torch.equal(nT, n.t().contiguous())
        if n.shape[0] > rows:
            assert n[rows:].abs().max().item() == 0 and inv[rows:].abs().max().item() == 0
        if Dp > D:
            assert n[:, D:].abs().max().item() == 0
    go = torch.tensor([GO], device=DEV)
    loss, rank, lse, labt = K.arcface_fused_fwd(xn, wn, labd, B, C, S, M, easy)
    dx = K.arcface_fused_dx(xn, wn, wnT, labd, lse, labt, go, 1.0 / B, inv_x, B, C, D, S, dtype == torch.bfloat16)
    dw = K.arcface_fused_dw(xn, xnT, wn, labd, lse, labt, go, 1.0 / B, inv_w, B, C, D, S)
    torch.cuda.synchronize()
    g = R.f32(GO) * R.f32(1.0 / B)
    ref = R.arcface_head(xn, wn, inv_x, inv_w, lab, B, C, D, S, M, easy, g)
    return dict(loss=loss, rank=rank, lse=lse, dx=dx, dw=dw, ref=ref, Dp=Dp)


@pytest.mark.parametrize("easy", [True, False], ids=["easy", "hard"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C,D", FUSED_SHAPES)
def test_fused_head_matched_operands(K, B, C, D, dtype, easy):
    """arcface_l2norm_t -> arcface_fused_fwd / _dx / _dw (the bound ops, not the autograd wrapper)
    against the fp64 head on the xn, wn and inverse norms the normalisation kernel returned.  The
    measured dX / dW errors and the derivation of every other bound: the module docstring."""
    o = _fused_case(K, B, C, D, dtype, easy, 4000 + B + C)
    ref, Dp = o["ref"], o["Dp"]
    valid = ref["valid"]
    assert o["loss"].shape == (B,) and o["dx"].shape == (B, D) and o["dw"].shape == (C, D)
    assert o["dx"].dtype == dtype and o["dw"].dtype == torch.float32
    tol = _loss_tol(S)
    el = (R.f64(o["loss"]) - ref["loss"]).abs()
    es = (R.f64(o["lse"])[:B] - ref["lse"]).abs()
    print("fused loss / lse err over tol", (el / tol).max().item(), (es / tol).max().item())
    assert (el <= tol).all() and (es <= tol).all(), (el, es)
    assert (R.f64(o["loss"])[~valid] == 0).all()
    # rank: both sides of the compare are fp32-accumulated dots of unit vectors times s
    band = 2.0 * S * Dp * 2.0 ** -24
    ties = R.near_ties(ref["x"], ref["t"], ref["onehot"], band)
    assert ((o["rank"].cpu().long() - ref["rank"]).abs() <= ties)[valid].all(), (o["rank"].cpu(), ref["rank"], ties)
    assert R.f64(o["dx"])[~valid].abs().max().item() == 0
    assert torch.isfinite(o["dx"]).all() and torch.isfinite(o["dw"]).all()
    ex, ew = R.relerr(o["dx"], ref["dx"]), R.relerr(o["dw"], ref["dw"])
    print(f"fused head B{B} C{C} D{D} {dtype} easy{int(easy)}: dX relerr {ex:.3e} dW relerr {ew:.3e}")
    if dtype == torch.bfloat16:
        # the bf16 store of dX, element by element: before its rounding the value is the fp32 path's,
        # whose error vector has a norm <= FUSED_DX_TOL |dX| -- so no single element is off by more
        elem = R.bf16_excess(o["dx"], ref["dx"], FUSED_DX_TOL * ref["dx"].norm().item())
        print("fused bf16 dX element rule excess", elem)
        assert elem <= 0, elem
    else:
        assert ex <= FUSED_DX_TOL, ex
    assert ew <= FUSED_DW_TOL, ew
