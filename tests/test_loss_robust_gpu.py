"""The GCE / SCE / ELR kernels (csrc/loss_robust.hip: xent_robust_fwd / xent_robust_bwd) against the fp64
evaluation of their formulas (tests/robust_ref.py).

Shapes: C crosses one lane group (3), the lane boundary (64, 65), an odd tail (1000), the
register-resident limit (2048) and the re-reading kernel (2049, 2173); ld = C (rows that are 16-byte
aligned only by chance: the scalar path) and ld = round_up(C, 8) + 8 (aligned rows, pad columns); B = 1, 5,
67 (a last workgroup with 1 and 3 of its 4 rows).  The random rows are standard normal: the row-relative
rule of the cross-entropy case needs 1 - p_a well above 2^-24 |lse| / 1e-5 (about 0.02), and at C = 3 rows
of twice that scale reach p_a = 0.995, where torch's own fp32 evaluation misses the rule.  Row 2 (row 0 at
B = 1) spreads its logits over 12 units, so its low classes fall below the elr clamp, and is labelled with its lowest class (on a class of
p -> 1 the gradient p_a - 1 cancels, and no fp32 evaluation meets a relative rule: test_loss_rows_gpu.py
labels its x40 row the same way); with B >= 5 rows 1 and 3 carry the labels -1 and C.
The elr indices are a reversed, shifted range into a table of B + 3 rows whose three unindexed rows
hold 0.25; two steps run, the second on the first one's table.

Bound: ``yard`` is the largest error that the same formula, evaluated by torch in fp32 on the CPU on
the test's own inputs, makes against fp64 over the tensor at hand (loss, gradient, table).  Every
element of the kernel's result may differ from fp64 by 4 yard: __expf / __logf and the reduction order
differ from torch's, and four is the margin the cross-entropy tests leave for them.  A bf16 gradient
adds one rounding of the value before it, 2^-8 (|ref| + 4 yard).  The cross-entropy case (sce, alpha 1,
beta 0) and every mode's lse are held to the rules of test_loss_rows_gpu.py as well.  rank, the
invalid rows, the pad columns and the unindexed table rows are exact.

Measured on an MI355X (profiles/r22/robust_loss.txt): the kernels compute in fp64 and round once, so the
worst fp32 element's error equals the yardstick (a quarter of the bound) in every case.  A first version
in fp32 arithmetic missed the bound in 29 of the 84 shape cases, by up to 5.3 x (gce q = 1 gradient,
1.42e-9 against a yardstick of 6.67e-11): over a small tensor torch's fp32 evaluation is often far inside
half an ulp of the result.
"""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import head_ref as R
from tests import robust_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GO = 0.37
PLANS = [("gce", 0.7), ("gce", 1.0), ("sce", 1.0, 0.0), ("sce", 0.5, 1.5)]
MODE = {"gce": 0, "sce": 1, "elr": 2}


def _inputs(B, C, ld, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ld, generator=gen)
    x[min(2, B - 1), :C] = (torch.rand(C, generator=gen) * 12.0 - 6.0)
    x[min(2, B - 1), [0, C - 1]] = torch.tensor([-6.0, 6.0])
    lab = torch.randint(0, C, (B,), generator=gen)
    lab[min(2, B - 1)] = 0  # the spread row's lowest class, as test_loss_rows_gpu.py labels its x40 row
    if B >= 5:
        lab[1], lab[3] = -1, C
    return x.to(dtype), lab, torch.arange(B).flip(0) + 2


def _close(got, ref, yard, tag, bf16=False):
    err = (R.f64(got) - ref).abs()
    tol = 4 * yard + (R.BF16_REL * (ref.abs() + 4 * yard) if bf16 else 0.0)
    print(tag, "kernel err", err.max().item(), "fp32 yardstick", float(yard), "worst err / bound", (err / tol).max().item())
    assert (err <= tol).all(), (tag, err.max().item(), float(yard))


def _step(K, xd, x, lab, C, plan, table_d, ref_table, yard_table, idx):
    """One forward + both backwards of ``plan`` against fp64; -> (reference, fp32 yardstick run)."""
    B, ld = x.shape
    g = R.f32(GO) * R.f32(1.0 / B)
    ref = RR.robust(x, lab, C, plan, g, table=ref_table, idx=idx)
    y32 = RR.robust(x, lab, C, plan, g, torch.float32, table=yard_table, idx=idx)
    elr = plan[0] == "elr"
    idx_d = idx.to(DEV) if elr else None
    a0, a1 = (plan + (0.0,))[1:3]
    loss, rank, rec = K.xent_robust_fwd(xd, lab.to(DEV), C, MODE[plan[0]], a0, a1, table_d, idx_d)
    valid = ref["valid"]
    assert torch.equal(rank.cpu().long()[valid], ref["rank"][valid]), plan
    assert (loss.cpu()[~valid] == 0).all()
    _close(loss, ref["loss"], (R.f64(y32["loss"]) - ref["loss"]).abs().max(), (plan, "loss"))
    absmax = R.f64(x)[:, :C].abs().amax(1).clamp_min(1.0)
    assert ((R.f64(rec[:, 0]) - ref["lse"]).abs() <= 2e-5 * absmax).all(), plan
    yard = (R.f64(y32["grad"]) - ref["grad"]).abs().max()
    for out_bf16 in (False, True):
        d = K.xent_robust_bwd(xd, lab.to(DEV), C, rec, MODE[plan[0]], a0, table_d, idx_d, torch.tensor([GO], device=DEV),
                              1.0 / B, out_bf16).cpu()
        assert d.shape == (B, ld) and d.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
        assert (d[:, C:] == 0).all() and (d[~valid] == 0).all(), plan
        _close(d[:, :C], ref["grad"], yard, (plan, "grad", "bf16" if out_bf16 else "fp32"), bf16=out_bf16)
        if plan == ("sce", 1.0, 0.0):  # plain cross-entropy: the rules of xent_fwd / xent_bwd
            assert ((R.f64(loss) - ref["loss"]).abs() <= 2e-5 * absmax).all()
            if out_bf16:
                assert R.bf16_excess(d[:, :C], ref["grad"], 1e-7 * abs(g)) <= 0
            else:
                assert R.row_relerr(d[:, :C], ref["grad"]).max().item() <= 1e-5
                assert R.f64(d).sum(1).abs().max().item() <= 1e-6 * abs(g)
    return ref, y32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("pad", [False, True], ids=["ldC", "ldpad"])
@pytest.mark.parametrize("C", [3, 64, 65, 1000, 2048, 2049, 2173])
def test_robust_kernels(C, pad, B, dtype):
    K = _ext.hip_ops()
    ld = (C + 7) // 8 * 8 + 8 if pad else C
    x, lab, idx = _inputs(B, C, ld, dtype, 1000 * B + C)
    xd = x.to(DEV)
    for plan in PLANS:
        _step(K, xd, x, lab, C, plan, None, None, None, idx)
    N = B + 3
    table = torch.zeros(N, C)
    table[[0, 1, N - 1]] = 0.25
    table_d, ref_table, yard_table = table.to(DEV), table, table
    for step in range(2):
        ref, y32 = _step(K, xd, x, lab, C, ("elr", 3.0, 0.7), table_d, ref_table, yard_table, idx)
        ref_table, yard_table = ref["table"], y32["table"]
        got = table_d.cpu()
        assert torch.equal(got[[0, 1, N - 1]], table[[0, 1, N - 1]])
        _close(got, ref_table, (R.f64(yard_table) - ref_table).abs().max(), ("elr table", step))
    assert ref_table[idx[ref["valid"]]].abs().min().item() > 0  # the second step read a non-zero table


def test_elr_step_replays_from_a_graph():
    """An elr step (forward, backward, table update) captured once and replayed twice is torch.equal to two
    eager steps: loss, rank, gradient and table."""
    B, C = 5, 65
    x, lab, idx = _inputs(B, C, C, torch.bfloat16, 11)
    lab_d, idx_d = lab.to(DEV), idx.to(DEV)

    def step(leaf, table):
        loss, rank = Fn.cross_entropy(leaf, lab_d, C, return_rank=True, robust=("elr", 3.0, 0.7, table, idx_d))
        (grad,) = torch.autograd.grad(loss * GO, leaf)
        return loss.detach(), rank, grad

    leaf_e, table_e = x.to(DEV).requires_grad_(True), torch.zeros(B + 3, C, device=DEV)
    eager = []
    for _ in range(2):
        eager.append([t.clone() for t in step(leaf_e, table_e)] + [table_e.clone()])
    leaf_g, table_g = x.to(DEV).requires_grad_(True), torch.zeros(B + 3, C, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(leaf_g, table_g)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    table_g.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(leaf_g, table_g)
    table_g.zero_()  # the capture ran nothing; be explicit
    for want in eager:
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(list(out) + [table_g], want):
            assert torch.equal(got, ref)
