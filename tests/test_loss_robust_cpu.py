"""Fn.cross_entropy(robust=...) on the CPU (the reference math of ops/_ref.py) against the fp64 autograd
evaluation of the formulas (tests/robust_ref.py), the refusals of the keyword and of the --loss flag."""
import pytest
import torch

from ddp_classification_pytorch_amd.config import parse_args
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import robust_ref as RR

B, C, LD, N = 6, 11, 16, 9
GO = 0.37


def _inputs():
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, LD, generator=gen) * 2.0
    x[2, :C] = torch.linspace(-6.0, 6.0, C)  # the low classes fall below the elr clamp
    lab = torch.randint(0, C, (B,), generator=gen)
    lab[1], lab[3] = -1, C
    idx = torch.arange(B).flip(0) + 2
    return x, lab, idx


@pytest.mark.parametrize("plan", [("gce", 0.7), ("gce", 1.0), ("sce", 1.0, 0.0), ("sce", 0.5, 1.5), ("elr", 3.0, 0.7)],
                         ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_ref_path_is_the_formula(plan, reduction):
    x, lab, idx = _inputs()
    scale = 1.0 / B if reduction == "mean" else 1.0
    table = ref_table = torch.zeros(N, C)
    for _ in range(2):  # the second elr step reads a non-zero table
        ref = RR.robust(x, lab, C, plan, GO * scale, table=ref_table, idx=idx)
        leaf = x.clone().requires_grad_(True)
        robust = plan + (table, idx) if plan[0] == "elr" else plan
        loss, rank = Fn.cross_entropy(leaf, lab, C, reduction=reduction, return_rank=True, robust=robust)
        (loss * GO).backward()
        assert abs(loss.item() - ref["loss"].sum().item() * scale) <= 1e-5 * B
        assert torch.equal(rank.long()[ref["valid"]], ref["rank"][ref["valid"]])
        assert (leaf.grad[:, :C].double() - ref["grad"]).abs().max().item() <= 1e-6
        assert leaf.grad[:, C:].abs().max().item() == 0 and leaf.grad[~ref["valid"]].abs().max().item() == 0
        if plan[0] == "elr":
            ref_table = ref["table"]
            assert (table.double() - ref_table).abs().max().item() <= 1e-6
            assert torch.equal(table[[0, 1, N - 1]], torch.zeros(3, C))  # rows no index names


def test_robust_none_is_the_plain_call():
    x, lab, _ = _inputs()
    lab[1], lab[3] = 0, C - 1
    for kw in (dict(), dict(smoothing=0.1)):
        a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        la, ra = Fn.cross_entropy(a, lab, C, return_rank=True, **kw)
        lb, rb = Fn.cross_entropy(b, lab, C, return_rank=True, robust=None, **kw)
        la.backward(), lb.backward()
        assert torch.equal(la, lb) and torch.equal(ra, rb) and torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("kw", [dict(robust=("gce", 0.7), smoothing=0.1),
                                dict(robust=("sce", 1.0, 1.0), mix=(torch.zeros(B, dtype=torch.int32), torch.ones(B))),
                                dict(robust=("elr", 3.0, 0.7))], ids=["smoothing", "mix", "malformed"])
def test_keyword_refusals(kw):
    x, lab, _ = _inputs()
    with pytest.raises(ValueError, match="cross_entropy robust covers"):
        Fn.cross_entropy(x, lab.clamp(0, C - 1), C, **kw)


@pytest.mark.parametrize("argv,match", [
    (["--workload", "cdr", "--loss", "gce"], "baseline only"),
    (["--workload", "arcface", "--loss", "elr"], "baseline only"),
    (["--loss", "sce", "--mixup-alpha", "0.2"], "one hard label"),
    (["--loss", "gce", "--label-smoothing", "0.1"], "one hard label"),
    (["--loss", "gce", "--gce-q", "1.5"], "--gce-q covers"),
    (["--loss", "elr", "--world-size", "2"], "one process"),
])
def test_loss_flag_refusals(argv, match):
    with pytest.raises(ValueError, match=match):
        parse_args(argv + ["--device", "cpu"])


def test_loss_flag_defaults():
    a = parse_args(["--device", "cpu"])
    assert (a.loss, a.gce_q, a.sce_alpha, a.sce_beta, a.elr_lambda, a.elr_beta) == ("ce", 0.7, 1.0, 1.0, 3.0, 0.7)
    assert parse_args(["--loss", "sce", "--world-size", "2", "--device", "cpu"]).loss == "sce"
