"""The supervised contrastive loss off the GPU: limits, the CPU path, the workload flag, and what the
inputs of test_supcon_gpu.py can detect.

With the fp64 reference alone (tests/supcon_ref.py, G rounded to bf16), four deliberate errors move dx
on the GPU test's inputs by (relative change; ``pad`` needs padding columns, so not B = 64):
  shape                  self in the denominator   padding as negatives   dS_ai dropped   mean over all rows
  (70, 37, 9, 0.1)       0.592                     0.121                  0.501           0.0713
  (64, 128, 5, 0.07)     0.771                     -                      0.505           0.0624
  (65, 512, 64, 0.07)    0.163                     0.0749                 0.502           0.384
  (130, 200, 40, 0.1)    0.174                     0.0498                 0.500           0.139
  (530, 128, 20, 0.1)    0.303                     0.0181                 0.500           0.051
each >= 1e-2, so a dx bound of 1e-3 separates the kernel from all four.
"""
import pytest
import torch

import main as entry
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import head_ref as R
from tests import supcon_ref as SR
from tests.supcon_ref import CASES, case_inputs


@pytest.mark.parametrize("case", range(1, len(CASES)))
def test_inputs_detect_the_deliberate_errors(case):
    (B, D, classes, tau), (x, y) = CASES[case], case_inputs(case)
    zn, inv = R.l2norm_rows(x, 1e-12)
    zn = zn.float().bfloat16()
    ref = SR.supcon(zn, inv, y, D, tau)["dx"]
    moved = {f: R.relerr(SR.supcon(zn, inv, y, D, tau, fault=f)["dx"], ref) for f in SR.FAULTS if f != "pad" or B % 64}
    print(f"supcon {CASES[case]}: " + " ".join(f"{f} {v:.3g}" for f, v in moved.items()))
    assert all(v >= 1e-2 for v in moved.values()), moved


@pytest.mark.parametrize("case", [0, 1, 4])
def test_cpu_path_is_the_reference(case):
    (B, D, classes, tau), (x, y) = CASES[case], case_inputs(case)
    xt = x.float().requires_grad_(True)
    loss = Fn.supcon_loss(xt, y, tau)
    (2.0 * loss).backward()
    zn, inv = R.l2norm_rows(xt, 1e-12)
    ref = SR.supcon(zn, inv, y, D, tau, g=2.0, round_g=False)
    assert abs(loss.item() - ref["loss"].item()) <= 1e-5 * max(1.0, abs(ref["loss"].item()))
    assert R.relerr(xt.grad, ref["dx"]) <= 1e-5 and xt.grad[~ref["valid"]].abs().max().item() == 0


def test_limits():
    x, y = torch.randn(6, 16), torch.arange(6) % 2
    for bad in (dict(x=torch.randn(6, 16, 1)), dict(x=torch.randn(16, 6).t()), dict(x=x.half()),
                dict(x=torch.randn(1, 16), y=y[:1]), dict(x=torch.randn(6, 513)), dict(y=y.int()), dict(y=y[:5]),
                dict(temperature=0.0), dict(splits=0), dict(splits=65)):
        kw = {"x": x, "y": y, "temperature": 0.07, "splits": None, **bad}
        with pytest.raises(ValueError, match="supcon_loss covers"):
            Fn.supcon_loss(kw["x"], kw["y"], kw["temperature"], kw["splits"])


BASE = ("--model resnet18 --data synthetic --dataset CIFAR10 --image-size 32 --batchsize 8 --synthetic-train-size 16 "
        "--synthetic-val-size 8 --workers 0 --log-interval 100 --device cpu --epochs 1").split()


def test_workload_flag(tmp_path):
    entry.main(["--workload", "arcface", "--arc-supcon-weight", "0.5", "--out-dir", str(tmp_path)] + BASE)
    assert (tmp_path / "last.pth").exists()
    with pytest.raises(ValueError, match="--arc-supcon-weight"):
        entry.main(["--workload", "baseline", "--arc-supcon-weight", "0.5", "--out-dir", str(tmp_path)] + BASE)
