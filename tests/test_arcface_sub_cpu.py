"""Sub-center ArcFace off the GPU: the CPU reference path against fp64 autograd, the module's limits,
and the ARCFACE workload with --arc-sub-centers end to end (checkpoint, resume, weight EMA)."""
import math

import pytest
import torch

import main as entry
from ddp_classification_pytorch_amd.models.heads import ArcMarginProduct
from ddp_classification_pytorch_amd.ops import functional as Fn


@pytest.mark.parametrize("easy", [True, False])
def test_cpu_path_matches_fp64_autograd(easy):
    torch.manual_seed(1)
    B, C, K, D, s, m = 12, 9, 3, 20, 30.0, 0.5
    x, W, lab = torch.randn(B, D), torch.randn(C, K, D), torch.randint(0, C, (B,))
    W[2, 2] = W[2, 0] * 2  # an exact tie (same normalised bits): the first centre takes the gradient
    lab[0] = 2
    x[0] = W[2, 0] + 0.3 * torch.randn(D)
    xd, Wd = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    loss, rank, _, sub = Fn.arcface_loss(xd, Wd, lab, s, m, easy, return_sub_idx=True)
    loss.backward()
    x6, W6 = x.double().requires_grad_(True), W.double().requires_grad_(True)
    cos = (torch.nn.functional.normalize(x6) @ torch.nn.functional.normalize(W6.view(C * K, D)).t()).view(B, C, K)
    cbar, arg = cos.max(2)
    phi = cbar * math.cos(m) - torch.sqrt(1 - cbar ** 2) * math.sin(m)
    phi = torch.where(cbar > 0, phi, cbar) if easy else torch.where(cbar > math.cos(math.pi - m), phi,
                                                                    cbar - math.sin(math.pi - m) * m)
    oh = torch.nn.functional.one_hot(lab, C).double()
    logits = s * (oh * phi + (1 - oh) * cbar)
    ref = torch.nn.functional.cross_entropy(logits, lab)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert sub[0].item() == 0 and Wd.grad[2, 2].abs().max().item() == 0 and Wd.grad[2, 0].abs().max().item() > 0
    notie = torch.ones(C, dtype=torch.bool)
    notie[2] = False  # (torch's max may pick either of two equal centres)
    assert torch.equal(sub.long()[lab != 2], arg[torch.arange(B), lab][lab != 2])
    assert torch.allclose(xd.grad.double(), x6.grad, rtol=1e-4, atol=1e-6)
    assert torch.allclose(Wd.grad.double()[notie], W6.grad[notie], rtol=1e-4, atol=1e-6)
    assert torch.equal(rank.long(), (logits > logits.gather(1, lab[:, None])).sum(1))


def test_module_shapes_and_limits():
    head = ArcMarginProduct(32, 10, sub_centers=3)
    assert head.weight.shape == (10, 3, 32) and "last_sub_idx" not in head.state_dict()
    bound = math.sqrt(6.0 / (32 + 30))  # xavier-uniform over the [C K, D] matrix
    assert bound * 0.9 < head.weight.abs().max().item() <= bound
    x, lab = torch.randn(6, 32), torch.randint(0, 10, (6,))
    head(x, lab)[0].backward()
    assert head.last_sub_idx.shape == (6,) and head.weight.grad.shape == (10, 3, 32)
    assert head.margin_logits(x, lab).shape == (6, 10)
    for bad in (dict(sub_centers=5), dict(sub_centers=0), dict(sub_centers=2, in_features=300)):
        with pytest.raises(ValueError, match="Sub-center"):
            ArcMarginProduct(**{"in_features": 32, "out_features": 10, **bad})


def test_workload_checkpoint_resume_and_ema(tmp_path):
    base = ["--workload", "arcface", "--arc-sub-centers", "3", "--model", "resnet18", "--data", "synthetic",
            "--dataset", "CIFAR10", "--image-size", "32", "--batchsize", "8", "--synthetic-train-size", "16",
            "--synthetic-val-size", "8", "--workers", "0", "--log-interval", "100", "--device", "cpu", "--model-ema",
            "--out-dir", str(tmp_path)]
    entry.main(base + ["--epochs", "1"])
    ck = torch.load(tmp_path / "last.pth", weights_only=True)
    w = ck["models"]["model"]["arc.weight"]
    assert w.dim() == 3 and w.shape[1] == 3 and w.dtype == torch.float32
    assert ck["ema"]["averages"]["model.arc.weight"].shape == w.shape
    entry.main(base + ["--epochs", "2", "--resume", str(tmp_path / "last.pth")])
    assert "resumed from" in open(tmp_path / "output.txt").read()
