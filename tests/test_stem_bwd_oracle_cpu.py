"""The fused-stem-backward oracle (tests/stem_bwd_oracle.py) against things the project did not write:
fp64 torch autograd through conv -> training BN -> ReLU -> max pool for the patch geometry and the
G1 / G2 / G3 identity, ``Fn.stem_s2d_weight`` and its autograd transpose for the weight index maps; and
the lattice builder's preconditions on small problems of every family."""
import pytest
import torch
import torch.nn.functional as F

from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import stem_bwd_oracle as S
from tests.pointwise_oracle import maxpool_first


def _autograd_problem(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x16 = torch.randn((N, H, W, 16), generator=g, dtype=torch.float64)
    w = (torch.randn((64, 4, 4, 16), generator=g, dtype=torch.float64) / 16).requires_grad_(True)
    gamma = (torch.rand(64, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(64, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    dy = torch.randn((N, H // 2, W // 2, 64), generator=g, dtype=torch.float64)
    return x16, w, gamma, beta, dy


@pytest.mark.parametrize("N,H,W", [(2, 6, 8), (1, 2, 4), (3, 4, 10)])
def test_oracle_matches_autograd(N, H, W):
    """conv 4x4 / 1 over x16 padded (2, 1, 2, 1) -> training BN -> ReLU -> max_pool2d(3, 2, 1), no pooling
    ties; the oracle runs without its bf16 roundings (the inputs are not bf16 numbers)"""
    eps = 1e-5
    x16, w, gamma, beta, dy = _autograd_problem(N, H, W, 1234 + W)
    xin = F.pad(x16.permute(0, 3, 1, 2), (2, 1, 2, 1))
    z = F.conv2d(xin, w.permute(0, 3, 1, 2))  # [N,64,H,W]
    mean = z.mean((0, 2, 3))
    var = z.var((0, 2, 3), unbiased=False)
    invstd = (var + eps).rsqrt()
    bn = (z - mean[None, :, None, None]) * (invstd * gamma)[None, :, None, None] + beta[None, :, None, None]
    y = F.max_pool2d(F.relu(bn), 3, 2, 1)
    (y * dy.permute(0, 3, 1, 2)).sum().backward()

    with torch.no_grad():
        scale = gamma * invstd
        shift = beta - mean * scale
        zh = z.permute(0, 2, 3, 1).contiguous()
        # the argmax of the BN output: monotone with its ReLU wherever the maximum is positive, and a
        # window without a positive value passes no gradient either way
        _, idx, tied = maxpool_first(zh * scale + shift, 3, 2, 1)
        assert tied == 0.0
        ref = S.reference(zh, x16, dy, idx, scale, shift, mean, invstd, 1, bf16=False)
        assert float((ref.g != 0).double().mean()) > 0.05 and float((zh * scale + shift <= 0).double().mean()) > 0.2
        count = float(N * H * W)
        dw, mag = S.dw_algebra(ref.G1, ref.G2, ref.G3, ref.s1, ref.s2raw, scale, invstd, count)
        text = S.dw_textbook(ref, x16, scale, invstd, count)
        assert bool(((dw - text).abs() <= 1e-12 * mag).all()), "algebraic and textbook dW differ"
        assert bool(((dw - w.grad).abs() <= 1e-11 * mag.clamp_min(1e-3)).all()), float((dw - w.grad).abs().max())
        torch.testing.assert_close(ref.sums[0], beta.grad, rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(ref.sums[1], gamma.grad, rtol=1e-11, atol=1e-11)


# "grow" leaves g' one image row: with the ReLU mask on top a channel may lose all of it, so it runs unmasked
@pytest.mark.parametrize("family,act", [(f, a) for f in S.FAMILIES for a in (0, 1) if (f, a) != ("grow", 1)])
def test_lattice_preconditions_and_forms(family, act):
    """a small problem of every family: the builder's own assertions, the ``tot`` layout, and the two
    forms of dW against each other in fp64"""
    N, H, W = 8, 4, 16
    pr = S.problem(N, H, W, act, family, (1, 2) if family in ("xrow", "grow") else None)
    ref = pr.ref
    assert pr.want_tot.shape == (S.TOT,) and pr.want_sums.shape == (2, 64)
    parts = S.split_tot(ref.tot)
    assert torch.equal(parts["G1"][0].reshape(64, 256), ref.G1) and torch.equal(parts["s2raw"][0], ref.s2raw)
    assert torch.equal(parts["G3"][0].reshape(256), ref.G3) and torch.equal(parts["G2"][0].reshape(64, 256), ref.G2)
    # G3 by hand for one column: k = (ty 1, tx 3, c 5) sums x16[n][y - 1][x + 1][5]
    assert ref.G3[1 * 64 + 3 * 16 + 5].item() == pr.x16[:, : H - 1, 1:, 5].double().sum().item()
    if family == "xrow":
        assert int((pr.x16 != 0).any(3).any(2).sum()) == 1
    if family in ("corner", "four", "bigfour"):
        assert not bool(ref.g[:, 0::2].any()) and not bool(ref.g[:, :, 0::2].any())
    if family in ("four", "bigfour"):  # only pixels (4 i + 1, 4 j + 1) receive, each from four windows
        assert not bool(ref.g[:, 3::4].any()) and not bool(ref.g[:, :, 3::4].any())
        want = pr.dy.double().reshape(N, H // 4, 2, W // 4, 2, 64).sum((2, 4))
        assert torch.equal(ref.raw[:, 1::4, 1::4], want)
    for count in (float(N * H * W), 64.0):
        dw, mag = S.dw_algebra(ref.G1, ref.G2, ref.G3, ref.s1, ref.s2raw, pr.scale, pr.invstd, count)
        text = S.dw_textbook(ref, pr.x16, pr.scale, pr.invstd, count)
        assert bool(((dw - text).abs() <= 1e-12 * mag).all())


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("Co", [1, 64, 65])
def test_s2d_weight_refs(C, Co):
    g = torch.Generator().manual_seed(100 * Co + C)
    w7 = torch.randn((Co, 7, 7, C), generator=g).requires_grad_(True)
    w16 = Fn.stem_s2d_weight(w7)
    assert torch.equal(S.s2d_weight_ref(w7.detach()), w16.detach())
    g16 = torch.randn((Co, 4, 4, 16), generator=g)
    w16.backward(g16)
    assert torch.equal(S.s2d_weight_bwd_ref(g16, C), w7.grad)
    # every 7x7 element has exactly one image; the other 256 - 49 C taps per filter are zero
    assert int((S.s2d_weight_ref(torch.ones(Co, 7, 7, C)) != 0).sum()) == Co * 49 * C


def test_launch_geometry():
    assert S.launch_geometry(1, 4, 256) == (4, 1)
    assert S.launch_geometry(257, 2, 256) == (256, 3)
    assert S.launch_geometry(205, 10, 256) == (256, 9)
    assert S.launch_geometry(129, 2, 256) == (256, 2)
