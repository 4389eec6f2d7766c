"""bn3's sum of g xhat from conv3's weight-gradient GEMM (csrc/bn_lin.hip, bn_lin_s2_kernel), in the fp32
reference math of ops/_ref.py on the CPU, at conv3 inputs with a mean of 32 standard deviations.

    S2[c] = invstd[c] sum_k W3[c][k] (G[c][k] - S1[c] colmean[k]),   G = g^T a2 (fp32, conv_wgrad)

against invstd sum g (a2 W3^T - mean) in fp64 from the same bf16 operands, with the bound of
tests/test_bn3_s2_gpu.py: (n + m) 2^-24 times the sum of the magnitudes of the terms.

The centred form (the difference taken per k, before the sum) is compared with two uncentred ones,
sum_k W3 G - mean S1 with mean = W3 colmean(a2) in fp32, and with the mean a BN layer holds (the statistics
of the bf16-rounded conv output).  The issue behind this change expected the uncentred form to exceed the
bound at 32 sigma.  It does not: the bound is a worst case over n + m roundings of terms that carry the
mean themselves, and the uncentred forms make a handful of roundings at that magnitude.  Measured at
(2,14,14,256,1024): bound 1.7e+02 on |S2| = 6.5e+02; centred 1.5e-03, uncentred 3.1e-03, uncentred with the
BN's mean 1.5e+00.  What the figures do show, and what is asserted: the centred form is within the bound,
it is the most accurate of the three, and the BN's own mean costs three orders of magnitude (its rounding
error, times S1, stays whole) -- the reason the kernel takes colmean(a2) and not the saved mean.
"""
import pytest
import torch

from ddp_classification_pytorch_amd.ops import _ref

BF16 = torch.bfloat16


@pytest.mark.parametrize("add", ["none", "full", "compact"])
def test_reference_dgrad_without_bn_input(add):
    """ops/_ref.py's ``conv_dgrad_bn`` without the BN input: the gradient and S1 of the call with it,
    row 1 of the sums zeros (the contract of the HIP epilogue variant)."""
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    N, H, W, C, Kc = 2, 7, 7, 16, 8
    dy, wt = rnd(N, H, W, Kc).to(BF16), rnd(C, 1, 1, Kc).to(BF16)
    y = rnd(N, H, W, C).to(BF16)
    mask = torch.randint(0, 256, (N, H, W, C // 8), generator=gen, dtype=torch.uint8)
    v = [rnd(C) for _ in range(4)]
    a = {"none": None, "full": rnd(N, H, W, C).to(BF16), "compact": rnd(N, 4, 4, C).to(BF16)}[add]
    dx_y, sums_y = _ref.conv_dgrad_bn(dy, wt, 0, a, y, None, *v, 1, mask)
    dx_n, sums_n = _ref.conv_dgrad_bn(dy, wt, 0, a, None, None, *v, 1, mask)
    assert torch.equal(dx_n, dx_y) and torch.equal(sums_n[0], sums_y[0])
    assert not bool(sums_n[1].any()) and bool(sums_y[1].any())


@pytest.mark.parametrize("shape", [(2, 14, 14, 256, 1024), (3, 5, 5, 192, 768)], ids=str)
def test_centred_s2_in_fp32_at_32_sigma(shape):
    N, H, W, m, C = shape
    n = N * H * W
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    a2 = torch.relu(0.25 * rnd(n, m) + 8.0).to(BF16)
    w3 = (rnd(C, m) / m ** 0.5).to(BF16)
    g = rnd(n, C).to(BF16)
    a64, w64, g64 = a2.double(), w3.double(), g.double()
    x3 = a64 @ w64.t()
    mean, istd = x3.mean(0), (x3.var(0, unbiased=False) + 1e-5).rsqrt()
    assert (mean.abs() * istd).median().item() > 10.0  # conv3's output: means of tens of sigma
    S1, want = g64.sum(0), (g64 * (x3 - mean)).sum(0) * istd
    mag = istd * (w64.abs() * (g64.abs().t() @ a64.abs() + torch.outer(S1.abs(), a64.mean(0).abs()))).sum(1)
    bound = (n + m) * 2.0 ** -24 * mag.norm().item()
    # fp32, as the kernels compute
    G = _ref.conv_wgrad(g.reshape(N, H, W, C), a2.reshape(N, H, W, m), 1, 1, 1, 0).reshape(C, m).float()
    cm, S1f, istdf, wf = a2.float().sum(0) / n, S1.float(), istd.float(), w3.float()
    centred = istdf * (wf * (G - torch.outer(S1f, cm))).sum(1)
    uncentred = istdf * ((wf * G).sum(1) - (wf @ cm) * S1f)
    x3b, _ = _ref.conv_fwd(a2.reshape(N, H, W, m), w3.reshape(C, 1, 1, m), 1, 0, False)  # bf16, as stored
    bn_mean = x3b.float().reshape(n, C).mean(0)
    uncentred_bn = istdf * ((wf * G).sum(1) - bn_mean * S1f)
    e = {k: (v.double() - want).norm().item()
         for k, v in (("centred", centred), ("uncentred", uncentred), ("uncentred_bn_mean", uncentred_bn))}
    print(f"{shape}: bound {bound:.3e} |S2| {want.norm().item():.3e} " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["centred"] <= bound
    assert e["centred"] < e["uncentred"] < e["uncentred_bn_mean"]
    assert e["uncentred_bn_mean"] > 100 * e["centred"]
