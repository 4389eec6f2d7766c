"""bn3's sum of g xhat from conv3's weight-gradient GEMM instead of a pass over bn3's input.

Three layers, smallest shapes at which each can still go wrong:

* the dgrad epilogue without the xhat sum (``conv_dgrad_bn`` with no BN input) against the same call
  with it: the stored gradient and the S1 sums must be ``torch.equal``, row 1 of the sums is zeros.
  98 rows (N = 2, 7 x 7: one partial 128-row tile), BN widths 64 / 128 / 256 (one 64-channel tile, one
  128-channel tile, several tiles), K = 64 / 128 (one k-tile; two, which is what split-K needs), no add
  source / a full-size one / the compact stride-2 subgrid, under every 128-row configuration the
  autotuner can pick (tile width, k depth, ring depth) and the split-K pair of launches.
* ``bn_lin_s2`` against fp64 at the shapes of ``test_conv1x1_bn_lin_bwd_matches_fp64``, also with conv3's
  input at a mean of 32 standard deviations.  Bound, from the number formats alone:
  S2[c] = invstd[c] sum_k W3[c][k] (G[c][k] - S1[c] colmean[k]); G[c][k] and colsum[k] are fp32 sums of n
  exact bf16 products / values, the k-sum has m terms, so the error is at most (n + m) 2^-24 times the sum
  of the MAGNITUDES of the terms, invstd sum_k |W3| (sum_rows |g| |a2| + |S1| |colmean|) (norm over c).
  That worst case is far above what the kernel does (measured 1e-7 .. 1e-5 of it) -- and, unlike the
  issue that asked for this test supposed, it is not exceeded by the UNCENTRED form sum_k W3 G - mean S1
  either: tests/test_bn3_s2_cpu.py measures both forms in fp32 (32 sigma, (2,14,14,256,1024): bound
  1.7e+02 on |S2| = 6.5e+02, centred 1.5e-03, uncentred 3.1e-03, uncentred with the BN's own mean of the
  bf16-rounded conv output 1.5e+00).  The centred form is kept because it is the more accurate one by
  these figures, not because the other fails this bound.
* two identity bottlenecks in a row (tests/test_bn3_linear_gpu.py's set-up: m = 64, N = 4, 14 x 14, plain
  and with conv3's input at 32 sigma): forward outputs and the gradient handed to block 0 bitwise equal to
  ``set_bn3_linear(False)``, ``bn3.weight.grad`` bitwise DIFFERENT (the sum took the other route), every
  gradient of block 0 within max(F_BF16 x yardstick, FLOOR) of the fp64 mirror (tests/test_block_grads.py),
  once under ``torch.cuda.graph`` bitwise against eager, and the fallback: the path switched off between
  forward and backward, when the epilogue has already skipped the sum.
"""
import copy

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import model_mirror as M
from tests.test_block_grads import F_BF16, FLOOR
from tests.test_bn3_linear_gpu import PIPELINE, ROW128, _mirror, _name, _step, _two_blocks, slots

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def K():
    return _ext.hip_ops()


# ----------------------------------------------------------------------------- the epilogue variant
# split-K runs on 64-channel tiles with at most 3 stages; tg_split_k = 3 asks for three slices and gets
# the two that K = 128 has (K = 64 does not split: those configurations then repeat the unsplit ones)
SPLIT = [(("tg_split_k", 3),)] + [(("tg_split_k", 3), ("tg_tile_n", 64)) + c for c in PIPELINE
                                  if ("tg_stages", 4) not in c]
EPI_CFGS = ROW128 + SPLIT


@pytest.mark.parametrize("add", ["none", "full", "compact"])
@pytest.mark.parametrize("Kc", [64, 128])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_dgrad_epilogue_without_xhat_sum_bitwise(K, C, Kc, add):
    N, H, W = 2, 7, 7
    gen = torch.Generator().manual_seed(C * 1000 + Kc)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    dy = rnd(N, H, W, Kc).to(BF16).to(DEV)
    wt = (rnd(C, 1, 1, Kc) / Kc ** 0.5).to(BF16).to(DEV)
    y = (3.0 + rnd(N, H, W, C)).to(BF16).to(DEV)
    mask = torch.randint(0, 256, (N, H, W, C // 8), generator=gen, dtype=torch.uint8).to(DEV)
    scale, shift, mean = (rnd(C).to(DEV) for _ in range(3))
    invstd = (rnd(C).abs() + 0.5).to(DEV)
    a = None
    if add == "full":
        a = rnd(N, H, W, C).to(BF16).to(DEV)
    elif add == "compact":
        a = rnd(N, (H + 1) // 2, (W + 1) // 2, C).to(BF16).to(DEV)
    for cfg in EPI_CFGS:
        with slots(K, cfg):
            dx_y, sums_y = K.conv_dgrad_bn(dy, wt, 0, a, y, None, scale, shift, mean, invstd, 1, mask, 0.0)
            dx_n, sums_n = K.conv_dgrad_bn(dy, wt, 0, a, None, None, scale, shift, mean, invstd, 1, mask, 0.0)
        tag = f"C={C} K={Kc} add={add} {_name(cfg)}"
        assert torch.equal(dx_n, dx_y), f"masked gradient differs: {tag}"
        assert torch.equal(sums_n[0], sums_y[0]), f"S1 differs: {tag}"
        assert not bool(sums_n[1].any()), f"the S2 row is not zeros: {tag}"
        assert bool(sums_y[1].any()), f"the reference call formed no S2: {tag}"


def test_dgrad_without_bn_input_needs_relu_mask_bits(K):
    dy = torch.zeros(2, 7, 7, 64, dtype=BF16, device=DEV)
    wt = torch.zeros(64, 1, 1, 64, dtype=BF16, device=DEV)
    v = torch.ones(64, device=DEV)
    mask = torch.zeros(2, 7, 7, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="mask bits"):
        K.conv_dgrad_bn(dy, wt, 0, None, None, None, v, v, v, v, 1, None, 0.0)
    with pytest.raises(RuntimeError, match="mask bits"):
        K.conv_dgrad_bn(dy, wt, 0, None, None, None, v, v, v, v, 0, mask, 0.0)


# ----------------------------------------------------------------------------- S2 against fp64
@pytest.mark.parametrize("big_mean", [False, True], ids=["plain", "mean32sigma"])
@pytest.mark.parametrize("shape", [(2, 14, 14, 256, 1024), (2, 7, 7, 512, 2048), (3, 5, 5, 192, 768)], ids=str)
def test_bn_lin_s2_matches_fp64(K, shape, big_mean):
    """sum g xhat against invstd sum g (a2 W3^T - mean) in fp64 from the same bf16 operands; the bound is
    derived in the module docstring.  Also: row 0 of the sums is left alone, the returned G and colsum are
    the weight-gradient GEMM's and the column sums, and ``conv1x1_bn_lin_bwd`` given them returns exactly
    what it returns when it computes them itself."""
    N, H, W, m, C = shape
    n = N * H * W
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    if big_mean:  # relu(0.25 xhat + 8): mean 8, standard deviation 0.25 (the block test's bn2 setting)
        a2 = torch.relu(0.25 * rnd(n, m) + 8.0).to(BF16)
    else:
        a2 = (torch.relu(rnd(n, m)) + 0.5 * rnd(1, m).abs()).to(BF16)
    w3 = (rnd(C, m) / m ** 0.5).to(BF16)
    g = rnd(n, C).to(BF16)
    a64, w64, g64 = a2.double(), w3.double(), g.double()
    x3 = a64 @ w64.t()
    mean, istd = x3.mean(0), (x3.var(0, unbiased=False) + 1e-5).rsqrt()
    S1, want = g64.sum(0), (g64 * (x3 - mean)).sum(0) * istd
    cm = a64.mean(0)
    mag = istd * (w64.abs() * (g64.abs().t() @ a64.abs() + torch.outer(S1.abs(), cm.abs()))).sum(1)
    bound = (n + m) * 2.0 ** -24 * mag.norm().item()
    f32 = lambda t: t.float().to(DEV)
    gd, ad = g.reshape(N, H, W, C).to(DEV), a2.reshape(N, H, W, m).to(DEV)
    w3d, wtd = w3.reshape(C, 1, 1, m).to(DEV), w3.t().contiguous().reshape(m, 1, 1, C).to(DEV)
    sums = torch.stack([f32(S1), torch.zeros(C, device=DEV)]).contiguous()
    G, cs = K.bn_lin_s2(gd, ad, w3d, f32(istd), sums, float(n))
    torch.cuda.synchronize()
    err = (sums[1].double().cpu() - want).norm().item()
    print(f"{shape} {'32 sigma' if big_mean else 'plain'}: S2 err {err:.3e} bound {bound:.3e} "
          f"(|S2| {want.norm().item():.3e}, median |mean| / sigma of x3 {(mean.abs() * istd).median().item():.1f})")
    assert err <= bound
    assert torch.equal(sums[0], f32(S1)), "row 0 (S1) was written"
    assert torch.equal(G, K.conv_wgrad(gd, ad, 1, 1, 1, 0))
    cs_err = (cs.double().cpu() - a64.sum(0)).abs().max().item()
    assert cs_err <= n * 2.0 ** -24 * a64.abs().sum(0).max().item()
    # the payload route of conv3's backward: G and colsum handed over, not recomputed
    gamma = f32(rnd(C).abs() + 0.5)
    scale = gamma * f32(istd)
    dx0, dw0 = K.conv1x1_bn_lin_bwd(gd, ad, w3d, wtd, scale, f32(istd), sums, float(n), True, True)
    dx1, dw1 = K.conv1x1_bn_lin_bwd(gd, ad, w3d, wtd, scale, f32(istd), sums, float(n), True, True, G, cs)
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw1)


# ----------------------------------------------------------------------------- block level
def _check_against_mirror(blk64, x, dy0, paths, tag):
    ref = _mirror(blk64, x, dy0, None)
    yard = _mirror(blk64, x, dy0, torch.bfloat16)
    bad = []
    for path, grads in paths:
        for q, r in ref.items():
            ours = grads[q]
            ours = ours.double().cpu().permute(0, 3, 1, 2) * (M._nchw64(x) > 0) if q == "dx" else ours.double().cpu()
            err, y = M.rel_l2(ours, r), M.rel_l2(yard[q], r)
            print(f"{tag} {path} {q}: err {err:.3e} yardstick {y:.3e}")
            if not err <= max(F_BF16 * y, FLOOR):
                bad.append((path, q, err, y))
    assert not bad, bad


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(4, 14, 14, 256, generator=g)).to(BF16).to(DEV)
    dy = torch.randn(4, 14, 14, 256, generator=g).to(BF16).to(DEV)
    return x, dy


@pytest.mark.parametrize("big_mean", [False, True], ids=["plain", "mean32sigma"])
def test_identity_block_s2_from_gemm(K, big_mean):
    net = _two_blocks(big_mean)
    blk64 = copy.deepcopy(net[0]).double()
    net = net.to(DEV)
    x, dy = _inputs(1)
    out_new, mid_new, g_new, dy0_new = _step(net, x, dy, True)
    out_old, mid_old, g_old, dy0_old = _step(net, x, dy, False)
    assert torch.equal(out_new, out_old) and torch.equal(mid_new, mid_old), "forward outputs differ"
    assert torch.equal(dy0_new, dy0_old), "the gradient handed to the block under test differs"
    # S1 comes from the same epilogue reduction either way, S2 from another sum: the path really ran
    assert torch.equal(g_new["bn3.bias"], g_old["bn3.bias"]), "bn3's sum of g changed"
    assert not torch.equal(g_new["bn3.weight"], g_old["bn3.weight"]), "the S2-from-GEMM path was not taken"
    _check_against_mirror(blk64, x, dy0_new, (("s2-from-gemm", g_new), ("elementwise", g_old)),
                          "mean32" if big_mean else "plain")


@pytest.mark.parametrize("big_mean", [False, True], ids=["plain", "mean32sigma"])
def test_identity_block_fallback_after_skipped_sum(K, big_mean):
    """Forward with the path on (the epilogue is told to skip the sum), switched off before backward: bn3
    must form both sums itself, never read the skipped row."""
    net = _two_blocks(big_mean)
    blk64 = copy.deepcopy(net[0]).double()
    net = net.to(DEV)
    x, dy = _inputs(1)
    cap = {}
    prev = Fn._BN3_LINEAR[0]
    Fn.set_bn3_linear(True)
    try:
        xin = x.clone().requires_grad_(True)
        mid = net[0](xin)
        mid.register_hook(lambda g: cap.__setitem__("dy0", g.detach().clone()))
        out = net[1](mid)
        Fn.set_bn3_linear(False)
        out.backward(dy)
        torch.cuda.synchronize()
    finally:
        Fn.set_bn3_linear(prev)
    grads = {n: p.grad.detach().clone() for n, p in net[0].named_parameters()}
    grads["dx"] = xin.grad.detach().clone()
    assert bool(grads["bn3.weight"].any())
    _check_against_mirror(blk64, x, cap["dy0"], (("fallback", grads),), "mean32" if big_mean else "plain")


def test_identity_block_s2_graph_matches_eager(K):
    net = _two_blocks(False).to(DEV)
    x, dy = _inputs(2)

    def run():
        for p in net.parameters():
            p.grad = None
        xin = x.clone().requires_grad_(True)
        net(xin).backward(dy)
        return [xin.grad] + [p.grad for p in net.parameters()]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = run()
    graph.replay()
    torch.cuda.synchronize()
    names = ["dx"] + [n for n, _ in net.named_parameters()]
    for n, a, b in zip(names, eager, held):
        assert torch.equal(a, b), n
