"""The linear bn3 backward on the GPU: the K-concatenated two-source tap GEMM bit-exact on integer
lattices under every kernel that gained the second source, and one identity bottleneck's gradients
through the new path against the fp64 block mirror.

Two-source GEMM (``conv1x1_cat``): out = x w1^T + x2 w2^T + bias with integer-valued bf16 operands and
an integer fp32 bias -- every partial sum is an integer fp32 holds (tests/exact_oracle.py), so the
only correct output is the exact sum rounded once, whatever the tile, k depth, ring depth, schedule,
persistent loop or stream-K cut; the comparison is ``torch.equal``.  Shapes: the smallest at which
each kernel can still go wrong --
  * 98 rows x 64 channels out: a partial 128-row tile, 64-channel tiles;
  * 392 rows x 256: a partial 256-row big tile (256 x 256 and 256 x 128, every schedule, 5-slot ring,
    persistent loop, stream-K on the 256 x 128 tile's four tiles);
  * 588 rows x 256: three 256 x 256 tiles, the fewest stream-K cuts between workgroups need there;
  * 98 rows x 128 with 64-deep and 32-deep k-tiles: the source switch on a k-tile boundary of both.

Block level: two identity bottlenecks in a row (the second one's conv1 dgrad epilogue is what hands the
first one's bn3 its masked gradient and sums), m = 64, N = 4, 14 x 14.  Forward outputs of the new path
and of ``set_bn3_linear(False)`` must be bitwise equal; every gradient of the first block under both
paths is held to the project's rule against the fp64 mirror of that block on the captured tensors,
err <= max(F_BF16 x yardstick, 1e-2) (tests/test_block_grads.py).  Repeated with bn2's affine set so
that conv3's input has a mean of 32 standard deviations (conv3's output means are then tens of its
standard deviations): the case an uncentred constant term fails.  Once under ``torch.cuda.graph``,
bitwise against eager.
"""
import copy

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.models import resnet as R
from ddp_classification_pytorch_amd.ops import functional as Fn
from ddp_classification_pytorch_amd.tuning import slot as tslot
from tests import exact_oracle as X
from tests import model_mirror as M
from tests.test_block_grads import F_BF16, FLOOR

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = X.BF16


@pytest.fixture(scope="module")
def K():
    return _ext.hip_ops()


class slots:
    """set the tuning slots of ``cfg`` = ((name, value), ...), run to completion, restore every one"""

    def __init__(self, K, cfg):
        self.K, self.cfg = K, cfg

    def __enter__(self):
        for name, v in self.cfg:
            self.K.set_tuning(tslot(name), v)

    def __exit__(self, *exc):
        try:
            torch.cuda.synchronize()
        finally:
            for name, _ in self.cfg:
                self.K.set_tuning(tslot(name), 0)
        return False


def _name(cfg):
    return ",".join(f"{k}={v}" for k, v in cfg) or "default"


def _cat_problem(shape):
    N, H, W, C1, C2, Co = shape
    mx, mw = X.pick_ranges(C1 + C2)
    x = X.lattice((N, H, W, C1), -mx, mx, X._seed("cx", shape))
    x2 = X.lattice((N, H, W, C2), -mx, mx, X._seed("cx2", shape))
    w = X.lattice((Co, C1 + C2), -mw, mw, X._seed("cw", shape))
    bias = X.int_vector(Co, -200, 200, X._seed("cb", shape))
    e1 = x.double().reshape(-1, C1) @ w[:, :C1].double().t()
    e2 = x2.double().reshape(-1, C2) @ w[:, C1:].double().t()
    exact1 = e1.reshape(N, H, W, Co)
    exact2 = (e1 + e2).reshape(N, H, W, Co)
    exactb = (e1 + e2 + bias.double()).reshape(N, H, W, Co)
    X.check_lattice(x, w[:, :C1], C1, exact1, BF16)
    X.check_lattice(torch.cat([x, x2], -1), w, C1 + C2, exact2, BF16)
    X.check_lattice(torch.cat([x, x2], -1), w, C1 + C2, exactb, BF16, bias=bias)
    return x, x2, w, bias, exact1, exact2, exactb


PIPELINE = [(("tg_stages", 2), ("tg_kdepth", 64)), (("tg_stages", 3),), (("tg_stages", 4),),
            (("tg_stages", 2), ("tg_kdepth", 32)), (("tg_stages", 3), ("tg_kdepth", 32)),
            (("tg_stages", 4), ("tg_kdepth", 32))]
ROW128 = [()] + PIPELINE + [c + (("tg_tile_n", 64),) for c in PIPELINE] + [(("tg_tile_n", 128),)]


def _big(modes, sks):
    out = []
    for mode in modes:
        for cvar in (0, 1, 2, 3):
            for stages, persist in ((0, 0), (5, 0), (0, 1)):
                if stages and mode != 1:
                    continue  # the 5-slot ring is the 256 x 256 tile's
                out.append((("tg_big", mode), ("tg_big_cvar", cvar), ("tg_big_stages", stages),
                            ("tg_big_persist", persist)))
        out += [(("tg_big", mode), ("tg_big_sk", sk)) for sk in sks]
        out += [(("tg_big", mode), ("tg_big_sk", sk), ("tg_big_cvar", 1)) for sk in sks[:1]]
    return out


CASES = [
    ((2, 7, 7, 256, 64, 64), ROW128),
    ((2, 14, 14, 1024, 256, 256), ROW128 + _big((1, 3), (3, 5, 7))),
    ((3, 14, 14, 512, 256, 256), _big((1,), (3,))),
    ((2, 7, 7, 512, 128, 128), ROW128 + _big((3,), ())),
]


@pytest.mark.parametrize("shape,cfgs", CASES, ids=[str(c[0]) for c in CASES])
def test_two_source_gemm_exact(K, shape, cfgs):
    N, H, W, C1, C2, Co = shape
    x, x2, w, bias, exact1, exact2, exactb = _cat_problem(shape)
    xd, x2d, wd, bd = x.to(DEV), x2.to(DEV), w.to(DEV), bias.to(DEV)
    w1d = w[:, :C1].contiguous().to(DEV)
    want1, want2, wantb = (X.rounded(e, BF16).to(DEV) for e in (exact1, exact2, exactb))
    # the single-source result of the forward conv, the reference of "src2 = nullptr changes nothing"
    y_fwd, _ = K.conv_fwd(xd, w1d.reshape(Co, 1, 1, C1), 1, 0, False)
    X.assert_exact(y_fwd, want1, X.NHWC, f"conv_fwd {shape}")
    for cfg in cfgs:
        with slots(K, cfg):
            y1 = K.conv1x1_cat(xd, None, w1d, None)
            y2 = K.conv1x1_cat(xd, x2d, wd, None)
            yb = K.conv1x1_cat(xd, x2d, wd, bd)
        assert torch.equal(y1, y_fwd), f"one source differs from conv_fwd: {shape} {_name(cfg)}"
        X.assert_exact(y2, want2, X.NHWC, f"two sources {shape} {_name(cfg)}")
        X.assert_exact(yb, wantb, X.NHWC, f"two sources + bias {shape} {_name(cfg)}")


# ----------------------------------------------------------------------------- block level
def _two_blocks(big_mean):
    torch.manual_seed(0)
    net = torch.nn.Sequential(R.Bottleneck(256, 64), R.Bottleneck(256, 64))
    with torch.no_grad():
        for blk in net:
            for bn in (blk.bn1, blk.bn2, blk.bn3):
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.normal_(0.0, 0.3)
        if big_mean:  # conv3's input relu(0.25 xhat + 8): mean 8, standard deviation 0.25
            net[0].bn2.weight.fill_(0.25)
            net[0].bn2.bias.fill_(8.0)
    return net


def _step(net, x, dy, linear):
    """forward + backward of the two blocks -> (output, {quantity: gradient of block 0}, captures)"""
    prev = Fn._BN3_LINEAR[0]
    Fn.set_bn3_linear(linear)
    cap = {}
    try:
        for p in net.parameters():
            p.grad = None
        xin = x.clone().requires_grad_(True)
        mid = net[0](xin)
        mid.register_hook(lambda g: cap.__setitem__("dy0", g.detach().clone()))
        out = net[1](mid)
        out.backward(dy)
        torch.cuda.synchronize()
    finally:
        Fn.set_bn3_linear(prev)
    grads = {n: p.grad.detach().clone() for n, p in net[0].named_parameters()}
    grads["dx"] = xin.grad.detach().clone()
    return out.detach().clone(), mid.detach().clone(), grads, cap["dy0"]


def _mirror(blk64, x, dy0, round_to):
    blk64.zero_grad(set_to_none=True)
    x64 = M._nchw64(x).requires_grad_(True)
    M.block_forward(blk64, x64, True, round_to).backward(M._nchw64(dy0))
    seg = M._param_grads(blk64)
    seg["dx"] = x64.grad * (x64.detach() > 0)
    return seg


@pytest.mark.parametrize("big_mean", [False, True], ids=["plain", "mean32sigma"])
def test_identity_block_gradients(K, big_mean):
    net = _two_blocks(big_mean)
    blk64 = copy.deepcopy(net[0]).double()
    net = net.to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.relu(torch.randn(4, 14, 14, 256, generator=g)).to(BF16).to(DEV)
    dy = torch.randn(4, 14, 14, 256, generator=g).to(BF16).to(DEV)
    out_new, mid_new, g_new, dy0_new = _step(net, x, dy, True)
    out_old, mid_old, g_old, dy0_old = _step(net, x, dy, False)
    assert torch.equal(out_new, out_old) and torch.equal(mid_new, mid_old), "forward outputs differ"
    assert torch.equal(dy0_new, dy0_old), "the gradient handed to the block under test differs"
    # the new path really ran: conv3's gradients round at other points
    assert not torch.equal(g_new["conv3.weight"], g_old["conv3.weight"]), "the linear path was not taken"
    ref = _mirror(blk64, x, dy0_new, None)
    yard = _mirror(blk64, x, dy0_new, torch.bfloat16)
    bad = []
    for path, grads in (("linear", g_new), ("elementwise", g_old)):
        for q, r in ref.items():
            ours = grads[q]
            ours = ours.double().cpu().permute(0, 3, 1, 2) * (M._nchw64(x) > 0) if q == "dx" else ours.double().cpu()
            err, y = M.rel_l2(ours, r), M.rel_l2(yard[q], r)
            print(f"{'mean32' if big_mean else 'plain'} {path} {q}: err {err:.3e} yardstick {y:.3e}")
            if not err <= max(F_BF16 * y, FLOOR):
                bad.append((path, q, err, y))
    assert not bad, bad


def test_identity_block_graph_matches_eager(K):
    net = _two_blocks(False).to(DEV)
    g = torch.Generator().manual_seed(2)
    x = torch.relu(torch.randn(4, 14, 14, 256, generator=g)).to(BF16).to(DEV)
    dy = torch.randn(4, 14, 14, 256, generator=g).to(BF16).to(DEV)

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


# ----------------------------------------------------------------------------- the op against fp64
@pytest.mark.parametrize("shape", [(2, 14, 14, 256, 1024), (2, 7, 7, 512, 2048), (3, 5, 5, 192, 768)], ids=str)
def test_conv1x1_bn_lin_bwd_matches_fp64(K, shape):
    """``conv1x1_bn_lin_bwd`` at the widths the block test does not reach (the Q product's channel slices,
    several column tiles of the fix-up, a width whose 8-channel chunks do not divide a workgroup) against
    fp64 autograd through conv1x1 -> BN on the same bf16 inputs.

    Bounds, from the number formats alone (worst case, no statistics; |.|+ is the norm of the matrix of
    sums of the terms' MAGNITUDES, which accounts for every cancellation).  d_a2 = T1 + T2 + bias with
    T1 = g (aW3), T2 = a2 Qr: every weight entry is rounded to bf16 once (relative 2^-9), and so is the
    sum: err <= 2^-9 (|T1|+ + |T2|+ + |d_a2|).  dW3 is fp32 from bf16 inputs: each of its terms is an fp32
    sum of at most n + C products (relative (n + C) 2^-24 of the magnitudes), the covariance a difference
    of two of them: err <= (n + C) 2^-24 (|t1|+ + |t2a|+ + |t2b|+ + |t3|+)."""
    N, H, W, m, C = shape
    n = N * H * W
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    a2 = (torch.relu(rnd(n, m)) + 0.5 * rnd(1, m).abs()).to(BF16)
    w3 = (rnd(C, m) / m ** 0.5).to(BF16)
    g = rnd(n, C).to(BF16)
    gamma = (rnd(C).abs() + 0.5).double()
    eps = 1e-5
    a64, w64, g64 = a2.double(), w3.double(), g.double()
    ar, wr = a64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
    x3 = ar @ wr.t()
    torch.nn.functional.batch_norm(x3, None, None, gamma, None, training=True, eps=eps).backward(g64)
    want_dx, want_dw = ar.grad, wr.grad
    x3 = x3.detach()
    mean, istd = x3.mean(0), (x3.var(0, unbiased=False) + eps).rsqrt()
    S1, S2 = g64.sum(0), (g64 * (x3 - mean) * istd).sum(0)
    a, b, e = gamma * istd, -gamma * istd * istd * S2 / n, gamma * istd * S1 / n
    cs = a64.sum(0)
    # magnitudes (a > 0, a2 >= 0)
    T1, T2 = g64.abs() @ (a[:, None] * w64).abs(), a64 @ (w64.t() @ (b[:, None] * w64)).abs()
    t1, t3 = a[:, None] * (g64.abs().t() @ a64), torch.outer(e.abs(), cs)
    t2a = b.abs()[:, None] * (w64.abs() @ (a64.t() @ a64))
    t2b = b.abs()[:, None] * (w64.abs() @ torch.outer(cs, cs)) / n
    f32 = lambda t: t.float().to(DEV)
    dx, dw = K.conv1x1_bn_lin_bwd(g.reshape(N, H, W, C).to(DEV), a2.reshape(N, H, W, m).to(DEV),
                                  w3.reshape(C, 1, 1, m).to(DEV), w3.t().contiguous().reshape(m, 1, 1, C).to(DEV),
                                  f32(a), f32(istd), torch.stack([f32(S1), f32(S2)]).contiguous(), float(n), True, True)
    torch.cuda.synchronize()
    err_dx = (dx.double().cpu().reshape(n, m) - want_dx).norm().item()
    bound_dx = 2.0 ** -9 * (T1.norm() + T2.norm() + want_dx.norm()).item()
    err_dw = (dw.double().cpu().reshape(C, m) - want_dw).norm().item()
    bound_dw = (n + C) * 2.0 ** -24 * (t1.norm() + t2a.norm() + t2b.norm() + t3.norm()).item()
    print(f"{shape}: d_a2 err {err_dx:.3e} bound {bound_dx:.3e} (|d_a2| {want_dx.norm().item():.3e}); "
          f"dW3 err {err_dw:.3e} bound {bound_dw:.3e} (|dW3| {want_dw.norm().item():.3e})")
    assert err_dx <= bound_dx
    assert err_dw <= bound_dw
