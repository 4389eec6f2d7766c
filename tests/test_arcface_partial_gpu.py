"""Partial FC on the GPU (csrc/arcface_pfc.hip): the device-side sampler against its definition
(``_ref.pfc_sample``), the sampled head bit for bit against the full fused head on the gathered rows,
sample_rate = 1 against the full head, the gradients against fp64, and HIP-graph replays that draw a
new subset each."""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.ops import _ref
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests.test_arcface_fused_gpu import relerr
from tests.test_arcface_partial_cpu import head64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x1234567_89ABCDEF


def _labels(B, C):
    """Random labels with a duplicate, a -1 and a C among them."""
    lab = torch.randint(0, C, (B,))
    lab[1], lab[2], lab[3] = lab[0], -1, C
    return lab


def _sample(lab, C, Cs, step):
    idx, slot, lab2 = _ext.hip_ops().pfc_sample(lab.to(DEV), C, Cs, SEED, step)
    return idx.cpu(), slot.cpu(), lab2.cpu()


@pytest.mark.parametrize("B,C,rate", [(8, 100, 0.1), (64, 1000, 0.25), (300, 257, 0.5), (16, 70001, 0.1), (5, 1, 1.0)])
def test_sampler_equals_definition(B, C, rate):
    torch.manual_seed(C)
    lab, Cs = _labels(B, C), _ref.pfc_num_sampled(B, C, rate)
    step = torch.full((1,), (3 << 32) + 5, dtype=torch.int64, device=DEV)
    idx, slot, lab2 = _sample(lab, C, Cs, step)
    assert int(step) == (3 << 32) + 6
    # from the output alone
    Csp = (Cs + 63) // 64 * 64
    assert idx.shape == (Csp,) and slot.shape == (C,) and (idx[Cs:] == -1).all()
    assert (idx[:Cs] >= 0).all() and (idx[:Cs] < C).all() and (idx[1:Cs] > idx[:Cs - 1]).all()
    assert torch.equal(slot[idx[:Cs].long()], torch.arange(Cs, dtype=torch.int32)) and (slot >= 0).sum() == Cs
    valid = (lab >= 0) & (lab < C)
    assert (slot[lab[valid]] >= 0).all() and (lab2[~valid] == -1).all()
    # the definition
    ridx, rslot, rlab = _ref.pfc_sample(lab, C, Cs, SEED, (3 << 32) + 5)
    assert torch.equal(idx, ridx) and torch.equal(slot, rslot) and torch.equal(lab2, rlab)


def test_sampler_counter_advances_and_resets():
    torch.manual_seed(0)
    B, C, Cs = 16, 70001, 7001
    lab = _labels(B, C)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    first, second = _sample(lab, C, Cs, step)[0], _sample(lab, C, Cs, step)[0]
    assert int(step) == 2 and not torch.equal(first, second)
    assert torch.equal(second, _ref.pfc_sample(lab, C, Cs, SEED, 1)[0])
    step.zero_()
    assert torch.equal(_sample(lab, C, Cs, step)[0], first)


def _partial(x, W, lab, easy, rate):
    """One sampled step -> (loss, rank, idx, dx, dW)."""
    xd, Wd = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    loss, rank, idx = Fn.arcface_partial_loss(xd, Wd, lab, 30.0, 0.5, easy, sample_rate=rate)
    loss.backward()
    return loss.detach(), rank, idx, xd.grad, Wd.grad


def _full(x, W, lab, easy):
    xd, Wd = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    loss, rank, _ = Fn.arcface_loss(xd, Wd, lab, 30.0, 0.5, easy)
    loss.backward()
    return loss.detach(), rank, xd.grad, Wd.grad


def _inputs(B, C, D, dtype=torch.float32):
    torch.manual_seed(B + C)
    return (torch.randn(B, D, device=DEV).to(dtype), (torch.randn(C, D) * 0.05).to(DEV),
            torch.randint(0, C, (B,), device=DEV))


@pytest.mark.parametrize("B,C,D,rate,dtype,easy", [(48, 700, 100, 0.3, torch.float32, True),
                                                   (100, 1000, 256, 0.2, torch.bfloat16, False),
                                                   (40, 333, 300, 0.5, torch.float32, False)])
def test_sampled_head_is_full_head_on_gathered_rows(B, C, D, rate, dtype, easy):
    x, W, lab = _inputs(B, C, D, dtype)
    loss, rank, idx, dx, dw = _partial(x, W, lab, easy, rate)
    Cs = _ref.pfc_num_sampled(B, C, rate)
    assert idx.shape == (Cs,) and Cs % 64 != 0 and dx.dtype == dtype
    slot = torch.full((C,), -1, dtype=torch.int64, device=DEV)
    slot[idx.long()] = torch.arange(Cs, device=DEV)
    lf, rf, dxf, dwf = _full(x, W[idx.long()].clone(), slot[lab], easy)
    assert torch.equal(loss, lf) and torch.equal(rank, rf) and torch.equal(dx, dxf)
    assert torch.equal(dw[idx.long()], dwf) and dwf.abs().sum() > 0
    assert (dw[slot < 0] == 0).all() and dw.shape == (C, D)


def test_rate_one_is_the_full_head():
    B, C, D = 64, 300, 256
    x, W, lab = _inputs(B, C, D)
    loss, rank, idx, dx, dw = _partial(x, W, lab, True, 1.0)
    lf, rf, dxf, dwf = _full(x, W, lab, True)
    assert torch.equal(idx.cpu(), torch.arange(C, dtype=torch.int32))
    assert torch.equal(loss, lf) and torch.equal(rank, rf) and torch.equal(dx, dxf) and torch.equal(dw, dwf)


@pytest.mark.parametrize("B,C,D,rate", [(32, 1000, 256, 0.1), (48, 700, 512, 0.25)])
def test_sampled_head_against_fp64(B, C, D, rate):
    x, W, lab = _inputs(B, C, D)
    loss, _, idx, dx, dw = _partial(x, W, lab, True, rate)
    ii = idx.long().cpu()
    slot = torch.full((C,), -1, dtype=torch.int64)
    slot[ii] = torch.arange(len(ii))
    lr, _, dxr, dwr = head64(x.cpu(), W.cpu()[ii], slot[lab.cpu()], 30.0, 0.5, True)
    print(f"loss {loss.item():.6f} ref {lr.item():.6f} dx {relerr(dx, dxr):.3e} dW {relerr(dw[idx.long()], dwr):.3e}")
    assert torch.isfinite(loss) and torch.isfinite(dx).all() and torch.isfinite(dw).all()
    assert abs(loss.item() - lr.item()) / abs(lr.item()) < 1e-2
    rx, rw = torch.isfinite(dxr).all(1), torch.isfinite(dwr).all(1)
    assert rx.all() and rw.all()
    assert relerr(dx[rx.to(DEV)], dxr[rx]) < 3e-2 and relerr(dw[idx.long()][rw.to(DEV)], dwr[rw]) < 3e-2


def test_graph_replays_draw_new_subsets():
    B, C, D, rate = 48, 700, 100, 0.3
    x, W, lab = _inputs(B, C, D)
    Cs = _ref.pfc_num_sampled(B, C, rate)
    _partial(x, W, lab, True, rate)  # the eager step that creates the device counter
    seed, step = Fn.pfc_state(x.device)
    xs, Ws = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs.grad = Ws.grad = None
            Fn.arcface_partial_loss(xs, Ws, lab, 30.0, 0.5, True, sample_rate=rate)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    xs.grad = Ws.grad = None
    with torch.cuda.graph(graph):
        loss, _, idx = Fn.arcface_partial_loss(xs, Ws, lab, 30.0, 0.5, True, sample_rate=rate)
        loss.backward()
    n = int(step)
    got = []
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(step) == n + i + 1
        assert torch.equal(idx.cpu(), _ref.pfc_sample(lab, C, Cs, seed, n + i)[0][:Cs])
        got.append((loss.clone(), idx.clone(), xs.grad.clone(), Ws.grad.clone()))
    assert not torch.equal(got[0][1], got[1][1])
    for i, (gl, gi, gdx, gdw) in enumerate(got):
        step.fill_(n + i)
        el, _, ei, edx, edw = _partial(x, W, lab, True, rate)
        assert torch.equal(gl, el) and torch.equal(gi, ei) and torch.equal(gdx, edx) and torch.equal(gdw, edw)
