"""Fused cosine top-k retrieval (csrc/knn.hip) on the GPU: bit-exact on an integer lattice where ties are
everywhere, within the derived fp32 bound on random normalised rows, its memory, and HIP-graph replay."""
import math

import pytest
import torch

from ddp_classification_pytorch_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ref_topk(E, k, exclude=None, ql=None, gl=None):
    """E fp64 [Nq, Ng] -> (val fp32, idx int32, first_hit int32): excluded columns -inf, stable descending
    sort, (-inf, -1) past the candidates."""
    E = E.clone()
    if exclude is not None:
        E[torch.arange(E.shape[1], device=E.device)[None, :] == exclude[:, None]] = -math.inf
    v, i = torch.sort(E, dim=1, descending=True, stable=True)
    pad = max(0, k - E.shape[1])
    v = torch.cat([v[:, :k], v.new_full((E.shape[0], pad), -math.inf)], 1)
    i = torch.cat([i[:, :k], i.new_full((E.shape[0], pad), -1)], 1)
    i = torch.where(v == -math.inf, torch.full_like(i, -1), i)
    hit = None
    if ql is not None:
        same = (gl[i.clamp(min=0)] == ql[:, None]) & (i >= 0)
        hit = torch.where(same, torch.arange(k, device=E.device), k).amin(1).int()
    return v.float(), i.int(), hit


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("Nq,Ng,D,k,splits", [(1, 1, 128, 8, 1), (70, 63, 100, 3, 1), (65, 130, 256, 8, 3),
                                              (130, 600, 200, 5, 8), (64, 65, 384, 1, 2)])
def test_lattice_bit_for_bit(Nq, Ng, D, k, splits, own, negative):
    """Integer entries in [-2, 2] are exact in bf16 and every partial sum is an integer below 2^24, so the
    fp32 score is exact in any order: val, idx and first_hit must equal the fp64 reference, ties and all.
    ``negative``: every score is below zero, so a zero padding row would win if it were a candidate."""
    gen = torch.Generator().manual_seed(Nq * 1000 + Ng)
    if negative:
        q = torch.randint(1, 3, (Nq, D), generator=gen).float()
        g = -torch.randint(1, 3, (Ng, D), generator=gen).float()
    else:
        q = torch.randint(-2, 3, (Nq, D), generator=gen).float()
        g = torch.randint(-2, 3, (Ng, D), generator=gen).float()
    ql, gl = torch.randint(0, 5, (Nq,), generator=gen).to(DEV), torch.randint(0, 5, (Ng,), generator=gen).to(DEV)
    q, g = q.to(DEV), g.to(DEV)
    ex = torch.arange(Nq, device=DEV, dtype=torch.int32) if own else None
    val, idx, hit = Fn.cosine_topk(q, g, k, normalize=False, exclude=ex, q_labels=ql, g_labels=gl, splits=splits)
    rv, ri, rh = ref_topk(q.double() @ g.double().t(), k, ex, ql, gl)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and hit.dtype == torch.int32
    assert torch.equal(val, rv)
    assert torch.equal(idx, ri)
    assert torch.equal(hit, rh)


def test_same_bits_for_any_split_count():
    torch.manual_seed(1)
    q, g = torch.randn(130, 200, device=DEV), torch.randn(600, 200, device=DEV)
    ql, gl = torch.randint(0, 7, (130,), device=DEV), torch.randint(0, 7, (600,), device=DEV)
    outs = [Fn.cosine_topk(q, g, 5, q_labels=ql, g_labels=gl, splits=s) for s in (1, 2, 8)]
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [100, 200, 300])
def test_operand_bits_equal_arcface_operands(D, dtype):
    """knn_prep with normalize=True and the ArcFace operand kernel normalise a row through the same
    helper (csrc/score_tile.cuh: norm_row): the same bits, and zero padding in both."""
    from ddp_classification_pytorch_amd import _ext

    torch.manual_seed(3)
    x = torch.randn(70, D, device=DEV).to(dtype)
    Dp = Fn.arcface_fused_dp(D)
    assert Dp == {100: 128, 200: 256, 300: 512}[D]
    kn = Fn.knn_operand(x)
    an = _ext.hip_ops().arcface_l2norm_t(x, 128, Dp, 1e-12)[0]
    assert kn.shape == (128, Dp) and an.shape == (128, Dp)
    assert torch.equal(kn[:70], an[:70]) and kn[:70, :D].any()
    for t in (kn, an):
        assert not t[70:].any() and not t[:, D:].any()


@pytest.mark.parametrize("Nq,Ng,D,k", [(130, 700, 256, 8), (70, 300, 512, 4)])
def test_random_normalised_within_fp32_bound(Nq, Ng, D, k):
    """Against fp64 on the SAME bf16 operands (the preparation kernel's output).  Products of two bf16
    numbers are exact in fp32, so any summation order errs by at most Dp 2^-24 |q||g| with
    |q|, |g| <= 1 + 2^-8: tol = 1.01 Dp 2^-24.  Orderings of near-ties are never compared."""
    torch.manual_seed(2)
    q, g = torch.randn(Nq, D, device=DEV), torch.randn(Ng, D, device=DEV)
    qn, gn = Fn.knn_operand(q), Fn.knn_operand(g)
    Dp = qn.shape[1]
    assert qn.dtype == torch.bfloat16 and Dp == D and not qn[Nq:].any() and not gn[Ng:].any()
    E = qn[:Nq].double() @ gn[:Ng].double().t()
    tol = 1.01 * Dp * 2.0 ** -24
    val, idx = Fn.cosine_topk(q, g, k)
    li = idx.long()
    assert ((li >= 0) & (li < Ng)).all()
    assert all(len(set(r)) == k for r in li.tolist())
    err = (val.double() - E.gather(1, li)).abs().max().item()
    rest = E.scatter(1, li, -math.inf).amax(1)  # the best gallery row NOT returned
    over = (rest - val[:, k - 1].double()).max().item()
    print(f"max |val - E| {err:.3e}, max (unreturned - kth) {over:.3e}, tol {tol:.3e}")
    assert err <= tol
    assert over <= 2 * tol


def test_memory_far_below_the_score_matrix():
    """(8192, 65536, 256, k = 8): operands and partials are ~ 110 MB by the byte count; the bound is a
    quarter of the fp32 [Nq, Ng] matrix (512 MB of 2 GB)."""
    torch.manual_seed(3)
    Nq, Ng = 8192, 65536
    q, g = torch.randn(Nq, 256, device=DEV), torch.randn(Ng, 256, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    val, idx = Fn.cosine_topk(q, g, 8)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak extra memory {extra / 2**20:.1f} MB")
    assert extra < Nq * Ng * 4 // 4
    assert val.shape == (Nq, 8) and (idx >= 0).all() and (val[:, :-1] >= val[:, 1:]).all()


def test_graph_replay_equals_eager():
    torch.manual_seed(4)
    Nq, Ng, D, k = 130, 600, 200, 5
    q, g = torch.randn(Nq, D, device=DEV), torch.randn(Ng, D, device=DEV)
    ql, gl = torch.randint(0, 7, (Nq,), device=DEV), torch.randint(0, 7, (Ng,), device=DEV)
    ex = torch.arange(Nq, device=DEV, dtype=torch.int32)
    call = lambda: Fn.cosine_topk(q, g, k, exclude=ex, q_labels=ql, g_labels=gl)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(3):  # inputs overwritten in place: every replay against the eager call
        q.normal_()
        g.normal_()
        gl.random_(0, 7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, call()))


@pytest.mark.parametrize("bad", [dict(D=513), dict(k=0), dict(k=9)])
def test_limits_raise(bad):
    q = torch.zeros(4, bad.get("D", 64), device=DEV)
    with pytest.raises(ValueError, match="cosine_topk covers"):
        Fn.cosine_topk(q, q, bad.get("k", 1))
