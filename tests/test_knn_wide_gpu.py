"""Wide fused cosine top-k (csrc/knn_wide.hip, k <= 256, an LDS candidate pool) and the kNN label vote on
the GPU: bit-exact on integer lattices and monotone streams, within the derived fp32 bound on random
normalised rows; the vote against its fp64 definition."""
import math

import pytest
import torch

from ddp_classification_pytorch_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ref_topk(E, k, exclude=None):
    """E fp64 [Nq, Ng] -> (val fp32, idx int32): excluded columns -inf, stable descending sort, (-inf, -1)
    past the candidates."""
    E = E.clone()
    if exclude is not None:
        E[torch.arange(E.shape[1], device=E.device)[None, :] == exclude[:, None]] = -math.inf
    v, i = torch.sort(E, dim=1, descending=True, stable=True)
    pad = max(0, k - E.shape[1])
    v = torch.cat([v[:, :k], v.new_full((E.shape[0], pad), -math.inf)], 1)
    i = torch.cat([i[:, :k], i.new_full((E.shape[0], pad), -1)], 1)
    i = torch.where(v == -math.inf, torch.full_like(i, -1), i)
    return v.float(), i.int()


def ref_vote(val, idx, gl, ql, T, weighted):
    """The definition in fp64 on the given fp32 val -> (pred, conf, agree, margin between the two best shares)."""
    valid = idx >= 0
    lab = gl[idx.clamp(min=0).long()]
    w = torch.exp((val.double() - val[:, :1].double()) / T) if weighted else torch.ones_like(val, dtype=torch.float64)
    w = w * valid
    C = int(gl.max()) + 1
    votes = torch.zeros(val.shape[0], C, dtype=torch.float64, device=val.device).scatter_add_(1, lab, w)
    W = w.sum(1)
    share = torch.where(W[:, None] > 0, votes / W[:, None].clamp(min=1e-300), torch.zeros_like(votes))
    top2 = share.topk(2, dim=1).values
    first = torch.where(share == share.amax(1, keepdim=True), torch.arange(C, device=val.device), C).amin(1)
    pred = torch.where(valid.any(1), first, torch.full_like(first, -1))
    return pred, share.amax(1), share.gather(1, ql[:, None]).squeeze(1), top2[:, 0] - top2[:, 1]


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("Nq,Ng,D,k,splits", [(5, 100, 40, 256, 1), (70, 3000, 64, 9, 1), (70, 3000, 256, 64, 3),
                                              (130, 3000, 384, 200, 8), (33, 2100, 512, 256, 1)])
def test_lattice_bit_for_bit(Nq, Ng, D, k, splits, own, negative):
    """Integer entries in [-2, 2]: exact fp32 scores in any order, ties everywhere.  ``negative``: every
    score is below zero, so a zero padding row would win if it were a candidate."""
    gen = torch.Generator().manual_seed(Nq * 1000 + Ng)
    if negative:
        q = torch.randint(1, 3, (Nq, D), generator=gen).float().to(DEV)
        g = -torch.randint(1, 3, (Ng, D), generator=gen).float().to(DEV)
    else:
        q = torch.randint(-2, 3, (Nq, D), generator=gen).float().to(DEV)
        g = torch.randint(-2, 3, (Ng, D), generator=gen).float().to(DEV)
    ex = torch.arange(Nq, device=DEV, dtype=torch.int32) if own else None
    val, idx = Fn.cosine_topk_wide(q, g, k, normalize=False, exclude=ex, splits=splits)
    rv, ri = ref_topk(q.double() @ g.double().t(), k, ex)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32
    assert torch.equal(val, rv)
    assert torch.equal(idx, ri)


def test_same_bits_for_any_split_count_and_run():
    torch.manual_seed(1)
    q, g = torch.randn(130, 200, device=DEV), torch.randn(3000, 200, device=DEV)
    outs = [Fn.cosine_topk_wide(q, g, 100, splits=s) for s in (1, 3, 8, 1)]
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


@pytest.mark.parametrize("k", [9, 64, 256])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_monotone_streams(sign, k):
    """g_i = (i mod 16, i div 16), q = +-(1, 16): the score is +-i.  Ascending, every candidate enters the
    pool (the most prunes); descending, nothing enters after the first KCAP."""
    i = torch.arange(3000, device=DEV)
    g = torch.stack([i % 16, i // 16], 1).float()
    q = sign * torch.tensor([[1.0, 16.0]], device=DEV)
    val, idx = Fn.cosine_topk_wide(q, g, k, normalize=False, splits=1)
    rv, ri = ref_topk(q.double() @ g.double().t(), k)
    assert torch.equal(val, rv) and torch.equal(idx, ri)


@pytest.mark.parametrize("k", [1, 4, 8])
def test_small_k_equals_cosine_topk(k):
    torch.manual_seed(5)
    q, g = torch.randn(130, 200, device=DEV), torch.randn(700, 200, device=DEV)
    ex = torch.arange(130, device=DEV, dtype=torch.int32)
    a, b = Fn.cosine_topk_wide(q, g, k, exclude=ex), Fn.cosine_topk(q, g, k, exclude=ex)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.fixture(scope="module", params=[(130, 700, 256, 200, 5), (70, 3000, 512, 256, 10)])
def random_case(request):
    """Random normalised rows, the fp64 scores of the SAME bf16 operands, and the wide op's output."""
    Nq, Ng, D, k, C = request.param
    gen = torch.Generator().manual_seed(3)  # (the fp64 reference alone leaves out no row of either case)
    q, g = torch.randn(Nq, D, generator=gen).to(DEV), torch.randn(Ng, D, generator=gen).to(DEV)
    qn, gn = Fn.knn_operand(q), Fn.knn_operand(g)
    E = qn[:Nq].double() @ gn[:Ng].double().t()
    val, idx = Fn.cosine_topk_wide(q, g, k)
    gl, ql = torch.randint(0, C, (Ng,), generator=gen).to(DEV), torch.randint(0, C, (Nq,), generator=gen).to(DEV)
    return E, qn.shape[1], k, val, idx, gl, ql


def test_random_normalised_within_fp32_bound(random_case):
    """Products of two bf16 numbers are exact in fp32, so any summation order errs by at most
    Dp 2^-24 |q||g| with |q|, |g| <= 1 + 2^-8: tol = 1.01 Dp 2^-24, position by position and for the score
    of every returned index.  Orderings of near-ties are never compared."""
    E, Dp, k, val, idx, _, _ = random_case
    tol = 1.01 * Dp * 2.0 ** -24
    li = idx.long()
    assert ((li >= 0) & (li < E.shape[1])).all()
    assert all(len(set(r)) == k for r in li.tolist())
    pos = (val.double() - torch.sort(E, dim=1, descending=True).values[:, :k]).abs().max().item()
    own = (val.double() - E.gather(1, li)).abs().max().item()
    print(f"max |val_j - ref_j| {pos:.3e}, max |val - E[idx]| {own:.3e}, tol {tol:.3e}")
    assert pos <= tol
    assert own <= tol


@pytest.mark.parametrize("T", [0.07, 1.0])
def test_weighted_vote_against_fp64(random_case, T):
    """tol = 2 (k 2^-24 + (2 / T + 3) 2^-23): a k-term fp32 sum plus exp of an argument of magnitude
    <= 2 / T, doubled for the quotient.  pred is compared where the reference's two best shares differ by
    more than 2 tol; at most 2 % of the rows may be left out."""
    _, _, k, val, idx, gl, ql = random_case
    pred, conf, agree = Fn.knn_vote(val, idx, gl, ql, temperature=T)
    rp, rc, ra, margin = ref_vote(val, idx, gl, ql, T, True)
    tol = 2 * (k * 2.0 ** -24 + (2 / T + 3) * 2.0 ** -23)
    ec, ea = (conf.double() - rc).abs().max().item(), (agree.double() - ra).abs().max().item()
    clear = margin > 2 * tol
    print(f"conf err {ec:.3e}, agree err {ea:.3e}, tol {tol:.3e}, rows left out {(~clear).sum().item()}")
    assert pred.dtype == torch.int64 and conf.dtype == torch.float32
    assert ec <= tol and ea <= tol
    assert (~clear).float().mean().item() <= 0.02
    assert torch.equal(pred[clear], rp[clear])


def test_majority_vote_ties_and_empty_rows():
    """Integer votes, exact: the smallest class wins a tie, a row without neighbours gives (-1, 0, 0)."""
    gl = torch.tensor([3, 1, 1, 3, 2, 0, 7], device=DEV)
    idx = torch.tensor([[0, 1, 2, 3], [4, 5, -1, -1], [-1, -1, -1, -1], [6, 0, 3, 1], [2, -1, 4, 4]],
                       device=DEV, dtype=torch.int32)
    val = torch.linspace(1, 0, 20, device=DEV).view(5, 4)
    ql = torch.tensor([3, 2, 0, 1, 2], device=DEV)
    pred, conf, agree = Fn.knn_vote(val, idx, gl, ql, weighted=False)
    rp, rc, ra, _ = ref_vote(val, idx, gl, ql, 0.07, False)
    assert pred.tolist() == [1, 0, -1, 3, 2]
    assert torch.equal(pred, rp) and torch.equal(conf, rc.float()) and torch.equal(agree, ra.float())
    big_i = torch.randint(-1, 7, (67, 256), device=DEV, dtype=torch.int32)
    big_q = torch.randint(0, 8, (67,), device=DEV)
    pred, conf, agree = Fn.knn_vote(torch.zeros(67, 256, device=DEV), big_i, gl, big_q, weighted=False)
    rp, rc, ra, _ = ref_vote(torch.zeros(67, 256, device=DEV), big_i, gl, big_q, 0.07, False)
    assert torch.equal(pred, rp) and torch.equal(conf, rc.float()) and torch.equal(agree, ra.float())
    assert Fn.knn_vote(val, idx, gl)[2] is None


def test_classify_runs_both_routes():
    torch.manual_seed(6)
    q, g = torch.randn(70, 64, device=DEV), torch.randn(300, 64, device=DEV)
    gl = torch.randint(0, 5, (300,), device=DEV)
    for k, top in ((8, Fn.cosine_topk), (50, Fn.cosine_topk_wide)):
        out = Fn.knn_classify(q, g, gl, k)
        ref = Fn.knn_vote(*top(q, g, k), gl)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])


@pytest.mark.parametrize("bad", [dict(D=513), dict(k=0), dict(k=257)])
def test_limits_raise(bad):
    q = torch.zeros(4, bad.get("D", 64), device=DEV)
    with pytest.raises(ValueError, match="cosine_topk_wide covers"):
        Fn.cosine_topk_wide(q, q, bad.get("k", 1))
