"""fp64 reference of the fused Sub-center ArcFace head (csrc/arcface_sub.hip) and the lattice inputs
of test_arcface_sub_gpu.py.  The head is tests/head_ref.py's ``arcface_rows`` on the max over the K
centres, a scatter of dcos to the first maximum, then ``l2norm_grad``."""
import torch

from tests import head_ref as R

F64 = R.F64


def operand_rows(C, K):
    """[C, K] -> row of centre (c, k) in the kernels' sub-centre-planar operand order, and the padded
    row count: 64-row tiles of (4 / KP class groups) x (KP planes) x 16 classes, KP = 2 for K = 2 else 4."""
    KP = 2 if K == 2 else 4
    CT = 64 // KP
    c = torch.arange(C)[:, None]
    k = torch.arange(K)[None, :]
    return (c // CT) * 64 + ((c % CT) // 16 * KP + k) * 16 + c % 16, (C + CT - 1) // CT * 64


def lattice_inputs(B, C, K, D, seed):
    """x [B, D], W [C, K, D] fp32, labels [B] (two invalid: -1 and C + 3).  Every row has 64 non-zero
    entries +-2^e (one e per row): the squared norm is a power of four, the normalised entries are
    exactly +-1/8, every cosine a multiple of 1/64 and every partial sum exact.  The centres of a class
    are drawn from two directions of that class (at another scale), so exact ties between sub-centres
    occur at every (row, class) with K >= 3 and at about half of them with K = 2."""
    g = torch.Generator().manual_seed(seed)

    def rows(n):
        v = torch.zeros(n, D)
        for r in range(n):
            idx = torch.randperm(D, generator=g)[:64]
            v[r, idx] = (torch.randint(0, 2, (64,), generator=g) * 2 - 1).float()
        return v

    def scale(v):
        return v * torch.exp2(torch.randint(-3, 4, v.shape[:-1], generator=g).float()).unsqueeze(-1)

    x = scale(rows(B))
    pool = rows(2 * C).view(C, 2, D)
    pick = torch.randint(0, 2, (C, K), generator=g)
    W = scale(pool.gather(1, pick[:, :, None].expand(C, K, D)))
    lab = torch.randint(0, C, (B,), generator=g)
    lab[1], lab[B - 2] = -1, C + 3
    return x, W, lab


def sub_head(xn, wn, inv_x, inv_w, labels, D, s, m, easy, g, rule="first", route="winner"):
    """xn [B, Dp], wn [C, K, Dp] (the normalised bf16 operands), inverse norms [B], [C, K].
    -> the ``arcface_rows`` dict on cbar = max_k cos, plus sub_idx [B, C] (the first maximum), dx [B, D],
    dw [C, K, D] with dcos rounded to bf16.  ``rule="last"`` / ``route="all"`` are the two deliberate
    errors the module docstring of test_arcface_sub_gpu.py measures the inputs against."""
    xn, wn = R.f64(xn), R.f64(wn)
    C, K, Dp = wn.shape
    cos = torch.einsum("bd,ckd->bck", xn, wn)
    top = cos == cos.amax(2, keepdim=True)
    ar = torch.arange(K)
    kst = torch.where(top, ar, K).amin(2) if rule == "first" else torch.where(top, ar, -1).amax(2)
    r = R.arcface_rows(cos.amax(2), labels, C, s, m, easy, g)
    dcos = r["dcos"].float().bfloat16().to(F64)
    d3 = dcos[:, :, None].expand(-1, -1, K).clone()
    if route == "winner":
        d3 = torch.zeros_like(d3).scatter_(2, kst[:, :, None], dcos[:, :, None])
    r["sub_idx"] = kst
    r["dx"] = R.l2norm_grad(torch.einsum("bck,ckd->bd", d3, wn), xn, inv_x, D)
    dwn = torch.einsum("bck,bd->ckd", d3, xn).reshape(C * K, Dp)
    r["dw"] = R.l2norm_grad(dwn, wn.reshape(C * K, Dp), R.f64(inv_w).reshape(-1), D).reshape(C, K, D)
    return r
