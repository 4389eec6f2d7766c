"""fp64 reference of the fused supervised contrastive loss (csrc/supcon.hip) and the seeded cases of
test_supcon_gpu.py and test_supcon_cpu.py.  :func:`supcon` takes the normalised operand rows the kernels
read (after their bf16 rounding) and evaluates the definition of README "Supervised contrastive loss" in
fp64, G rounded to bf16 when ``round_g`` (the second MFMA's operand); ``fault`` evaluates one deliberate
error instead (test_supcon_cpu.py measures what each moves)."""
import torch

from tests.head_ref import F64, f32, f64, l2norm_grad

FAULTS = ("self", "pad", "transpose", "mean")
CASES = [(4, 24, 2, 0.1),        # one tile, D padding
         (70, 37, 9, 0.1),       # two row blocks, padding columns inside the second tile
         (64, 128, 5, 0.07),     # exact tile, no padding
         (65, 512, 64, 0.07),    # one row past a tile at Dp = 512, mostly singleton classes
         (130, 200, 40, 0.1),    # D padded to 256, three row blocks
         (530, 128, 20, 0.1)]    # >= 8 column splits through the XCD remap


def case_inputs(case):
    """Seeded CPU rows and labels of CASES[case] (B, D, classes, tau), fp32 and bf16 alternating: row 0
    alone in the last class, about 5 % of the other rows invalid (the first of them 2^32 + 5, the rest -1)."""
    B, D, classes, _ = CASES[case]
    g = torch.Generator().manual_seed(100 + case)
    x = torch.randn(B, D, generator=g).to(torch.bfloat16 if case % 2 else torch.float32)
    y = torch.randint(0, classes - 1, (B,), generator=g)
    y[0] = classes - 1
    bad = 1 + torch.randperm(B - 1, generator=g)[:max(1, round(0.05 * B))]
    y[bad] = -1
    y[bad[0]] = 2 ** 32 + 5
    return x, y


def supcon(zn, inv, labels, D, tau, g=1.0, round_g=True, fault=None):
    z, y = f64(zn), labels.detach().cpu().long()
    B = len(y)
    z, it = z[:B], f32(1.0 / f32(tau))
    valid = (y >= 0) & (y < 2 ** 31)
    eye = torch.eye(B, dtype=torch.bool)
    pair = valid[:, None] & valid[None, :] & ~eye
    pos = pair & (y[:, None] == y[None, :])
    cnt = pos.sum(1)
    anchor, has = cnt > 0, pair.any(1)
    s = (z @ z.t()) * it
    den = pair | (eye & valid[:, None]) if fault == "self" else pair
    lse = torch.logsumexp(torch.where(has[:, None], s.masked_fill(~den, -float("inf")), torch.zeros_like(s)), 1)
    if fault == "pad" and B % 64:  # the padding columns as zero-vector negatives: exp(0) each
        lse = torch.logaddexp(lse, torch.tensor(float(64 - B % 64), dtype=F64).log())
    lse = torch.where(has, lse, torch.zeros_like(lse))
    safe = cnt.clamp(min=1).to(F64)
    rows = torch.where(anchor, lse - (s * pos).sum(1) / safe, torch.zeros_like(lse))
    n = B if fault == "mean" else max(1, int(anchor.sum()))
    dS = torch.where(anchor[:, None] & den, torch.exp(s - lse[:, None]) - pos / safe[:, None], torch.zeros_like(s))
    G = f32(g) * f32(1.0 / n) * it * (dS if fault == "transpose" else dS + dS.t())
    if round_g:
        G = G.float().bfloat16().to(F64)
    G = G.masked_fill(eye, 0.0)
    return {"valid": valid, "cnt": cnt, "anchor": anchor, "n": int(anchor.sum()), "lse": lse, "rows": rows,
            "loss": rows.sum() / n, "dx": l2norm_grad(G @ z, z, f64(inv)[:B], D)}
