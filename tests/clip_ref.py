"""Reference of global gradient-norm clipping, the non-finite skip and the two trust clamps
(csrc/optim.hip: mt_gnorm2 / gnorm_finish and the clip block the update kernels read; optim/fused.py:
_GradClip), shared by test_clip_cpu.py, test_clip_kernels_gpu.py and test_clip_graph_gpu.py.

    norm = fl32(sqrt(sum over groups of grad_scale^2 * sum over the group's gradients of g^2))   fp64 sum
    coef = fl32(fl32(max_norm) / fl32(norm + fl32(1e-6))), replaced by 1 when it exceeds 1; NaN stays NaN
    skip = skip_nonfinite and norm is inf or NaN
    the clipped step = the plain step with grad_scale' = fl32(fl32(grad_scale) * coef)

    LARS trust_clip:   trust' = min(fl32(trust / lr), 1)   (1 when lr <= 0; only where trust is adaptive)
    LAMB phi:          trust  = fl32(clamp(|w|, phi_min, phi_max) / |u|)

The norm's bound, counted from the kernels' chain of fp32 operations as lamb_ref counts its trust
ratio: a chunk partial is within 25 u of the sum of the squares it adds (16 fused multiply-adds in
series per thread, 6 butterfly levels, 3 additions of block_sum; u = 2^-24); every term is
non-negative, so the fp64 merge of the partials (its own error ~1e-16) keeps 25 u relative; the
square root halves that (12.5 u) and the one rounding to fp32 adds 1:  K_NORM = 13.5, 8.0e-7.
"""
import numpy as np
import torch

from tests import lars_ref as L

F32 = np.float32
U = 2.0 ** -24
SLACK = 1.001     # second-order terms
K_NORM = 12.5 + 1.0
EPS = F32(1e-6)


def global_norm64(grads, scales=None, drop=None, drop_tail_of=None):
    """The norm in fp64 (a Python float).  ``grads``: tensors; ``scales``: their groups' grad_scale
    (rounded to fp32, as the kernel's argument is).  ``drop``: leave that tensor out; ``drop_tail_of``:
    leave out the last (partial) chunk of that tensor (both only for the sensitivity checks)."""
    total = 0.0
    for i, g in enumerate(grads):
        if g is None or i == drop:
            continue
        x = L.f64(g).reshape(-1)
        if i == drop_tail_of:
            x = x[:(x.numel() - 1) // L.CHUNK * L.CHUNK]
        gs = float(F32(1.0 if scales is None else scales[i]))
        total += gs * gs * float((x * x).sum())
    return total ** 0.5 if total == total else float("nan")


def global_norm(grads, scales=None, **kw):
    """The norm rounded to fp32 once."""
    return F32(global_norm64(grads, scales, **kw))


def clip_coef(norm, max_norm, eps=EPS):
    """The fp32 coefficient from the fp32 norm, every operation rounded on its own."""
    if not max_norm > 0:
        return F32(1.0)
    with np.errstate(all="ignore"):
        c = F32(max_norm) / (F32(norm) + F32(eps))   # numpy float32 operands: one rounding per operation
    assert c.dtype == np.float32
    return F32(1.0) if c > 1 else c                  # a NaN compares false and stays


def skips(norm, skip_nonfinite):
    return bool(skip_nonfinite and not np.isfinite(F32(norm)))


def eff_scale(grad_scale, coef):
    """grad_scale' of the clipped step: one fp32 product."""
    with np.errstate(all="ignore"):
        return float(F32(grad_scale) * F32(coef))


def eps_is_absorbed(norm):
    """The lattice's precondition: norm + 1e-6 rounds back to norm in fp32, so with a power-of-two
    norm and max_norm the coefficient is an exact power of two."""
    return bool(F32(norm) + EPS == F32(norm))


def lars_trust_clip(trust, lr):
    """LARC's clip mode on an adaptive trust ratio, in fp32."""
    if not lr > 0:
        return F32(1.0)
    t = F32(trust) / F32(lr)
    return F32(1.0) if t > 1 else t


def lamb_trust_phi(wn, un, phi_min=0.0, phi_max=float("inf")):
    """LAMB's trust ratio with |w| clamped to [phi_min, phi_max], in fp32 from the fp32 norms."""
    wn, un = F32(wn), F32(un)
    if not (wn > 0 and un > 0):
        return F32(1.0)
    return min(max(wn, F32(phi_min)), F32(phi_max)) / un


def norm_lattice(sizes, total_exp, s_exp, gen):
    """Gradients on the lattice: entries 0 or +-2^s_exp, 4^a non-zero entries in total with
    a + s_exp = total_exp, so the global norm is exactly 2^total_exp.  Every tensor gets at least its
    edge positions (last element, first element of the second chunk); the rest is dealt out over the
    tensors in proportion to their free room."""
    a = total_exp - s_exp
    want = 4 ** a
    musts = [L.edge_positions(n) for n in sizes]
    counts = [len(m) for m in musts]
    room = [n - c for n, c in zip(sizes, counts)]
    left = want - sum(counts)
    assert 0 <= left <= sum(room), "the lattice does not fit these sizes"
    for i in sorted(range(len(sizes)), key=lambda i: -room[i]):
        take = min(room[i], left)
        counts[i] += take
        left -= take
    assert left == 0 and sum(counts) == want
    return [L.lattice(n, c, 0, s_exp, m, gen) for n, c, m in zip(sizes, counts, musts)]
