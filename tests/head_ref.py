"""fp64 references of the loss-head, ArcFace, optimizer and CDR kernels (csrc/loss.hip, arcface.hip,
optim.hip, the head helpers of misc.hip), shared by test_loss_rows_gpu.py,
test_arcface_kernels_gpu.py and test_optim_kernels_gpu.py; verified against torch autograd in fp64 by
test_head_ref_cpu.py.

Every function takes the values a kernel reads (bf16 / fp32 tensors on any device), converts them
to fp64 on the CPU *after* their rounding and evaluates the textbook formula there.  The loss heads' scalars
that a kernel receives as ``float`` (smoothing, scale, margin constants) are rounded to fp32 first
(:func:`f32`), so a reference never differs from its kernel by an argument's rounding; the
optimizers' hyper-parameters are NOT (their references are the textbook updates).
"""
import math

import torch

F64 = torch.float64
BF16_REL = 2.0 ** -8  # one bf16 rounding (2^-9 relative) of a value with a small fp32 error


def f64(t):
    return t.detach().to("cpu").to(F64)


def f32(v):
    """A Python scalar as the kernel sees it: rounded to fp32, returned as a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def row_relerr(got, ref):
    """Per-row ||got - ref|| / ||ref|| ([R]); a row whose reference and result are both exactly zero
    has error 0."""
    got, ref = f64(got), f64(ref)
    err, den = (got - ref).norm(dim=1), ref.norm(dim=1)
    return torch.where(err == 0, torch.zeros_like(err), err / den)


def relerr(got, ref):
    got, ref = f64(got).reshape(-1), f64(ref).reshape(-1)
    err = (got - ref).norm()
    return 0.0 if err == 0 else (err / ref.norm()).item()


def bf16_excess(got, ref, atol):
    """Largest violation of the bf16 output rule |got - ref| <= 2^-8 |ref| + atol (<= 0: it holds).
    ``atol`` (scalar or broadcastable tensor) is the fp32 error of the quantity before rounding."""
    got, ref = f64(got), f64(ref)
    atol = atol if torch.is_tensor(atol) else torch.tensor(float(atol), dtype=F64)
    return ((got - ref).abs() - (BF16_REL * ref.abs() + atol)).max().item()


# ----------------------------------------------------------------------------- softmax cross-entropy
def label_info(labels, C):
    lab = labels.detach().cpu().long()
    valid = (lab >= 0) & (lab < C)
    return lab, valid, lab.clamp(0, max(C - 1, 0))


def xent_rows(x, labels, C, smoothing=0.0):
    """Rows of softmax cross-entropy over the first C columns of x.

    -> dict: loss [B] (0 on a row whose label is outside [0, C)), rank [B] (#{j : x_j > x_label},
    meaningful on valid rows), valid [B], p [B, C] (softmax), lse [B], absmax [B] (max_j |x_j|)."""
    x = f64(x)[:, :C]
    lab, valid, safe = label_info(labels, C)
    sm = f32(smoothing)
    xl = x.gather(1, safe[:, None]).squeeze(1)
    lse = torch.logsumexp(x, 1)
    loss = lse - xl
    if sm > 0:
        loss = (1.0 - sm) * loss + sm * (lse - x.mean(1))
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    rank = (x > xl[:, None]).sum(1)
    return {"loss": loss, "rank": rank, "valid": valid, "p": torch.exp(x - lse[:, None]), "lse": lse,
            "absmax": x.abs().amax(1)}


def xent_grad(x, labels, C, g, smoothing=0.0):
    """d/dx of g * sum_rows(loss) -> [B, C]; invalid rows are zero."""
    r = xent_rows(x, labels, C, smoothing)
    lab, valid, safe = label_info(labels, C)
    sm = f32(smoothing)
    tgt = torch.full_like(r["p"], sm / C)
    tgt.scatter_add_(1, safe[:, None], torch.full((len(lab), 1), 1.0 - sm, dtype=F64))
    d = float(g) * (r["p"] - tgt)
    return d * valid[:, None].to(F64)


def log_softmax_rows(x, C):
    x = f64(x)[:, :C]
    return x - torch.logsumexp(x, 1, keepdim=True)


def log_softmax_grad(y, dy):
    """dx = dy - exp(y) * sum_j dy_j from the log-probabilities y the backward kernel reads."""
    y, dy = f64(y), f64(dy)
    return dy - torch.exp(y) * dy.sum(1, keepdim=True)


def prefix_mask(x, keep):
    """x * (arange(D) < keep), in x's own dtype (exact)."""
    x = x.detach().cpu()
    m = (torch.arange(x.shape[1]) < int(keep)).to(x.dtype)
    return x * m


# ----------------------------------------------------------------------------- L2 normalisation
def l2norm_rows(x, eps):
    """-> (y [R, D] = x / max(|x|, eps), inv [R] = 1 / max(|x|, eps))."""
    x = f64(x)
    inv = 1.0 / x.norm(dim=1).clamp_min(f32(eps))
    return x * inv[:, None], inv


def l2norm_grad(dy, y, inv, D):
    """Backward of y = x / |x| from the normalised rows the kernel reads:
    dx = inv * (dy - y <dy, y>) over the first D columns."""
    dy, y, inv = f64(dy)[:, :D], f64(y)[:, :D], f64(inv)
    return inv[:, None] * (dy - y * (dy * y).sum(1, keepdim=True))


# ----------------------------------------------------------------------------- ArcFace
def arc_consts(m):
    """(cos m, sin m, cos(pi - m), sin(pi - m) * m) as the bindings compute them in fp32 (cosf / sinf
    of the fp32 arguments, taken here as the correctly rounded values)."""
    mf = f32(m)
    pim = f32(f32(3.14159265358979) - mf)
    return f32(math.cos(mf)), f32(math.sin(mf)), f32(math.cos(pim)), f32(f32(math.sin(pim)) * mf)


def arc_margin(c, m, easy):
    """Additive angular margin on label cosines c (fp64 [B]) -> (phi, dphi / dcos), with the kernels'
    guards: c clamped to [-1, 1], the sin -> 0 term dropped for sin <= 1e-6."""
    cm, sm, th, mm = arc_consts(m)
    c = c.clamp(-1.0, 1.0)
    sn = torch.sqrt((1.0 - c * c).clamp(0.0, 1.0))
    p = c * cm - sn * sm
    dp = cm + torch.where(sn > 1e-6, sm * c / sn.clamp_min(1e-300), torch.zeros_like(c))
    on = c > 0 if easy else c > th
    phi = torch.where(on, p, c if easy else c - mm)
    dphi = torch.where(on, dp, torch.ones_like(c))
    return phi, dphi


def arcface_rows(cos, labels, C, s, m, easy, g=0.0, dphi=None):
    """Margin logits + cross-entropy rows from a cosine matrix (the first C columns of ``cos``).

    -> dict: x [B, C] margin logits, t [B] target logit s * phi, loss, rank, valid, lse, dphi, and
    dcos [B, C] = g s (softmax - onehot) (* dphi on the label column), zero on invalid rows.
    ``dphi``: take the label column's factor from the caller (the forward kernel's output)."""
    cos = f64(cos)[:, :C]
    lab, valid, safe = label_info(labels, C)
    s = f32(s)
    phi, dp = arc_margin(cos.gather(1, safe[:, None]).squeeze(1), m, easy)
    vz = valid.to(F64)
    phi, dp = phi * vz, dp * vz
    t = s * phi
    x = s * cos
    onehot = torch.zeros_like(x)
    onehot[valid, safe[valid]] = 1.0
    x = torch.where(onehot > 0, t[:, None], x)
    lse = torch.logsumexp(x, 1)
    loss = (lse - t) * vz
    rank = ((x > t[:, None]) & (onehot == 0)).sum(1)
    use = dp if dphi is None else f64(dphi)
    mult = 1.0 + onehot * (use[:, None] - 1.0)
    dcos = float(g) * s * (torch.exp(x - lse[:, None]) - onehot) * mult * vz[:, None]
    return {"x": x, "t": t, "loss": loss, "rank": rank, "valid": valid, "lse": lse, "dphi": dp, "dcos": dcos,
            "onehot": onehot}


def near_ties(x, t, onehot, band):
    """#{j != label : |x_j - t| <= band} per row: how far a rank may move when both sides of the
    compare carry an error of up to band / 2."""
    return (((x - t[:, None]).abs() <= band) & (onehot == 0)).sum(1)


def arcface_head(xn, wn, inv_x, inv_w, labels, B, C, D, s, m, easy, g):
    """The whole head from the normalised bf16 operands the fused kernels read (xn [Bp, Dp],
    wn [Cp, Dp], inverse norms): cosines, margin, loss, rank, and the gradients with dcos rounded to
    bf16 (the second MFMA's operand) and both normalisation backwards on the bf16 rows.

    -> the :func:`arcface_rows` dict plus dx [B, D], dw [C, D]."""
    xn, wn = f64(xn)[:B], f64(wn)[:C]
    r = arcface_rows(xn @ wn.t(), labels, C, s, m, easy, g)
    dcos = r["dcos"].float().bfloat16().to(F64)
    r["dx"] = l2norm_grad(dcos @ wn, xn, f64(inv_x)[:B], D)
    r["dw"] = l2norm_grad(dcos.t() @ xn, wn, f64(inv_w)[:C], D)
    return r


# ----------------------------------------------------------------------------- optimizers
def sgd_step(p, g, buf, first, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, grad_scale=1.0):
    """One torch.optim.SGD update in fp64 -> (new p, new momentum buffer or None).  The
    hyper-parameters stay the caller's doubles (the textbook update, as torch.optim applies it): a
    kernel that derives a constant from a rounded one (1 - beta from an fp32 beta) is measured."""
    p, g = f64(p), f64(g) * grad_scale
    if wd != 0:
        g = g + wd * p
    if momentum != 0:
        buf = g.clone() if first else momentum * f64(buf) + (1.0 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    else:
        buf = None
    return p - lr * g, buf


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, decoupled=False, grad_scale=1.0):
    """One torch.optim.Adam / AdamW update in fp64 -> (new p, new exp_avg, new exp_avg_sq); the
    hyper-parameters stay doubles (see :func:`sgd_step`)."""
    b1, b2 = betas
    p, g, m, v = f64(p), f64(g) * grad_scale, f64(m), f64(v)
    if wd != 0:
        if decoupled:
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


# ----------------------------------------------------------------------------- CDR
def cdr_select(params, grads, nonzero_ratio, clip):
    """CDR/main.py:186-204 over the 2-D / 4-D tensors, the products formed in fp32 on the CPU.

    -> (threshold (fp32 0-dim; inf when k = 0), masked gradients (1-D and other tensors unchanged))."""
    params = [p.detach().cpu().float() for p in params]
    grads = [g.detach().cpu().float() for g in grads]
    sel = [i for i, p in enumerate(params) if p.dim() in (2, 4)]
    metric = torch.cat([(grads[i] * params[i]).abs().reshape(-1) for i in sel])
    k = int(nonzero_ratio * metric.numel())
    out = [g.clone() for g in grads]
    if k <= 0:
        for i in sel:
            out[i].zero_()
        return torch.tensor(float("inf")), out
    thr = torch.topk(metric, k)[0][-1]
    c = torch.tensor(float(clip), dtype=torch.float32)
    for i in sel:
        keep = (grads[i] * params[i]).abs() >= thr
        out[i] = torch.where(keep, grads[i] * c, torch.zeros_like(grads[i]))
    return thr, out
