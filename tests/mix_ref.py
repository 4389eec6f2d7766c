"""fp64 oracles of the Mixup / CutMix kernels, written from the definitions (not from the kernels or
ops/_ref.py): the mixed input kernels (csrc/misc.hip) and the two-label cross-entropy
(csrc/loss.hip).  Shared by test_mix_cpu.py, test_mix_input_gpu.py, test_mix_loss_gpu.py and
test_mix_graph_gpu.py; test_mix_cpu.py checks the oracles themselves (preconditions, sensitivity to
seeded mistakes, an independent torch yardstick).

mix_images is the exact mix of the exactly normalised pixels; the GPU kernel blends the two
unmixed bf16 values (mix_layout on the unmixed kernel's output is its value before the one rounding).
On the integer lattice of the GPU tests the two coincide (0..255 are bf16 numbers).

A plan is (partner int [N], blend [N], box int [N, 4] = y0, x0, y1, x1 half open, wlab [N]).
Layouts: (S, CQ) = (1, 8) plain NHWC with 8 channel slots, (2, 4) the 2x2 space-to-depth stem input,
(4, 3) TResNet's 4x4; output [N, H/S, W/S, S*S*CQ] with channel (py*S + px)*CQ + c.

``bug`` seeds one mistake into an oracle (the sensitivity tests): "shift" the box moved by one pixel,
"block" the box edge decided per SxS output block instead of per source pixel, "swap" blend and
1 - blend exchanged, "wlab" the own label's weight applied to the partner's label.
"""
import torch

F64 = torch.float64
LAYOUTS = {"plain": (1, 8), "s2d2": (2, 4), "s2d4": (4, 3)}


def f64(t):
    return torch.as_tensor(t).detach().to("cpu").to(F64)


def normalised(src, nchw, in_scale, mean, std, cq):
    """(src * in_scale - mean) / std in fp64 -> [N, H, W, cq], zero in the channel slots past C."""
    x = f64(src)
    if nchw:
        x = x.permute(0, 2, 3, 1)
    N, H, W, C = x.shape
    x = x * float(in_scale)
    if mean is not None:
        x = x - f64(mean)
    if std is not None:
        x = x / f64(std)
    out = torch.zeros(N, H, W, cq, dtype=F64)
    out[..., :C] = x
    return out


def to_layout(x, S):
    """[N, H, W, CQ] -> [N, H/S, W/S, S*S*CQ], channel (py*S + px)*CQ + c."""
    N, H, W, CQ = x.shape
    return x.reshape(N, H // S, S, W // S, S, CQ).permute(0, 1, 3, 2, 4, 5).reshape(N, H // S, W // S, S * S * CQ)


def inside(box, N, H, W, S=1, bug=None):
    """bool [N, H, W]: source pixel (y, x) of image n lies in box[n]."""
    b = torch.as_tensor(box).detach().cpu().long().reshape(N, 4)
    if bug == "shift":
        b = b + torch.tensor([0, 1, 0, 1])
    ys = torch.arange(H).view(1, H, 1)
    xs = torch.arange(W).view(1, 1, W)
    if bug == "block":  # the whole SxS block follows its top-left pixel
        ys, xs = ys // S * S, xs // S * S
    y0, x0, y1, x1 = (b[:, k].view(N, 1, 1) for k in range(4))
    return (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)


def mix_pixels(a, plan, S=1, bug=None):
    """Mix [N, H, W, CQ] fp64 rows by the plan: the partner's pixel inside the box, elsewhere
    blend * own + (1 - blend) * partner."""
    partner, blend, box = plan[0], plan[1], plan[2]
    N, H, W, _ = a.shape
    p = torch.as_tensor(partner).detach().cpu().long()
    assert int(p.min()) >= 0 and int(p.max()) < N, "the oracle takes valid plans only"
    b = a[p]
    bl = f64(blend).view(N, 1, 1, 1)
    if bug == "swap":
        bl = 1.0 - bl
    out = bl * a + (1.0 - bl) * b
    return torch.where(inside(box, N, H, W, S, bug).unsqueeze(-1), b, out)


def mix_images(src, nchw, in_scale, mean, std, plan, layout="plain", bug=None):
    """The mixed input kernel's exact value in fp64 -> [N, H/S, W/S, S*S*CQ]."""
    S, cq = LAYOUTS[layout]
    return to_layout(mix_pixels(normalised(src, nchw, in_scale, mean, std, cq), plan, S, bug), S)


def mix_layout(A, plan, H, W, layout):
    """The plan applied to rows already in their output layout (the unmixed kernel's bf16 output
    [N, H/S, W/S, S*S*CQ]) in fp64: what the mixed kernel rounds once to bf16."""
    partner, blend, box = plan[0], plan[1], plan[2]
    A = f64(A)
    N = A.shape[0]
    B = A[torch.as_tensor(partner).detach().cpu().long()]
    bl = f64(blend).view(N, 1, 1, 1)
    return torch.where(inside_layout(box, N, H, W, layout), B, bl * A + (1.0 - bl) * B)


def inside_layout(box, N, H, W, layout):
    """bool [N, H/S, W/S, S*S*CQ]: the output element comes from a source pixel inside box[n]."""
    S, cq = LAYOUTS[layout]
    m = inside(box, N, H, W).unsqueeze(-1).expand(N, H, W, cq)
    return to_layout(m, S)


# ----------------------------------------------------------------------------- two-label cross-entropy
def label_pair(labels, partner, C):
    a = torch.as_tensor(labels).detach().cpu().long().view(-1)
    p = torch.as_tensor(partner).detach().cpu().long().view(-1)
    b2 = a[p]
    va, vb = (a >= 0) & (a < C), (b2 >= 0) & (b2 < C)
    return a, b2, va, vb


def xent_mix_rows(x, labels, partner, wlab, C, smoothing=0.0, bug=None):
    """Rows of the two-label loss over the first C columns of x:
    l = w (lse - x_a) + (1 - w) (lse - x_b2), smoothing s: (1 - s) l + s (lse - mean x); 0 on a row
    with a label outside [0, C).  rank = #{j : x_j > x_a} (meaningful where the own label is valid).
    ``smoothing`` is taken as given: the caller rounds it to fp32 the way the kernel receives it."""
    x = f64(x)[:, :C]
    a, b2, va, vb = label_pair(labels, partner, C)
    w = f64(wlab)
    if bug == "wlab":
        w = 1.0 - w
    sa, sb = a.clamp(0, max(C - 1, 0)), b2.clamp(0, max(C - 1, 0))
    xa = x.gather(1, sa[:, None]).squeeze(1)
    xb = x.gather(1, sb[:, None]).squeeze(1)
    lse = torch.logsumexp(x, 1)
    loss = w * (lse - xa) + (1.0 - w) * (lse - xb)
    if smoothing > 0:
        loss = (1.0 - smoothing) * loss + smoothing * (lse - x.mean(1))
    valid = va & vb
    return {"loss": torch.where(valid, loss, torch.zeros_like(loss)), "rank": (x > xa[:, None]).sum(1),
            "valid": valid, "own_valid": va, "p": torch.exp(x - lse[:, None]), "absmax": x.abs().amax(1)}


def xent_mix_targets(labels, partner, wlab, C, smoothing=0.0, bug=None):
    """t_j = (1 - s) (w [j == a] + (1 - w) [j == b2]) + s / C -> [B, C] (rows with both labels valid)."""
    a, b2, va, vb = label_pair(labels, partner, C)
    w = f64(wlab)
    if bug == "wlab":
        w = 1.0 - w
    B = a.numel()
    t = torch.full((B, C), smoothing / C, dtype=F64)
    t.scatter_add_(1, a.clamp(0, max(C - 1, 0))[:, None], ((1.0 - smoothing) * w)[:, None])
    t.scatter_add_(1, b2.clamp(0, max(C - 1, 0))[:, None], ((1.0 - smoothing) * (1.0 - w))[:, None])
    return t


def xent_mix_grad(x, labels, partner, wlab, C, g, smoothing=0.0, bug=None):
    """d/dx of g * sum_rows(loss) -> [B, C]; rows with an invalid label are zero."""
    r = xent_mix_rows(x, labels, partner, wlab, C, smoothing)
    t = xent_mix_targets(labels, partner, wlab, C, smoothing, bug)
    return float(g) * (r["p"] - t) * r["valid"][:, None].to(F64)
