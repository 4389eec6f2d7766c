"""Plain-PyTorch (NCHW, fp32, autograd) rendering of our NHWC ResNet using the
SAME parameter tensors — the oracle for end-to-end model parity tests.

The rendering comes in segments (stem, one residual block, head) so that a check can run ONE
segment in fp64 on the tensors the model under test itself produced ("teacher forcing",
:func:`teacher_forced_errors`): the error of a segment's gradients is then that segment's own,
not the amplified rounding of everything below it.  ``round_to=torch.bfloat16`` turns a segment
into the yardstick of that check, the fp64 reference with bf16 storage: the conv / fc weights and
every conv, BN, pool and fc output pass through ``x.to(round_to).to(x.dtype)``, whose autograd
rounds the matching gradients as well.  No project code takes part in it."""
import torch
import torch.nn.functional as F

from ddp_classification_pytorch_amd.models.resnet import BasicBlock, Bottleneck


def _rnd(x, round_to):
    return x if round_to is None else x.to(round_to).to(x.dtype)


def _conv(x, conv, round_to=None):
    w = _rnd(conv.weight.permute(0, 3, 1, 2), round_to)
    return _rnd(F.conv2d(x, w, stride=conv.stride, padding=conv.padding, groups=conv.groups), round_to)


def _bn(x, bn, training, round_to=None):
    rm = bn.running_mean.clone()
    rv = bn.running_var.clone()
    y = F.batch_norm(x, rm, rv, bn.weight, bn.bias, training=training, momentum=bn.momentum, eps=bn.eps)
    return _rnd(y, round_to)


def stem_forward(model, x_nchw, training=True, round_to=None, relu=F.relu):
    y = relu(_bn(_conv(x_nchw, model.conv1, round_to), model.bn1, training, round_to))
    if model.variant == "imagenet":
        y = F.max_pool2d(y, 3, 2, 1)
    return y


def block_forward(blk, y, training=True, round_to=None, relu=F.relu):
    r = y
    if blk.downsample is not None:
        r = _bn(_conv(y, blk.downsample[0], round_to), blk.downsample[1], training, round_to)
    if isinstance(blk, Bottleneck):
        z = relu(_bn(_conv(y, blk.conv1, round_to), blk.bn1, training, round_to))
        z = relu(_bn(_conv(z, blk.conv2, round_to), blk.bn2, training, round_to))
        z = _bn(_conv(z, blk.conv3, round_to), blk.bn3, training, round_to)
    else:
        z = relu(_bn(_conv(y, blk.conv1, round_to), blk.bn1, training, round_to))
        z = _bn(_conv(z, blk.conv2, round_to), blk.bn2, training, round_to)
    return relu(z + r)


def head_forward(model, y, round_to=None):
    f = _rnd(y.mean((2, 3)), round_to)
    if model.fc is None:
        return f
    return _rnd(F.linear(f, _rnd(model.fc.weight, round_to), model.fc.bias), round_to)


def named_blocks(model):
    """[(name, block)] of the residual blocks in forward order ("layer1.0", ...)."""
    return [(f"layer{i}.{j}", blk) for i in (1, 2, 3, 4) for j, blk in enumerate(getattr(model, f"layer{i}"))]


def mirror_forward(model, x_nchw, training=True, round_to=None):
    y = stem_forward(model, x_nchw, training, round_to)
    for _, blk in named_blocks(model):
        y = block_forward(blk, y, training, round_to)
    return head_forward(model, y, round_to)


def frozen_copy(m, seed=3):
    """Non-trivial running statistics / affine, BN frozen (NESTED freeze_bn: eval + no affine grad)."""
    from ddp_classification_pytorch_amd.models.layers import BatchNorm2d

    g = torch.Generator().manual_seed(seed)
    for mod in m.modules():
        if isinstance(mod, BatchNorm2d):
            C = mod.num_features
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(C, generator=g) * 0.5 + 0.75)
                mod.weight.copy_(torch.rand(C, generator=g) * 0.5 + 0.5)
                mod.bias.copy_(torch.randn(C, generator=g) * 0.1)
            mod.eval()
            mod.weight.requires_grad_(False)
            mod.bias.requires_grad_(False)
    return m


# ----------------------------------------------------------------------------- teacher forcing
def rel_l2(a, b):
    """|a - b| / |b| in fp64 on the CPU."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def image_of_input(model, x):
    """The model's input tensor (NHWC with the image channels zero-padded, or the s2d stem's
    [N, H/2, W/2, 16]: channel (py * 2 + px) * 4 + c) -> the fp64 NCHW image, image channels only."""
    x = x.detach().double().cpu()
    c = model.in_chans
    if x.shape[-1] == 16 and getattr(model, "stem_s2d", False):
        N, H2, W2, _ = x.shape
        x = x.reshape(N, H2, W2, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H2, 2 * W2, 4)
    return x[..., :c].permute(0, 3, 1, 2).contiguous()


class Captures:
    """What one training step left at the segment boundaries, fp64 NCHW on the CPU:
    ``image``; per block ``x[name]`` (block input), ``dx[name]`` (gradient at the block input) and
    ``dy[name]`` (gradient at the block output); ``y_last`` / ``dy_last`` for the last block's
    output; ``labels``.  ``dx`` of the first block is the stem's output gradient."""

    def __init__(self):
        self.image = self.y_last = self.dy_last = self.labels = None
        self.x, self.dx, self.dy = {}, {}, {}


def capture_step(model, run_step, labels):
    """Runs ``run_step(model)`` (forward, loss, backward) once with cloning hooks at every block
    boundary of the NHWC project model and returns the :class:`Captures`.  The hooks only clone,
    return None and are removed afterwards, so the step computes what it computes without them
    (a tensor hook returning None leaves the gradient buffer in place: the fused BN backward's
    buffer-identity test still sees the consuming conv's buffer)."""
    cap = Captures()
    cap.labels = labels.detach().cpu()
    blocks = named_blocks(model)
    handles = []
    raw = {}

    def grad_hook(key):
        def hook(g):
            raw[key] = g.detach().clone()
            return None
        return hook

    def model_pre(_m, args):
        raw["image"] = args[0].detach().clone()
        return None

    def block_pre(name):
        def hook(_m, args):
            x = args[0]
            raw["x", name] = x.detach().clone()
            if x.requires_grad:
                handles.append(x.register_hook(grad_hook(("dx", name))))
            return None
        return hook

    def last_fwd(_m, _args, out):
        raw["y_last"] = out.detach().clone()
        handles.append(out.register_hook(grad_hook("dy_last")))
        return None

    handles.append(model.register_forward_pre_hook(model_pre))
    for name, blk in blocks:
        handles.append(blk.register_forward_pre_hook(block_pre(name)))
    handles.append(blocks[-1][1].register_forward_hook(last_fwd))
    try:
        run_step(model)
    finally:
        for h in handles:
            h.remove()
    cap.image = image_of_input(model, raw["image"])
    names = [n for n, _ in blocks]
    for n in names:
        cap.x[n] = _nchw64(raw["x", n])
        cap.dx[n] = _nchw64(raw["dx", n])
    cap.y_last, cap.dy_last = _nchw64(raw["y_last"]), _nchw64(raw["dy_last"])
    for n, nxt in zip(names, names[1:]):
        cap.dy[n] = cap.dx[nxt]
    cap.dy[names[-1]] = cap.dy_last
    return cap


def mirror_capture_step(model64, image, labels, training=True, round_to=None):
    """(the same captures, {parameter name: gradient}) from a whole-model training step of the
    (optionally rounding) mirror itself."""
    cap = Captures()
    cap.image, cap.labels = image.detach().double(), labels.detach()
    model64.zero_grad(set_to_none=True)
    bound = []
    y = stem_forward(model64, cap.image, training, round_to)
    for name, blk in named_blocks(model64):
        y.retain_grad()
        bound.append((name, y))
        y = block_forward(blk, y, training, round_to)
    y.retain_grad()
    F.cross_entropy(head_forward(model64, y, round_to), labels).backward()
    for name, t in bound:
        cap.x[name], cap.dx[name] = t.detach().clone(), t.grad.detach().clone()
    cap.y_last, cap.dy_last = y.detach().clone(), y.grad.detach().clone()
    names = [n for n, _ in bound]
    for n, nxt in zip(names, names[1:]):
        cap.dy[n] = cap.dx[nxt]
    cap.dy[names[-1]] = cap.dy_last
    grads = _param_grads(model64)
    model64.zero_grad(set_to_none=True)
    return cap, grads


def _param_grads(mod, prefix=""):
    out = {prefix + n: p.grad.detach().clone() for n, p in mod.named_parameters(recurse=True) if p.grad is not None}
    return out


class _KinkReLU:
    """ReLU for the kink analysis of :func:`segment_grads`: records, per call, the flat indices of
    the pre-activations within ``tol`` (times the tensor's mean magnitude, at least 1) of zero, and
    inverts the mask of the one element ``flip = (call, index)``."""

    def __init__(self, tol, flip=None):
        self.tol, self.flip, self.call, self.found = tol, flip, 0, []

    def __call__(self, z):
        near = z.detach().abs() <= self.tol * z.detach().abs().mean().clamp_min(1.0)
        self.found += [(self.call, int(i)) for i in near.flatten().nonzero().flatten()]
        mask = (z.detach() > 0).contiguous()
        if self.flip is not None and self.flip[0] == self.call:
            mask.view(-1)[self.flip[1]] ^= True
        self.call += 1
        return z * mask.to(z.dtype)


def _with_kinks(run, kink_tol):
    """``run(relu)`` -> {quantity: gradient}.  With ``kink_tol``: adds "_kinks", one
    {quantity: change of the gradient} per pre-activation that lies at the ReLU kink, obtained by
    running the segment again with that one element's mask inverted."""
    if kink_tol is None:
        return run(F.relu)
    probe = _KinkReLU(kink_tol)
    seg = run(probe)
    seg["_kinks"] = []
    for flip in probe.found:
        alt = run(_KinkReLU(kink_tol, flip))
        seg["_kinks"].append({q: alt[q] - g for q, g in seg.items() if q != "_kinks"})
    return seg


def segment_grads(model64, cap, training=True, round_to=None, kink_tol=None):
    """{segment: {quantity: fp64 gradient}} of the mirror run ONE segment at a time on the captured
    tensors: "stem" (conv1.weight, bn1.weight, bn1.bias), each block (its named parameters and the
    masked input gradient ``dx``) and "head" (fc.weight, fc.bias, masked ``dy_last``).  A gradient
    that crosses a block boundary is compared where the activation there is > 0 only: the project
    may hand it over with the producing layer's ReLU mask already applied (BNSource), and the
    mask is idempotent, so feeding a masked gradient to a mirror segment changes nothing.
    ``kink_tol``: see :func:`_with_kinks` and :func:`teacher_forced_errors`."""
    out = {}
    blocks = named_blocks(model64)
    first = blocks[0][0]

    def run_stem(relu):
        model64.zero_grad(set_to_none=True)
        stem_forward(model64, cap.image, training, round_to, relu).backward(cap.dx[first])
        return {**_param_grads(model64.conv1, "conv1."), **_param_grads(model64.bn1, "bn1.")}

    out["stem"] = _with_kinks(run_stem, kink_tol)
    for name, blk in blocks:
        def run_block(relu, name=name, blk=blk):
            blk.zero_grad(set_to_none=True)
            x = cap.x[name].clone().requires_grad_(True)
            block_forward(blk, x, training, round_to, relu).backward(cap.dy[name])
            seg = _param_grads(blk)
            seg["dx"] = x.grad * (cap.x[name] > 0)
            return seg

        out[name] = _with_kinks(run_block, kink_tol)
    model64.zero_grad(set_to_none=True)
    y = cap.y_last.clone().requires_grad_(True)
    F.cross_entropy(head_forward(model64, y, round_to), cap.labels).backward()
    out["head"] = _param_grads(model64.fc, "fc.")
    out["head"]["dy_last"] = y.grad * (cap.y_last > 0)
    model64.zero_grad(set_to_none=True)
    return out


def project_segment_grads(model, cap):
    """The project model's own gradients after the captured step, keyed like :func:`segment_grads`."""
    out = {"stem": {}}
    for pre, mod in (("conv1.", model.conv1), ("bn1.", model.bn1)):
        out["stem"].update(_param_grads(mod, pre))
    for name, blk in named_blocks(model):
        seg = _param_grads(blk)
        seg["dx"] = cap.dx[name] * (cap.x[name] > 0)
        out[name] = seg
    out["head"] = _param_grads(model.fc, "fc.")
    out["head"]["dy_last"] = cap.dy_last * (cap.y_last > 0)
    return out


def _kink_residual(ours, ref, kinks):
    """{quantity: ours - ref}, each less its least-squares projection onto that quantity's gradient
    changes in ``kinks`` (per quantity, so that a real error in one is not spread over the others)."""
    d = {q: ours[q].detach().double().cpu() - g for q, g in ref.items()}
    if kinks:
        for q in d:
            A = torch.stack([k[q].flatten() for k in kinks], 1)
            A = A[:, A.norm(dim=0) > 0]
            if A.shape[1]:
                t = torch.linalg.lstsq(A, d[q].flatten()[:, None], driver="gelsd").solution
                d[q] = d[q] - (A @ t).reshape(d[q].shape)
    return d


def teacher_forced_errors(model, model64, run_step, training=True, labels=None, kink_tol=None):
    """{segment: {quantity: (err_ours, yardstick)}} for one training step of ``model``.

    ``run_step(model)`` does the forward, loss (mean cross-entropy over ``labels``) and backward.
    ``err_ours`` is the relative L2 error of the project's gradient against the fp64 mirror of that
    one segment (``model64``: a ``.double()`` CPU copy of the model before the step) fed the
    tensors captured from the step; ``yardstick`` is the same error of the ``round_to=bfloat16``
    mirror fed the same tensors.

    ``kink_tol`` (for bounds at fp32 rounding level; None for bf16 ones): a pre-activation that
    the fp64 mirror puts within ``kink_tol`` of zero can fall on the other side of the ReLU in
    fp32 arithmetic, and that one flipped mask element moves a block's gradients by ~1e-3 (any
    slope in [0, 1] is a subgradient there, so the reference is a set, not a point).  A few
    million pre-activations per step make such an element likely (expected smallest |z| ~ 2.5e-7).
    With ``kink_tol`` each quantity's error is measured after removing the component of
    ``ours - ref`` along each such element's change of that quantity: a handful of directions out
    of the many a gradient tensor spans."""
    cap = capture_step(model, run_step, labels)
    ours = project_segment_grads(model, cap)
    ref = segment_grads(model64, cap, training, None, kink_tol)
    yard = segment_grads(model64, cap, training, torch.bfloat16)
    errs = {}
    for seg, qs in ref.items():
        kinks = qs.pop("_kinks", [])
        missing = set(qs) - set(ours[seg])
        assert not missing, (seg, missing)
        d = _kink_residual(ours[seg], qs, kinks)
        errs[seg] = {q: (d[q].norm().item() / (g.norm().item() + 1e-300), rel_l2(yard[seg][q], g))
                     for q, g in qs.items()}
    return errs
