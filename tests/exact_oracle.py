"""Integer-lattice oracle for the MFMA conv / GEMM kernels (helper module, not collected).

With small-integer bf16 inputs every product and every partial sum of a convolution is an integer
below 2^24, so an fp32 accumulation is exact in ANY order: tile shape, k order, split-K, stream-K,
ping-pong and the stride-2 parity classes cannot change the result.  The only correct output is the
exact integer sum rounded ONCE to the output type, and the comparison is ``torch.equal``.

``lattice``        seeded i.i.d. integer-valued bf16 tensors
``exact_*``        fp64 CPU references (NHWC activations, [Co,KH,KW,Ci] weights, as the kernels)
``check_lattice``  the preconditions, asserted on the reference alone
``assert_exact``   ``torch.equal`` with a report that shows tile-tail / vector-tail patterns
``*_problem``      the cached (inputs, exact result) of one shape, shared by the CPU and GPU tests
``*_shapes``       the shape lists, taken from tests/test_kernels_gpu.py's own parametrisations
"""
from __future__ import annotations

import functools
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

TWO24 = float(1 << 24)
BF16, F32 = torch.bfloat16, torch.float32


# ----------------------------------------------------------------------------- lattice inputs
def lattice(shape, lo, hi, seed):
    """Integer-valued bf16 tensor, i.i.d. uniform on [lo, hi] from a seeded generator (|v| <= 256:
    every value is a bf16 number)."""
    assert -256 <= lo <= hi <= 256
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(BF16)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _var(m):  # variance of the uniform integers on [-m, m]
    return m * (m + 1) / 3.0


_RANGES = [(3, 3), (7, 3), (7, 7), (15, 7), (15, 15), (31, 15), (31, 31), (63, 31), (63, 63), (127, 63), (127, 127)]


def pick_ranges(k_eff):
    """(max|a|, max|b|) for a sum of ``k_eff`` products: the narrowest pair whose sums have a
    standard deviation of >= 700, i.e. most outputs beyond 256, where bf16 stops holding every
    integer -- wide for short K (1x1 on 64 channels, grouped convs), narrow for K = 4608."""
    for ma, mb in _RANGES:
        if k_eff * _var(ma) * _var(mb) >= 700.0 ** 2:
            return ma, mb
    return _RANGES[-1]


# ----------------------------------------------------------------------------- bf16 bit helpers
def _bits(exact):
    """int32 bit pattern of the fp32 image of an fp64 tensor that fp32 holds exactly."""
    f = exact.float()
    assert torch.equal(f.double(), exact.double()), "exact value not an fp32 number"
    return f.contiguous().view(torch.int32)


def bf16_representable(t):
    return (_bits(t.double()) & 0xFFFF) == 0


def bf16_tie(t):
    """exactly halfway between two neighbouring bf16 numbers: the rounding mode decides"""
    return (_bits(t.double()) & 0xFFFF) == 0x8000


def bf16_trunc(t):
    """round-toward-zero store (the defect a wrong conversion makes)"""
    return (_bits(t.double()) & ~0xFFFF).view(torch.float32).to(BF16)


def bf16_ulp(t):
    """spacing of the bf16 numbers at |t| (fp64 tensor)"""
    a = t.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def rounded(exact, dtype):
    """the one correct output: the exact value rounded once (fp32 holds every lattice sum)"""
    f = exact.float()
    assert torch.equal(f.double(), exact.double()), "exact value not an fp32 number"
    return f.to(BF16) if dtype == BF16 else f


# ----------------------------------------------------------------------------- exact references
def _nchw(x):
    return x.double().permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _oihw(w):
    return w.double().permute(0, 3, 1, 2)


def exact_conv_fwd(x, w, stride, pad, groups=1):
    return _nhwc(F.conv2d(_nchw(x), _oihw(w), stride=stride, padding=pad, groups=groups))


def _pad_geo(xc, KH, KW, stride, pad, Ho, Wo):
    H, W = xc.shape[2], xc.shape[3]
    Hp, Wp = (Ho - 1) * stride + KH, (Wo - 1) * stride + KW
    xc = F.pad(xc, (pad, max(0, Wp - pad - W), pad, max(0, Hp - pad - H)))
    return xc[:, :, :Hp, :Wp]


def exact_conv_fwd_geo(x, w, stride, pad, Ho, Wo):
    """explicit output grid: pad top / left, pad or crop bottom / right (the s2d stem geometry)"""
    xc = _pad_geo(_nchw(x), w.shape[1], w.shape[2], stride, pad, Ho, Wo)
    return _nhwc(F.conv2d(xc, _oihw(w), stride=stride))


def exact_conv_dgrad(dy, w, H, W, stride, pad, add=None, groups=1):
    """w: [Co,KH,KW,Ci/groups]; add: an integer tensor summed BEFORE the one rounding"""
    N = dy.shape[0]
    C = w.shape[3] * groups
    dx = torch.nn.grad.conv2d_input((N, C, H, W), _oihw(w), _nchw(dy), stride=stride, padding=pad, groups=groups)
    dx = _nhwc(dx)
    return dx if add is None else dx + add.double()


def exact_conv_wgrad(dy, x, KH, KW, stride, pad, groups=1):
    Co, C = dy.shape[3], x.shape[3]
    dw = torch.nn.grad.conv2d_weight(_nchw(x), (Co, C // groups, KH, KW), _nchw(dy), stride=stride, padding=pad,
                                     groups=groups)
    return dw.permute(0, 2, 3, 1).contiguous()


def exact_conv_wgrad_geo(dy, x, KH, KW, stride, pad):
    Co, C, Ho, Wo = dy.shape[3], x.shape[3], dy.shape[1], dy.shape[2]
    xc = _pad_geo(_nchw(x), KH, KW, stride, pad, Ho, Wo)
    dw = torch.nn.grad.conv2d_weight(xc, (Co, C, KH, KW), _nchw(dy), stride=stride)
    return dw.permute(0, 2, 3, 1).contiguous()


def exact_linear(x, w, bias=None, relu=False, width=None):
    """x [B,K], w [N,K] -> [B,width]; columns past N are exactly 0 (zero weight rows, no bias)"""
    y = x.double() @ w.double().t()
    if bias is not None:
        y[:, : bias.numel()] += bias.double()
    if relu:
        y = torch.relu(y)
    if width is not None and width > y.shape[1]:
        y = F.pad(y, (0, width - y.shape[1]))
    return y


def exact_act(z, act, slope):
    if act == 1:
        return torch.relu(z)
    if act == 2:
        return torch.where(z >= 0, z, z * slope)
    return z


def exact_affine(conv, scale, shift, act, slope, res=None):
    """act(conv * scale + shift [+ res]) of the EXACT conv, per output channel"""
    z = conv.double() * scale.double() + shift.double()
    if res is not None:
        z = z + res.double()
    return exact_act(z, act, slope)


def exact_prologue(x, scale, shift):
    """bf16(relu(x * scale + shift)): the operand the BN-prologue kernels feed to the MFMAs"""
    a = torch.relu(x.double() * scale.double() + shift.double())
    return rounded(a, BF16).double()


# ----------------------------------------------------------------------------- preconditions
def _is_pow2(t):
    t = torch.as_tensor(t, dtype=torch.float64).abs()
    m, _ = torch.frexp(t)
    return bool(((t > 0) & (m == 0.5)).all())


def _is_int(t):
    t = torch.as_tensor(t, dtype=torch.float64)
    return bool((t == t.round()).all())


def lattice_shares(exact):
    """(share of exact values bf16 cannot hold, share of exact ties)"""
    n = exact.numel()
    return (~bf16_representable(exact)).sum().item() / n, bf16_tie(exact).sum().item() / n


def check_lattice(a, b, k_total, exact, out_dtype, *, scale=None, shift=None, res=None, bias=None, slope=None,
                  min_norep=0.05, min_ties=0.01):
    """The lattice preconditions, asserted on the reference alone (before any GPU result is looked at).

    ``a`` / ``b``: the two MFMA operands (for the prologue form ``a`` is the operand AFTER scale and
    shift).  ``k_total``: products per output -- taps x channels (forward, dgrad), N*Ho*Wo (weight
    gradients).  k_total * max|a| * max|b| < 2^24 makes every partial sum, in any order, an integer
    fp32 holds: a condition, not a tolerance.  With an affine epilogue the bound applies after scale
    and shift, in units of the finest power of two involved."""
    for t in (a, b, res):
        if t is not None:
            f = t.double()
            assert torch.equal(f.float().to(BF16).double(), f), "input not bf16-representable"
    assert _is_int(a) and _is_int(b), "operands must be integers"
    bound = float(k_total) * a.double().abs().max().item() * b.double().abs().max().item()
    unit = 1.0
    if scale is not None:
        assert _is_pow2(scale), "scales must be signed powers of two"
        assert _is_int(shift), "shifts must be integers"
        bound = bound * scale.double().abs().max().item() + shift.double().abs().max().item()
        unit = min(unit, scale.double().abs().min().item())
    if res is not None:
        assert _is_int(res), "residual / add must be integers"
        bound += res.double().abs().max().item()
    if bias is not None:
        assert _is_int(bias), "bias must be integers"
        bound += bias.double().abs().max().item()
    if slope is not None:
        assert _is_pow2(slope), "leaky slope must be a power of two"
        unit *= min(1.0, float(slope))
    assert bound / unit < TWO24, f"partial sums may leave the fp32 integers: {bound / unit:.3g} >= 2^24"
    assert exact.double().abs().max().item() / unit < TWO24
    assert torch.equal(exact.float().double(), exact.double()), "exact result is not an fp32 number"
    if out_dtype == BF16:
        norep, ties = lattice_shares(exact)
        assert norep >= min_norep, f"only {norep:.1%} of the exact values need rounding (want >= {min_norep:.0%})"
        assert ties >= min_ties, f"only {ties:.1%} of the exact values are ties (want >= {min_ties:.0%})"
    return bound / unit


# ----------------------------------------------------------------------------- comparison
def mismatch_report(got, want, dims=None, limit=10):
    got, want = got.detach().cpu(), want.detach().cpu()
    g, w = got.double(), want.double()
    bad = (g != w) | (torch.isnan(g) != torch.isnan(w))
    idx = bad.nonzero()
    names = tuple(dims) if dims else tuple(f"d{i}" for i in range(got.dim()))
    lines = [f"{idx.shape[0]} of {got.numel()} elements differ (shape {tuple(got.shape)}, dims {names}); "
             f"largest |got - want| = {(g - w)[bad].abs().max().item():g}"]
    for i in idx[:limit].tolist():
        lines.append(f"  {dict(zip(names, i))}: got {g[tuple(i)].item():g} want {w[tuple(i)].item():g}")
    C = got.shape[-1]
    flat = bad.reshape(-1, C).nonzero()
    row, ch = flat[:, 0], flat[:, 1]

    def hist(v, m):
        c = torch.bincount(v % m, minlength=m)
        top = torch.argsort(c, descending=True)[:8]
        return ", ".join(f"{int(k)}:{int(c[k])}" for k in top if c[k] > 0)

    lines.append(f"  by output row mod 128: {hist(row, 128)}")
    lines.append(f"  by output row mod 256: {hist(row, 256)}")
    lines.append(f"  by channel mod 8:      {hist(ch, 8)}")
    lines.append(f"  by channel mod 64:     {hist(ch, 64)}")
    return "\n".join(lines)


def assert_exact(got, want, dims=None, what=""):
    """Passes only on ``torch.equal``; the failure names where the mismatches sit."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} vs {want.dtype}"
    if got.device != want.device:
        want = want.to(got.device)
    if torch.equal(got, want):
        return
    raise AssertionError(f"{what}: not bit-exact\n" + mismatch_report(got, want, dims))


NHWC = ("n", "h", "w", "c")
OHWI = ("co", "kh", "kw", "ci")


# ----------------------------------------------------------------------------- shape lists
def _tk():
    from tests import test_kernels_gpu as TK  # the shape lists live there; imported, never copied
    return TK


def params_of(test_fn, argnames):
    """argvalues of ``test_fn``'s ``pytest.mark.parametrize(argnames, ...)``"""
    want = [a.strip() for a in argnames.split(",")]
    for m in getattr(test_fn, "pytestmark", []):
        if m.name == "parametrize":
            have = m.args[0]
            have = [a.strip() for a in have.split(",")] if isinstance(have, str) else list(have)
            if have == want:
                return [tuple(v) if isinstance(v, (tuple, list)) else v for v in m.args[1]]
    raise LookupError(f"{test_fn.__name__} has no parametrize({argnames!r})")


def conv_shapes():
    return list(_tk().CONV_SHAPES)


def dgrad_shapes():
    tk = _tk()
    return params_of(tk.test_conv_dgrad, "shape")


def pipeline_shapes():
    return params_of(_tk().test_conv_pipeline_variants, "shape")


def big_tile_shapes():
    return params_of(_tk().test_big_tile_tap_gemm_matches, "shape")


def stream_k_shapes():
    return params_of(_tk().test_big_tile_stream_k_matches, "shape")


def split_k_shapes():
    return [(N, H, H, Ci, Co, k, s, p)
            for N, H, Ci, Co, k, s, p in params_of(_tk().test_split_k_short_grids, "N,H,Ci,Co,k,s,p")]


def ws_shapes():
    return [(N, H, W, Ci, Co, 1, 1, 0) for N, H, W, Ci, Co in _tk().WS_SHAPES]


def tile256_shapes():
    return params_of(_tk().test_conv_fwd_256_channel_tiles, "shape")


def c3_shapes():
    return [(N, H, W, 64, 64, 3, 1, 1) for N, H, W in params_of(_tk().test_conv3x3_direct_c64, "N,H,W")]


def parity_stream_shapes():
    return [(N, H, W, Ci, Co, k, 2, k // 2)
            for N, H, W, Ci, Co, k in params_of(_tk().test_conv_dgrad_stride2_parity_streams, "shape")]


def wgrad_variant_shapes():
    return params_of(_tk().test_conv_wgrad_variants, "shape")


def wgrad_variant_cfgs():
    return params_of(_tk().test_conv_wgrad_variants, "cfg")


def wgrad3x3_shapes():
    return [(N, H, W, Ci, Co, 3, 1, 1) for N, H, W, Ci, Co in params_of(_tk().test_wgrad3x3_direct, "N,H,W,Ci,Co")]


def affine_shapes():
    return params_of(_tk().test_conv_fwd_affine_folded_bn, "shape")


def pro_shapes():
    return params_of(_tk().test_conv_bn_prologue, "shape")  # N, H, W, C, Co (1x1)


def pro3x3_shapes():
    return params_of(_tk().test_conv3x3_bn_prologue, "N,H,W")


def stem_shapes():
    return params_of(_tk().test_stem_fwd, "N,H,W")


def geo_shapes():
    return params_of(_tk().test_conv_geo, "N,H,Ci,Co,k,pad")


def grouped_shapes():
    return params_of(_tk().test_grouped_conv_shapes, "N,H,W,C,G,KH,stride,pad")


def linear_shapes():
    """(B, K, N, width): test_linear's three, and the 1000-way head on the 1024-wide padded GEMM"""
    return [(B, K_, N, N) for B, K_, N, _, _ in params_of(_tk().test_linear, "B,K_,N,relu,bias")] + [(64, 512, 1000, 1024)]


def uniq(seq):
    out = []
    for s in seq:
        if s not in out:
            out.append(s)
    return out


def all_fwd_shapes():
    return uniq(conv_shapes() + pipeline_shapes() + big_tile_shapes() + stream_k_shapes() + split_k_shapes() +
                 ws_shapes() + tile256_shapes() + c3_shapes() + affine_shapes())


def all_dgrad_shapes():
    return uniq(dgrad_shapes() + pipeline_shapes() + big_tile_shapes() + stream_k_shapes() +
                 [s for s in split_k_shapes() if s[6] == 1] + parity_stream_shapes() + c3_shapes())


def all_wgrad_shapes():
    return uniq(conv_shapes() + wgrad_variant_shapes() + wgrad3x3_shapes())


# ----------------------------------------------------------------------------- cached problems
def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def fwd_problem(shape):
    """forward conv on the lattice: x, w, the exact y and its one-rounding bf16 image"""
    N, H, W, Ci, Co, k, s, p = shape
    K = k * k * Ci
    mx, mw = pick_ranges(K)
    x = lattice((N, H, W, Ci), -mx, mx, _seed("fx", shape))
    w = lattice((Co, k, k, Ci), -mw, mw, _seed("fw", shape))
    exact = exact_conv_fwd(x, w, s, p)
    return SimpleNamespace(shape=shape, x=x, w=w, K=K, exact=exact, want=rounded(exact, BF16), ranges=(mx, mw))


@functools.lru_cache(maxsize=None)
def dgrad_problem(shape):
    """data gradient on the lattice, without and with an integer add (summed before the rounding)"""
    N, H, W, Ci, Co, k, s, p = shape
    Ho, Wo = _out_hw(H, W, k, s, p)
    K = k * k * Co
    mdy, mw = pick_ranges(max(1, K // (s * s)))  # a stride-2 pixel sees a quarter of the taps
    dy = lattice((N, Ho, Wo, Co), -mdy, mdy, _seed("dy", shape))
    w = lattice((Co, k, k, Ci), -mw, mw, _seed("dw", shape))
    add = lattice((N, H, W, Ci), -100, 100, _seed("da", shape))
    exact = exact_conv_dgrad(dy, w, H, W, s, p)
    return SimpleNamespace(shape=shape, dy=dy, w=w, add=add, K=K, exact=exact, want=rounded(exact, BF16),
                           exact_add=exact + add.double(), want_add=rounded(exact + add.double(), BF16),
                           ranges=(mdy, mw))


@functools.lru_cache(maxsize=None)
def wgrad_problem(shape):
    """weight gradient on the lattice: fp32 output, exact"""
    N, H, W, Ci, Co, k, s, p = shape
    Ho, Wo = _out_hw(H, W, k, s, p)
    dy = lattice((N, Ho, Wo, Co), -7, 7, _seed("wdy", shape))
    x = lattice((N, H, W, Ci), -7, 7, _seed("wx", shape))
    exact = exact_conv_wgrad(dy, x, k, k, s, p)
    return SimpleNamespace(shape=shape, dy=dy, x=x, K=N * Ho * Wo, exact=exact, want=rounded(exact, F32))


def pow2_scales(C, seed, exps=(-1, 0, 1)):
    g = torch.Generator().manual_seed(int(seed))
    e = torch.tensor(exps, dtype=torch.float32)[torch.randint(0, len(exps), (C,), generator=g)]
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    return sign * torch.exp2(e)


def int_vector(C, lo, hi, seed):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, (C,), generator=g).float()


LEAKY_SLOPE = 0.125


@functools.lru_cache(maxsize=None)
def affine_problem(shape):
    """conv + per-channel power-of-two scale + integer shift [+ integer residual] + act"""
    f = fwd_problem(shape)
    Co = shape[4]
    scale = pow2_scales(Co, _seed("as", shape))
    shift = int_vector(Co, -64, 64, _seed("ah", shape))
    res = lattice(f.exact.shape, -100, 100, _seed("ar", shape))
    return SimpleNamespace(f=f, scale=scale, shift=shift, res=res)


@functools.lru_cache(maxsize=None)
def pro_problem(shape):
    """1x1 conv / weight gradient of a = bf16(relu(x * scale + shift)), scale a power of two"""
    N, H, W, C, Co = shape
    mx, mw = pick_ranges(C // 2)  # about half of the operands survive the ReLU
    x = lattice((N, H, W, C), -mx, mx, _seed("px", shape))
    w = lattice((Co, 1, 1, C), -mw, mw, _seed("pw", shape))
    scale = pow2_scales(C, _seed("ps", shape), exps=(0, 1))
    shift = int_vector(C, -3, 3, _seed("ph", shape))
    a = exact_prologue(x, scale, shift)
    exact = exact_conv_fwd(a, w, 1, 0)
    dy = lattice((N, H, W, Co), -7, 7, _seed("pdy", shape))
    dw = exact_conv_wgrad(dy, a, 1, 1, 1, 0)
    return SimpleNamespace(shape=shape, x=x, w=w, scale=scale, shift=shift, a=a, K=C, exact=exact,
                           want=rounded(exact, BF16), dy=dy, Kw=N * H * W, exact_dw=dw, want_dw=rounded(dw, F32))


@functools.lru_cache(maxsize=None)
def pro3x3_problem(shape):
    """64-channel 3x3 of a = bf16(relu(x * scale + shift)); the zero padding is of a, not of x"""
    N, H, W = shape
    C = 64
    mx, mw = pick_ranges(9 * C // 2)
    x = lattice((N, H, W, C), -mx, mx, _seed("qx", shape))
    w = lattice((C, 3, 3, C), -mw, mw, _seed("qw", shape))
    scale = pow2_scales(C, _seed("qs", shape), exps=(0, 1))
    shift = int_vector(C, -3, 3, _seed("qh", shape))
    a = exact_prologue(x, scale, shift)
    exact = exact_conv_fwd(a, w, 1, 1)
    dy = lattice((N, H, W, C), -7, 7, _seed("qdy", shape))
    dw = exact_conv_wgrad(dy, a, 3, 3, 1, 1)
    return SimpleNamespace(shape=shape, x=x, w=w, scale=scale, shift=shift, a=a, K=9 * C, exact=exact,
                           want=rounded(exact, BF16), dy=dy, Kw=N * H * W, exact_dw=dw, want_dw=rounded(dw, F32))


@functools.lru_cache(maxsize=None)
def geo_problem(shape):
    """explicit-grid conv (output grid = input grid, pad top / left) and its weight gradient"""
    N, H, W, Ci, Co, k, pad = shape
    K = k * k * Ci
    mx, mw = pick_ranges(K)
    x = lattice((N, H, W, Ci), -mx, mx, _seed("gx", shape))
    w = lattice((Co, k, k, Ci), -mw, mw, _seed("gw", shape))
    exact = exact_conv_fwd_geo(x, w, 1, pad, H, W)
    dy = lattice((N, H, W, Co), -7, 7, _seed("gdy", shape))
    x7 = lattice((N, H, W, Ci), -7, 7, _seed("gx7", shape))
    dw = exact_conv_wgrad_geo(dy, x7, k, k, 1, pad)
    return SimpleNamespace(shape=shape, x=x, w=w, K=K, exact=exact, want=rounded(exact, BF16), dy=dy, x7=x7,
                           Kw=N * H * W, exact_dw=dw, want_dw=rounded(dw, F32))


def stem_problem(shape):
    N, H, W = shape
    return geo_problem((N, H, W, 16, 64, 4, 2))


@functools.lru_cache(maxsize=None)
def grouped_problem(shape):
    N, H, W, C, G, KH, s, p = shape
    CG = C // G
    Ho, Wo = _out_hw(H, W, KH, s, p)
    K = KH * KH * CG
    mx, mw = pick_ranges(K)
    x = lattice((N, H, W, C), -mx, mx, _seed("Gx", shape))
    w = lattice((C, KH, KH, CG), -mw, mw, _seed("Gw", shape))
    y = exact_conv_fwd(x, w, s, p, groups=G)
    mdy, mwd = pick_ranges(max(1, K // (s * s)))
    dy = lattice((N, Ho, Wo, C), -mdy, mdy, _seed("Gdy", shape))
    wd = lattice((C, KH, KH, CG), -mwd, mwd, _seed("Gwd", shape))
    dx = exact_conv_dgrad(dy, wd, H, W, s, p, groups=G)
    dy7 = lattice((N, Ho, Wo, C), -7, 7, _seed("Gdy7", shape))
    x7 = lattice((N, H, W, C), -7, 7, _seed("Gx7", shape))
    dw = exact_conv_wgrad(dy7, x7, KH, KH, s, p, groups=G)
    return SimpleNamespace(shape=shape, x=x, w=w, K=K, exact=y, want=rounded(y, BF16),
                           dy=dy, wd=wd, exact_dx=dx, want_dx=rounded(dx, BF16),
                           dy7=dy7, x7=x7, Kw=N * Ho * Wo, exact_dw=dw, want_dw=rounded(dw, F32))


@functools.lru_cache(maxsize=None)
def linear_problem(shape):
    """y = x w^T + integer bias (ReLU on / off) on a GEMM ``width`` wide, dx = dy w, dw = dy^T x"""
    B, K_, N, width = shape
    mx, mw = pick_ranges(K_)
    x = lattice((B, K_), -mx, mx, _seed("lx", shape))
    w = lattice((N, K_), -mw, mw, _seed("lw", shape))
    bias = int_vector(N, -200, 200, _seed("lb", shape))
    mdy, mwd = pick_ranges(N)
    dy = lattice((B, width), -mdy, mdy, _seed("ldy", shape))
    wd = lattice((N, K_), -mwd, mwd, _seed("lwd", shape))
    dx = dy[:, :N].double() @ wd.double()
    dy7 = lattice((B, width), -7, 7, _seed("ldy7", shape))
    x7 = lattice((B, K_), -7, 7, _seed("lx7", shape))
    dw = dy7.double().t() @ x7.double()
    out = SimpleNamespace(shape=shape, x=x, w=w, bias=bias, K=K_, dy=dy, wd=wd, Kd=N, exact_dx=dx,
                          want_dx=rounded(dx, BF16), dy7=dy7, x7=x7, Kw=B, exact_dw=dw, want_dw=rounded(dw, F32))
    out.exact = {(b, r): exact_linear(x, w, bias if b else None, r, width) for b in (False, True) for r in (False, True)}
    out.want = {k: rounded(v, BF16) for k, v in out.exact.items()}
    return out
