"""The integer-lattice oracle (tests/exact_oracle.py) checked on the CPU alone.

* The project's fp32 reference functions (ops/_ref.py, also the CPU path) are exact on lattice
  inputs, for every shape tests/test_exact_lattice_gpu.py uses.
* The preconditions -- the 2^24 bound, the share of outputs that need rounding, the share of exact
  ties -- hold for every (shape, range) pair used there: the CPU-side proof that the reference alone
  stays inside them.
* Sensitivity: defects the norm tolerance of tests/test_kernels_gpu.py lets through are rejected by
  ``assert_exact``.
"""
import pytest
import torch

from ddp_classification_pytorch_amd.ops import _ref
from tests import exact_oracle as X

BF16, F32 = X.BF16, X.F32


def _eq(ref_fp32, exact):
    assert ref_fp32.dtype == torch.float32
    assert torch.equal(ref_fp32.double(), exact)


# ----------------------------------------------------------------------------- reference check + preconditions
@pytest.mark.parametrize("shape", X.all_fwd_shapes(), ids=str)
def test_conv_fwd_reference_and_preconditions(shape):
    N, H, W, Ci, Co, k, s, p = shape
    f = X.fwd_problem(shape)
    X.check_lattice(f.x, f.w, f.K, f.exact, BF16)
    _eq(_ref.conv_fwd(f.x.float(), f.w.float(), s, p, False)[0], f.exact)


@pytest.mark.parametrize("shape", X.all_dgrad_shapes(), ids=str)
def test_conv_dgrad_reference_and_preconditions(shape):
    N, H, W, Ci, Co, k, s, p = shape
    d = X.dgrad_problem(shape)
    X.check_lattice(d.dy, d.w, d.K, d.exact, BF16)
    X.check_lattice(d.dy, d.w, d.K, d.exact_add, BF16, res=d.add)
    wt = d.w.float().permute(3, 1, 2, 0)
    _eq(_ref.conv_dgrad(d.dy.float(), wt, H, W, s, p), d.exact)
    _eq(_ref.conv_dgrad(d.dy.float(), wt, H, W, s, p, d.add.float()), d.exact_add)


@pytest.mark.parametrize("shape", X.all_wgrad_shapes(), ids=str)
def test_conv_wgrad_reference_and_preconditions(shape):
    N, H, W, Ci, Co, k, s, p = shape
    g = X.wgrad_problem(shape)
    X.check_lattice(g.dy, g.x, g.K, g.exact, F32)
    _eq(_ref.conv_wgrad(g.dy.float(), g.x.float(), k, k, s, p), g.exact)


@pytest.mark.parametrize("shape", X.linear_shapes(), ids=str)
def test_linear_reference_and_preconditions(shape):
    B, K_, N, width = shape
    l = X.linear_problem(shape)
    wpad = torch.zeros(width, K_)
    wpad[:N] = l.w.float()
    for (bias, relu), exact in l.exact.items():
        X.check_lattice(l.x, l.w, l.K, exact, BF16, bias=l.bias if bias else None)
        _eq(_ref.linear_fwd(l.x.float(), wpad, l.bias if bias else None, int(relu)), exact)
        assert not exact[:, N:].any()
    X.check_lattice(l.dy, l.wd, l.Kd, l.exact_dx, BF16)
    _eq(_ref.linear_fwd(l.dy[:, :N].float(), l.wd.float().t(), None, 0), l.exact_dx)
    X.check_lattice(l.dy7, l.x7, l.Kw, l.exact_dw, F32)
    _eq(_ref.linear_wgrad(l.dy7.float(), l.x7.float()), l.exact_dw)


@pytest.mark.parametrize("shape", X.grouped_shapes(), ids=str)
def test_grouped_reference_and_preconditions(shape):
    N, H, W, C, G, KH, s, p = shape
    g = X.grouped_problem(shape)
    X.check_lattice(g.x, g.w, g.K, g.exact, BF16)
    _eq(_ref.grouped_conv_fwd(g.x.float(), g.w.float(), G, s, p), g.exact)
    X.check_lattice(g.dy, g.wd, g.K, g.exact_dx, BF16)
    _eq(_ref.grouped_conv_dgrad(g.dy.float(), g.wd.float(), H, W, G, s, p), g.exact_dx)
    X.check_lattice(g.dy7, g.x7, g.Kw, g.exact_dw, F32)
    _eq(_ref.grouped_conv_wgrad(g.dy7.float(), g.x7.float(), KH, KH, G, s, p), g.exact_dw)


@pytest.mark.parametrize("shape", X.uniq([(N, H, H, Ci, Co, k, pad) for N, H, Ci, Co, k, pad in X.geo_shapes()] +
                                          [(N, H, W, 16, 64, 4, 2) for N, H, W in X.stem_shapes()]), ids=str)
def test_geo_and_stem_reference_and_preconditions(shape):
    N, H, W, Ci, Co, k, pad = shape
    g = X.geo_problem(shape)
    X.check_lattice(g.x, g.w, g.K, g.exact, BF16)
    _eq(_ref.conv_fwd_geo(g.x.float(), g.w.float(), 1, pad, H, W, False)[0], g.exact)
    X.check_lattice(g.dy, g.x7, g.Kw, g.exact_dw, F32)
    _eq(_ref.conv_wgrad_geo(g.dy.float(), g.x7.float(), k, k, 1, pad), g.exact_dw)


@pytest.mark.parametrize("shape", X.affine_shapes(), ids=str)
def test_affine_preconditions(shape):
    a = X.affine_problem(shape)
    f = a.f
    for act in (0, 1, 2):
        for res in (None, a.res):
            exact = X.exact_affine(f.exact, a.scale, a.shift, act, X.LEAKY_SLOPE, res)
            X.check_lattice(f.x, f.w, f.K, exact, BF16, scale=a.scale, shift=a.shift, res=res,
                            slope=X.LEAKY_SLOPE if act == 2 else None)


@pytest.mark.parametrize("shape", X.pro_shapes(), ids=str)
def test_prologue_reference_and_preconditions(shape):
    q = X.pro_problem(shape)
    X.check_lattice(q.a, q.w, q.K, q.exact, BF16, scale=q.scale, shift=q.shift)
    X.check_lattice(q.dy, q.a, q.Kw, q.exact_dw, F32)
    # the operand is a bf16 number before the rounding: the fp32 reference (which does not round it) agrees
    _eq(_ref.conv_fwd_pro(q.x.float(), q.w.float(), q.scale, q.shift, False)[0], q.exact)
    _eq(_ref.conv_wgrad_pro(q.dy.float(), q.x.float(), q.scale, q.shift), q.exact_dw)


@pytest.mark.parametrize("shape", X.pro3x3_shapes(), ids=str)
def test_prologue3x3_reference_and_preconditions(shape):
    q = X.pro3x3_problem(shape)
    X.check_lattice(q.a, q.w, q.K, q.exact, BF16, scale=q.scale, shift=q.shift)
    X.check_lattice(q.dy, q.a, q.Kw, q.exact_dw, F32)
    _eq(_ref.conv3x3_fwd_pro(q.x.float(), q.w.float(), q.scale, q.shift, False)[0], q.exact)
    _eq(_ref.conv3x3_wgrad_pro(q.dy.float(), q.x.float(), q.scale, q.shift), q.exact_dw)


def test_check_lattice_rejects_what_it_must():
    x = X.lattice((1, 4, 4, 64), -3, 3, 1)
    w = X.lattice((64, 1, 1, 64), -3, 3, 2)
    exact = X.exact_conv_fwd(x, w, 1, 0)
    with pytest.raises(AssertionError, match="need rounding"):  # sums far below 256: nothing rounds
        X.check_lattice(x, w, 64, exact, BF16)
    with pytest.raises(AssertionError, match="2\\^24"):
        X.check_lattice(x, w, 1 << 22, exact, F32)
    with pytest.raises(AssertionError, match="integers"):
        X.check_lattice(x.float() * 0.5, w, 64, exact, F32)
    with pytest.raises(AssertionError, match="bf16-representable"):
        X.check_lattice(x.float() + 257.0, w, 64, exact, F32)
    with pytest.raises(AssertionError, match="powers of two"):
        X.check_lattice(x, w, 64, exact, F32, scale=torch.full((64,), 3.0), shift=torch.zeros(64))
    with pytest.raises(AssertionError, match="shifts"):
        X.check_lattice(x, w, 64, exact, F32, scale=torch.ones(64), shift=torch.full((64,), 0.5))


# ----------------------------------------------------------------------------- sensitivity
SENS_SHAPE = (2, 56, 56, 64, 64, 3, 1, 1)


def _relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _split_k_bf16(x, w, s, p, parts=4):
    """each of ``parts`` channel slices of the k loop rounded to bf16 before the sum"""
    Ci = x.shape[-1]
    step = Ci // parts
    acc = None
    for i in range(parts):
        part = X.exact_conv_fwd(x[..., i * step:(i + 1) * step], w[..., i * step:(i + 1) * step], s, p)
        part = part.float().to(BF16).double()
        acc = part if acc is None else acc + part
    return acc.float().to(BF16)


@pytest.mark.parametrize("inputs", ["gaussian", "lattice"])
def test_sensitivity_old_tolerance_passes_exact_rejects(inputs):
    """Three defects a kernel can have -- a truncating store, split-K partials rounded to bf16, a
    dropped 8-channel tail vector -- and one element off by one bf16 ulp: each stays under the
    relerr < 1e-2 of the tolerance tests and each is rejected by assert_exact."""
    N, H, W, Ci, Co, k, s, p = SENS_SHAPE
    if inputs == "lattice":
        f = X.fwd_problem(SENS_SHAPE)
        x, w, exact = f.x, f.w, f.exact
    else:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(N, H, W, Ci, generator=g).to(BF16)
        w = (torch.randn(Co, k, k, Ci, generator=g) / (k * k * Ci) ** 0.5).to(BF16)
        exact = X.exact_conv_fwd(x, w, s, p).float().double()  # (the fp32 image: what an fp32 accumulator holds)
    want = exact.float().to(BF16)
    X.assert_exact(want.clone(), want, X.NHWC, "the correct result")
    defects = {}
    defects["truncating store"] = X.bf16_trunc(exact)
    defects["4 split-K partials rounded to bf16"] = _split_k_bf16(x, w, s, p)
    tail = want.clone()
    tail[-1, -1, -1, -8:] = 0
    defects["last 8-channel vector not stored"] = tail
    ulp = want.clone()
    v = ulp[1, 17, 23, 5].double()
    ulp[1, 17, 23, 5] = (v + X.bf16_ulp(v)).float().to(BF16)
    defects["one element off by one bf16 ulp"] = ulp
    for name, got in defects.items():
        err = _relerr(got, exact)
        print(f"sensitivity[{inputs}] {name}: relerr {err:.2e}, {(got != want).sum().item()} of {want.numel()} differ")
        assert err < 1e-2, name  # the existing criterion lets it through
        with pytest.raises(AssertionError, match="not bit-exact"):
            X.assert_exact(got, want, X.NHWC, name)


def test_mismatch_report_shows_the_pattern():
    want = X.fwd_problem((3, 9, 11, 64, 72, 3, 1, 1)).want
    got = want.clone()
    got.view(-1, 72)[128:, 64:] = 30000.0  # a ragged channel tail past the first 128-row tile
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, want, X.NHWC, "tail")
    msg = str(e.value)
    n = (297 - 128) * 8
    assert f"{n} of {want.numel()} elements differ" in msg
    assert "largest |got - want| = " in msg and "by output row mod 128" in msg and "by channel mod 64" in msg
    assert "'n': 1, 'h': 2, 'w': 7, 'c': 64" in msg  # row 128 = (1, 2, 7)
    assert msg.count("got ") >= 10
