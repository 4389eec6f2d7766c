"""Bit-exact checks of the MFMA conv / GEMM kernels on integer-lattice inputs.

Every path tests/test_kernels_gpu.py reaches with Gaussian inputs and a norm tolerance is run here
on small-integer inputs (tests/exact_oracle.py): every partial sum is an integer fp32 holds, so the
result cannot depend on tile shape, k order, split-K, stream-K, ping-pong or the parity classes, and
the only correct output is the exact sum rounded once.  The comparison is ``torch.equal``; one wrong
element, one wrong rounding, one dropped tail vector fails.  Shape lists and slot matrices are
those of tests/test_kernels_gpu.py (imported); each shape's CPU reference is computed once and the
variants loop inside one test.

Two store epilogues round twice by design (see ``_two_roundings``): they are held to the exact
result of the arithmetic they perform AND to the per-element bound that arithmetic implies against
the one-rounding reference.

Not here: BN statistics (mean / M2 merge in floating point), the BN-backward dgrad epilogue,
sigmoid / SE, ArcFace, the BN and loss kernels -- their arithmetic is not a lattice; they keep
their tolerance tests.
"""
import collections
import contextlib

import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.tuning import slot as tslot
from tests import exact_oracle as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = X.BF16, X.F32
TALLY = collections.Counter()  # family -> (shape, variant) cases that compared bit-exact
OFF_ONE_ROUNDING = collections.Counter()  # two-rounding families: elements that differ from the one-rounding reference


@pytest.fixture(scope="module")
def K():
    ops = _ext.hip_ops()
    yield ops
    print("\n[exact-lattice] bit-exact (shape, variant) cases per family:")
    for fam, n in sorted(TALLY.items()):
        print(f"[exact-lattice]   {fam}: {n}")
    for fam in sorted(f for f in OFF_ONE_ROUNDING if not f.endswith("#n")):
        print(f"[exact-lattice]   {fam}: {OFF_ONE_ROUNDING[fam]} of {OFF_ONE_ROUNDING[fam + '#n']} elements differ "
              f"from the one-rounding reference, all inside the derived bound")


@contextlib.contextmanager
def slots(K, cfg):
    """set the tuning slots of ``cfg`` = ((name, value), ...), run to completion, restore every one"""
    try:
        for name, v in cfg:
            K.set_tuning(tslot(name), v)
        yield
        torch.cuda.synchronize()
    finally:
        for name, _ in cfg:
            K.set_tuning(tslot(name), 0)


def d(t):
    return None if t is None else t.to(DEV)


def exact(family, got, want, dims, what):
    X.assert_exact(got, want, dims, what)
    TALLY[family] += 1


def _two_roundings(model_pre, single_exact, first_err):
    """A store epilogue that rounds twice by design: the conv result goes through the bf16 tile image
    in LDS before the epilogue's own arithmetic, conv_igemm.hip tg_image_store (line 324, ``float t =
    bf2f(v[e]) * fsc[e] + fsh[e]`` for the folded BN; line 333, ``f2bf(bf2f(v[e]) + bf2f(a[e]))`` for
    the dgrad add source; the stride-2 dgrad adds its source with a bf16 ``dx.add_(*add)``,
    bindings.cpp line 540 in conv_dgrad).  So the output is bf16(f(bf16(conv))) and not bf16(f(conv)):
    16-18 % of the lattice outputs differ from the one-rounding reference
    (profiles/r7/exact_lattice.txt).  A precision decision, not a defect: ops/_ref.py conv_fwd_affine
    documents the folded BN as going "through the bf16-rounded conv output like the unfused chain".

    ``model_pre``: f(bf16(conv)) in fp64 -- everything after the first rounding is exact on the
    lattice, so the kernel must equal its rounding bit for bit.  Against the one-rounding reference
    ``single_exact`` = f(conv) the arithmetic implies, per element, half a bf16 ulp of the conv value
    (times |scale|; the activations are 1-Lipschitz) for the first rounding plus half a bf16 ulp of
    the stored value's pre-image for the second: that bound is asserted too, not a norm.
    -> the device tensors ``check_two_roundings`` compares against (built once per problem)."""
    bound = first_err + 0.5 * X.bf16_ulp(model_pre)
    return d(X.rounded(model_pre, BF16)), d(single_exact), d(bound), d(X.rounded(single_exact, BF16))


def check_two_roundings(family, got, model, dims, what):
    want2, single, bound, want1 = model
    bad = (got.double() - single).abs() > bound
    if bad.any():
        s = single.cpu()
        raise AssertionError(f"{what}: {int(bad.sum())} elements beyond the two-rounding bound\n" +
                             X.mismatch_report(torch.where(bad.cpu(), got.double().cpu(), s), s, dims))
    exact(family, got, want2, dims, what + " (two-rounding model)")
    OFF_ONE_ROUNDING[family] += int((got != want1).sum())
    OFF_ONE_ROUNDING[family + "#n"] += got.numel()


def _cfg_name(cfg):
    return ",".join(f"{k}={v}" for k, v in cfg) or "default"


PIPELINE = [(("tg_stages", 3),), (("tg_stages", 4),), (("tg_stages", 3), ("tg_kdepth", 32)),
            (("tg_stages", 4), ("tg_kdepth", 32))]


# ----------------------------------------------------------------------------- tap GEMM forward
@pytest.mark.parametrize("shape", X.conv_shapes(), ids=str)
def test_tap_gemm_fwd(K, shape):
    """conv_fwd under the default plan and the pipeline / tile / k-depth variants.  The 64 -> 64 3x3
    shapes take the direct kernel by default: every variant runs there with c3_off = 1 as well, so
    the slots act on the tap GEMM."""
    N, H, W, Ci, Co, k, s, p = shape
    f = X.fwd_problem(shape)
    X.check_lattice(f.x, f.w, f.K, f.exact, BF16)
    x, w, want = d(f.x), d(f.w), d(f.want)
    cfgs = [()] + PIPELINE + [(("tg_tile_n", v),) for v in (64, 128, 256)] + [(("tg_pingpong", v),) for v in (1, 2)]
    if Ci % 64 != 0:  # narrow-channel (per-lane tap lookup) shapes
        cfgs += [(("narrow_kdepth", 32),), (("narrow_kdepth", 64),)]
    if (Ci, Co, k, s) == (64, 64, 3, 1):
        cfgs += [c + (("c3_off", 1),) for c in cfgs]
    for cfg in cfgs:
        with slots(K, cfg):
            y, _ = K.conv_fwd(x, w, s, p, True)
        exact("tap GEMM forward", y, want, X.NHWC, f"conv_fwd {shape} {_cfg_name(cfg)}")
    y, none = K.conv_fwd(x, w, s, p, False)
    assert none.numel() == 0
    exact("tap GEMM forward", y, want, X.NHWC, f"conv_fwd {shape} plain store")


def _big_cfgs():
    out = []
    for mode in (1, 3):
        for cvar in (0, 1, 2, 3):
            for stages, persist in ((0, 0), (5, 0), (0, 1)):
                if stages and mode != 1:
                    continue  # the 5-slot ring is the 256 x 256 tile's
                out.append((("tg_big", mode), ("tg_big_cvar", cvar), ("tg_big_stages", stages),
                            ("tg_big_persist", persist)))
    return out


def _fwd_dgrad_variants(K, family, shape, cfgs, add=True):
    """forward (statistics epilogue) and data gradient of ``shape`` under each of ``cfgs``"""
    N, H, W, Ci, Co, k, s, p = shape
    f, g = X.fwd_problem(shape), X.dgrad_problem(shape)
    X.check_lattice(f.x, f.w, f.K, f.exact, BF16)
    X.check_lattice(g.dy, g.w, g.K, g.exact, BF16)
    x, w, want = d(f.x), d(f.w), d(f.want)
    dy, want_dx, addt = d(g.dy), d(g.want), d(g.add)
    _, wt = K.weight_prep(d(g.w.float()), 0, True)
    model = _dgrad_add_model(g) if add else None
    for cfg in cfgs:
        with slots(K, cfg):
            y, _ = K.conv_fwd(x, w, s, p, True)
            dx = K.conv_dgrad(dy, wt, H, W, s, p)
            dxa = K.conv_dgrad(dy, wt, H, W, s, p, addt) if add else None
        exact(family, y, want, X.NHWC, f"conv_fwd {shape} {_cfg_name(cfg)}")
        exact(family, dx, want_dx, X.NHWC, f"conv_dgrad {shape} {_cfg_name(cfg)}")
        if dxa is not None:
            check_two_roundings(family + " + add (two roundings)", dxa, model, X.NHWC,
                                f"conv_dgrad+add {shape} {_cfg_name(cfg)}")


def _dgrad_add_model(g):
    pre = X.rounded(g.exact, BF16).double() + g.add.double()
    return _two_roundings(pre, g.exact_add, 0.5 * X.bf16_ulp(g.exact))


@pytest.mark.parametrize("shape", X.big_tile_shapes(), ids=str)
def test_big_tile_fwd_dgrad(K, shape):
    """the 256 x 256 / 256 x 128 big tiles under every schedule, ring depth and as persistent workgroups"""
    _fwd_dgrad_variants(K, "big tiles", shape, _big_cfgs())


@pytest.mark.parametrize("shape", X.stream_k_shapes(), ids=str)
def test_stream_k_fwd_dgrad(K, shape):
    """stream-K big tiles: a tile cut between workgroups publishes an fp32 partial -- exact on the lattice"""
    cfgs = [(("tg_big", mode), ("tg_big_sk", sk)) for mode in (1, 3) for sk in (3, 5, 7)]
    _fwd_dgrad_variants(K, "stream-K", shape, cfgs)


@pytest.mark.parametrize("shape", X.split_k_shapes(), ids=str)
def test_split_k_fwd_dgrad(K, shape):
    """split-K of the 128-row tap GEMM on short grids: fp32 partial slices, one fixed-order reduce"""
    cfgs = [(), (("tg_split_k", 2),), (("tg_split_k", 4),), (("tg_kdepth", 32), ("tg_stages", 2))]
    _fwd_dgrad_variants(K, "split-K", shape, cfgs)


@pytest.mark.parametrize("shape", X.ws_shapes(), ids=str)
def test_conv1x1_ws_ps(K, shape):
    """the weight-stationary persistent 1x1 kernel and the loader / consumer kernel (4 and 8 consumer waves)"""
    N, H, W, Ci, Co, k, s, p = shape
    f = X.fwd_problem(shape)
    X.check_lattice(f.x, f.w, f.K, f.exact, BF16)
    x, w, want = d(f.x), d(f.w), d(f.want)
    for cfg in ((("tg_ws", 1),), (("tg_ps", 1),), (("tg_ps", 3),)):
        with slots(K, cfg):
            y, _ = K.conv_fwd(x, w, 1, 0, True)
            y0, _ = K.conv_fwd(x, w, 1, 0, False)
        exact("1x1 ws / ps", y, want, X.NHWC, f"conv_fwd+stats {shape} {_cfg_name(cfg)}")
        exact("1x1 ws / ps", y0, want, X.NHWC, f"conv_fwd {shape} {_cfg_name(cfg)}")


@pytest.mark.parametrize("shape", X.tile256_shapes(), ids=str)
def test_conv_fwd_256_channel_tiles(K, shape):
    N, H, W, Ci, Co, k, s, p = shape
    f = X.fwd_problem(shape)
    X.check_lattice(f.x, f.w, f.K, f.exact, BF16)
    x, w, want = d(f.x), d(f.w), d(f.want)
    for cfg in ((("tg_split_k", 2),), (("tg_split_k", 2), ("tg_tile_n", 256))):
        for stats in (True, False):
            with slots(K, cfg):
                y, _ = K.conv_fwd(x, w, s, p, stats)
            exact("256-channel tiles", y, want, X.NHWC, f"conv_fwd {shape} {_cfg_name(cfg)} stats={stats}")


# ----------------------------------------------------------------------------- direct 64 -> 64 3x3
@pytest.mark.parametrize("shape", X.c3_shapes(), ids=str)
def test_conv3x3_direct(K, shape):
    """conv3x3.hip: every workgroup variant x both store epilogues, with and without the statistics
    partials; the data gradient of the same geometry (the direct kernel on the flipped weight); and
    c3_off = 1 (the implicit GEMM) on the same inputs."""
    N, H, W, Ci, Co, k, s, p = shape
    f, g = X.fwd_problem(shape), X.dgrad_problem(shape)
    X.check_lattice(f.x, f.w, f.K, f.exact, BF16)
    X.check_lattice(g.dy, g.w, g.K, g.exact, BF16)
    x, w, want = d(f.x), d(f.w), d(f.want)
    dy, want_dx = d(g.dy), d(g.want)
    _, wt = K.weight_prep(d(g.w.float()), 0, True)
    for variant in (0, 1, 2, 3, 4):
        for epi in (0, 2):
            cfg = (("c3_variant", variant), ("c3_epilogue", epi))
            with slots(K, cfg):
                y, _ = K.conv_fwd(x, w, 1, 1, True)
                y0, _ = K.conv_fwd(x, w, 1, 1, False)
                dx = K.conv_dgrad(dy, wt, H, W, 1, 1)
            exact("direct 3x3", y, want, X.NHWC, f"conv3x3+stats {shape} {_cfg_name(cfg)}")
            exact("direct 3x3", y0, want, X.NHWC, f"conv3x3 {shape} {_cfg_name(cfg)}")
            exact("direct 3x3", dx, want_dx, X.NHWC, f"conv3x3 dgrad {shape} {_cfg_name(cfg)}")
    with slots(K, (("c3_off", 1),)):
        y, _ = K.conv_fwd(x, w, 1, 1, True)
        dx = K.conv_dgrad(dy, wt, H, W, 1, 1)
    exact("direct 3x3", y, want, X.NHWC, f"conv_fwd {shape} c3_off=1")
    exact("direct 3x3", dx, want_dx, X.NHWC, f"conv_dgrad {shape} c3_off=1")


# ----------------------------------------------------------------------------- data gradient
@pytest.mark.parametrize("shape", X.uniq(X.dgrad_shapes() + X.parity_stream_shapes()), ids=str)
def test_conv_dgrad(K, shape):
    """conv_dgrad, stride 1 and the stride-2 parity classes (serial and on concurrent streams), with
    and without an integer add source, under the pipeline, tile-width and big-tile variants"""
    N, H, W, Ci, Co, k, s, p = shape
    g = X.dgrad_problem(shape)
    X.check_lattice(g.dy, g.w, g.K, g.exact, BF16)
    X.check_lattice(g.dy, g.w, g.K, g.exact_add, BF16, res=g.add)
    dy, want, addt = d(g.dy), d(g.want), d(g.add)
    _, wt = K.weight_prep(d(g.w.float()), 0, True)
    cfgs = [()] + PIPELINE + [(("tg_tile_n", 64),), (("tg_tile_n", 128),), (("tg_big", 1),), (("tg_big", 3),)]
    model = _dgrad_add_model(g)
    if s == 2:
        cfgs += [(("dgrad_parity_streams", 1),)]
    for cfg in cfgs:
        with slots(K, cfg):
            dx = K.conv_dgrad(dy, wt, H, W, s, p)
            dxa = K.conv_dgrad(dy, wt, H, W, s, p, addt)  # (stride 2: added to the assembled classes, in bf16)
        exact("data gradient", dx, want, X.NHWC, f"conv_dgrad {shape} {_cfg_name(cfg)}")
        check_two_roundings("data gradient + add (two roundings)", dxa, model, X.NHWC,
                            f"conv_dgrad+add {shape} {_cfg_name(cfg)}")


# ----------------------------------------------------------------------------- weight gradient
WG_EVERYWHERE = [(), (("wg_splits_per_cu", 4),), (("wg_rows", 32),), (("wg_split_cap", 8),), (("wg_tile_mode", 2),),
                 (("wg_tile_mode", 3),), (("row_reduce", 2),), (("row_reduce", 16),)]


@pytest.mark.parametrize("shape", X.all_wgrad_shapes(), ids=str)
def test_conv_wgrad(K, shape):
    """conv_wgrad, fp32 output: split partials are fp32 and reduced in a fixed order, so every plan
    is exact.  The slot matrix of test_conv_wgrad_variants on its shapes; split plan, k-tile rows,
    tile mode and the reduction on all; wg3x3 = 1 (implicit GEMM) / 2 (direct kernel on any channel
    block count) on the 3x3 stride-1 shapes."""
    N, H, W, Ci, Co, k, s, p = shape
    g = X.wgrad_problem(shape)
    X.check_lattice(g.dy, g.x, g.K, g.exact, F32)
    dy, x, want = d(g.dy), d(g.x), d(g.want)
    cfgs = list(WG_EVERYWHERE)
    if shape in X.wgrad_variant_shapes():
        cfgs += [tuple(c) for c in X.wgrad_variant_cfgs()]
    if (k, s, p) == (3, 1, 1):
        cfgs += [(("wg3x3", 1),), (("wg3x3", 2),)]
    for cfg in X.uniq(cfgs):
        with slots(K, cfg):
            dw = K.conv_wgrad(dy, x, k, k, s, p)
        exact("weight gradient", dw, want, X.OHWI, f"conv_wgrad {shape} {_cfg_name(cfg)}")


# ----------------------------------------------------------------------------- linear
@pytest.mark.parametrize("shape", X.linear_shapes(), ids=str)
def test_linear(K, shape):
    """linear_fwd with an integer bias and ReLU on / off (bias joins the fp32 accumulator: one
    rounding), the input gradient through the transposed weight, linear_wgrad; an unpadded bias on
    the padded GEMM leaves the columns past it exactly 0."""
    B, K_, N, width = shape
    l = X.linear_problem(shape)
    for (bias, relu), ex in l.exact.items():
        X.check_lattice(l.x, l.w, l.K, ex, BF16, bias=l.bias if bias else None)
    X.check_lattice(l.dy, l.wd, l.Kd, l.exact_dx, BF16)
    X.check_lattice(l.dy7, l.x7, l.Kw, l.exact_dw, F32)
    wb, _ = K.weight_prep(d(l.w.float()), width, False)
    _, wdt = K.weight_prep(d(l.wd.float()), width, True)
    x = d(l.x)
    for (bias, relu), want in l.want.items():
        y = K.linear_fwd(x, wb, d(l.bias) if bias else None, int(relu))
        exact("linear", y, d(want), ("b", "n"), f"linear_fwd {shape} bias={bias} relu={relu}")
        assert not y[:, N:].any()
    dx = K.linear_fwd(d(l.dy), wdt, None, 0)
    exact("linear", dx, d(l.want_dx), ("b", "k"), f"linear dgrad {shape}")
    dw = K.linear_wgrad(d(l.dy7), d(l.x7))
    exact("linear", dw, d(l.want_dw), ("n", "k"), f"linear_wgrad {shape}")


# ----------------------------------------------------------------------------- affine / prologue
@pytest.mark.parametrize("shape", X.affine_shapes(), ids=str)
def test_conv_fwd_affine(K, shape):
    """conv_fwd_affine with power-of-two scales, integer shifts / residuals and a power-of-two leaky
    slope: act none / ReLU / leaky, with and without the residual.  Two roundings by design."""
    N, H, W, Ci, Co, k, s, p = shape
    a = X.affine_problem(shape)
    f = a.f
    x, w, scale, shift = d(f.x), d(f.w), d(a.scale), d(a.shift)
    conv_bf = X.rounded(f.exact, BF16).double()
    first = 0.5 * X.bf16_ulp(f.exact) * a.scale.double().abs()
    for act in (0, 1, 2):
        for res in (None, a.res):
            single = X.exact_affine(f.exact, a.scale, a.shift, act, X.LEAKY_SLOPE, res)
            X.check_lattice(f.x, f.w, f.K, single, BF16, scale=a.scale, shift=a.shift, res=res,
                            slope=X.LEAKY_SLOPE if act == 2 else None)
            y = K.conv_fwd_affine(x, w, s, p, scale, shift, act, X.LEAKY_SLOPE, d(res))
            torch.cuda.synchronize()
            pre = X.exact_affine(conv_bf, a.scale, a.shift, act, X.LEAKY_SLOPE, res)
            check_two_roundings("affine epilogue (two roundings)", y, _two_roundings(pre, single, first), X.NHWC,
                                f"conv_fwd_affine {shape} act={act} res={res is not None}")


@pytest.mark.parametrize("shape", X.pro_shapes(), ids=str)
def test_conv_bn_prologue(K, shape):
    """conv_fwd_pro / conv_wgrad_pro: relu(x * scale + shift) applied to the operand in registers"""
    q = X.pro_problem(shape)
    X.check_lattice(q.a, q.w, q.K, q.exact, BF16, scale=q.scale, shift=q.shift)
    X.check_lattice(q.dy, q.a, q.Kw, q.exact_dw, F32)
    x, w, scale, shift = d(q.x), d(q.w), d(q.scale), d(q.shift)
    for stats in (True, False):
        y, _ = K.conv_fwd_pro(x, w, scale, shift, stats)
        exact("BN prologue", y, d(q.want), X.NHWC, f"conv_fwd_pro {shape} stats={stats}")
    dw = K.conv_wgrad_pro(d(q.dy), x, scale, shift)
    exact("BN prologue", dw, d(q.want_dw), X.OHWI, f"conv_wgrad_pro {shape}")


@pytest.mark.parametrize("shape", X.pro3x3_shapes(), ids=str)
def test_conv3x3_bn_prologue(K, shape):
    """conv3x3_fwd_pro / conv3x3_wgrad_pro: the prologue on the staged windows, zero padding of its output"""
    N, H, W = shape
    q = X.pro3x3_problem(shape)
    X.check_lattice(q.a, q.w, q.K, q.exact, BF16, scale=q.scale, shift=q.shift)
    X.check_lattice(q.dy, q.a, q.Kw, q.exact_dw, F32)
    assert K.conv3x3_pro_fits(N, H, W, 64, 64)
    x, w, scale, shift = d(q.x), d(q.w), d(q.scale), d(q.shift)
    for stats in (True, False):
        y, _ = K.conv3x3_fwd_pro(x, w, scale, shift, stats)
        exact("BN prologue", y, d(q.want), X.NHWC, f"conv3x3_fwd_pro {shape} stats={stats}")
    dw = K.conv3x3_wgrad_pro(d(q.dy), x, scale, shift)
    exact("BN prologue", dw, d(q.want_dw), X.OHWI, f"conv3x3_wgrad_pro {shape}")


# ----------------------------------------------------------------------------- stem / geo / grouped
@pytest.mark.parametrize("shape", X.stem_shapes(), ids=str)
def test_stem_fwd(K, shape):
    """the dedicated s2d stem kernel (stem.hip) and its implicit-GEMM fallback, y only"""
    q = X.stem_problem(shape)
    X.check_lattice(q.x, q.w, q.K, q.exact, BF16)
    for stats in (True, False):
        y, _ = K.stem_fwd(d(q.x), d(q.w), stats)
        exact("stem / explicit grid", y, d(q.want), X.NHWC, f"stem_fwd {shape} stats={stats}")


@pytest.mark.parametrize("shape", X.geo_shapes(), ids=str)
def test_conv_geo(K, shape):
    """explicit-grid conv and its weight gradient; the narrow-channel k depths on the 16-channel shapes"""
    N, H, Ci, Co, k, pad = shape
    q = X.geo_problem((N, H, H, Ci, Co, k, pad))
    X.check_lattice(q.x, q.w, q.K, q.exact, BF16)
    X.check_lattice(q.dy, q.x7, q.Kw, q.exact_dw, F32)
    cfgs = [()] + ([(("narrow_kdepth", 32),), (("narrow_kdepth", 64),)] if Ci % 64 else [])
    for cfg in cfgs:
        with slots(K, cfg):
            y, _ = K.conv_fwd_geo(d(q.x), d(q.w), 1, pad, H, H, True)
        exact("stem / explicit grid", y, d(q.want), X.NHWC, f"conv_fwd_geo {shape} {_cfg_name(cfg)}")
    dw = K.conv_wgrad_geo(d(q.dy), d(q.x7), k, k, 1, pad)
    exact("stem / explicit grid", dw, d(q.want_dw), X.OHWI, f"conv_wgrad_geo {shape}")


@pytest.mark.parametrize("shape", X.grouped_shapes(), ids=str)
def test_grouped_conv(K, shape):
    """grouped_conv_fwd / _dgrad / _wgrad: default, the weight gradient's super-group choices
    (gconv_sg 16 / 32 / 1) and two super-groups-per-workgroup values for forward and dgrad"""
    N, H, W, C, G, KH, s, p = shape
    q = X.grouped_problem(shape)
    X.check_lattice(q.x, q.w, q.K, q.exact, BF16)
    X.check_lattice(q.dy, q.wd, q.K, q.exact_dx, BF16)
    X.check_lattice(q.dy7, q.x7, q.Kw, q.exact_dw, F32)
    for cfg in ((), (("gconv_sg", 16),), (("gconv_sg", 32),), (("gconv_sg", 1),), (("gconv_spw", 2),), (("gconv_spw", 3),)):
        with slots(K, cfg):
            y = K.grouped_conv_fwd(d(q.x), d(q.w), G, s, p)
            dx = K.grouped_conv_dgrad(d(q.dy), d(q.wd), H, W, G, s, p)
            dw = K.grouped_conv_wgrad(d(q.dy7), d(q.x7), KH, KH, G, s, p)
        exact("grouped conv", y, d(q.want), X.NHWC, f"grouped_conv_fwd {shape} {_cfg_name(cfg)}")
        exact("grouped conv", dx, d(q.want_dx), X.NHWC, f"grouped_conv_dgrad {shape} {_cfg_name(cfg)}")
        exact("grouped conv", dw, d(q.want_dw), ("co", "kh", "kw", "cg"), f"grouped_conv_wgrad {shape} {_cfg_name(cfg)}")
