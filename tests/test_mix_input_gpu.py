"""The mixed input kernels (csrc/misc.hip, to_nhwc_pix_mix_kernel<1,8> / <2,4> / <4,3>) against the
fp64 oracle of tests/mix_ref.py and against the unmixed kernels' own output.

Shapes: N = 5 (odd: the middle row pairs with itself) and N = 1; (H, W) = (8, 8), (12, 20) for every
layout and (7, 9) for the plain one; uint8 NHWC, uint8 NCHW (even W: the packed two-byte route of the
2x2 layout) and fp32 in both orders.  Boxes: empty, one pixel, the whole image, touching each edge,
odd coordinates (2x2 and 4x4 output blocks straddle every box edge).

* Lattice (torch.equal): mean 0, std 1, in_scale 1, integer pixels 0..255 and blend k/16.  Every
  intermediate of fmaf(blend, a, (1 - blend) * b) is then an fp32 number under any contraction
  (a multiple of 1/16 below 2^8: 12 bits), so the output is the fp64 value rounded once to bf16.
* ImageNet mean / std (torch.equal against the unmixed kernel): with blend in {0, 1} a plan is a
  per-pixel selection between the unmixed outputs of the two images; the identity plan is the
  unmixed kernel.
* General blend (0.3, 0.77): the kernel blends the two unmixed bf16 values in fp32 and rounds once, so
  with A, B the unmixed bf16 outputs and m = blend |A| + (1 - blend) |B|,
  |out - (blend A + (1 - blend) B)| <= 2^-8 m + 2^-20: one bf16 rounding of the result (unit roundoff
  2^-8, |result| <= m) and fp32 slack (1 - blend, the product and the fma round once each on |v| <= 2.7:
  below 2^-20).  The worst ratio is printed.
* The sampler's own plans on the lattice: rows with blend == 1 (CutMix, identity) exactly; Mixup rows
  (an arbitrary fp32 blend: 1 - blend, the product and the fma each round once in fp32, an absolute
  error below e = 3 * 2^-24 * 255) within 2^-8 |v| + 2 e of the fp64 value v -- its one bf16 rounding
  (unit roundoff 2^-8).
"""
import pytest
import torch

from ddp_classification_pytorch_amd import _ext
from ddp_classification_pytorch_amd.data.mix import MixSampler, identity_plan
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import mix_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = [("plain", 8, 8), ("plain", 12, 20), ("plain", 7, 9), ("s2d2", 8, 8), ("s2d2", 12, 20), ("s2d4", 8, 8),
          ("s2d4", 12, 20)]
SOURCES = ["u8-nhwc", "u8-nchw", "f32-nhwc", "f32-nchw"]


def _source(kind, N, H, W, seed):
    """-> (tensor as the op takes it, nchw)"""
    gen = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=gen)
    if kind.startswith("f32"):
        img = img.float()
    nchw = kind.endswith("nchw")
    return (img.permute(0, 3, 1, 2).contiguous() if nchw else img), nchw


def _boxes(H, W):
    return [[0, 0, 0, 0], [1, 1, 2, 2], [0, 0, H, W], [0, 0, 3, 5], [H - 3, W - 5, H, W], [0, W - 3, 3, W],
            [H - 3, 0, H, 3], [1, 3, 5, 7], [3, 1, H - 1, W - 3], [2, 0, 3, W]]


def _plans(N, H, W, blends):
    """Plans covering every box of _boxes and every blend of ``blends``, rows cycling through both."""
    boxes = _boxes(H, W)
    partner = torch.arange(N - 1, -1, -1, dtype=torch.int32)
    plans = []
    n_plans = max(-(-len(boxes) // N), -(-len(blends) // N)) + 1
    for k in range(n_plans):
        box = torch.tensor([boxes[(k * N + n) % len(boxes)] for n in range(N)], dtype=torch.int32)
        bl = torch.tensor([blends[(k * N + 2 * n + k) % len(blends)] for n in range(N)], dtype=torch.float32)
        plans.append((partner, bl, box))
    # rows that blend without a box, and boxed rows that do not blend
    plans.append((partner, torch.tensor([blends[(3 * n + 1) % len(blends)] for n in range(N)]),
                  torch.zeros(N, 4, dtype=torch.int32)))
    return plans


def _dev(plan):
    return tuple(t.to(DEV) for t in plan[:3])


def _run(src, nchw, layout, plan, mean=None, std=None, in_scale=1.0):
    S = M.LAYOUTS[layout][0]
    mean = mean.to(DEV) if torch.is_tensor(mean) else mean
    std = std.to(DEV) if torch.is_tensor(std) else std
    return Fn.to_device_nhwc(src.to(DEV), mean, std, cpad=8, nchw=nchw, in_scale=in_scale, s2d=S if S > 1 else False,
                             mix=None if plan is None else _dev(plan))


@pytest.mark.parametrize("N", [5, 1])
@pytest.mark.parametrize("layout,H,W", SHAPES)
def test_lattice_exact(layout, H, W, N):
    blends = [k / 16.0 for k in range(17)]
    zero, one = torch.zeros(3), torch.ones(3)
    for kind in SOURCES:
        src, nchw = _source(kind, N, H, W, 10 + H)
        for plan in _plans(N, H, W, blends):
            got = _run(src, nchw, layout, plan, zero, one).cpu()
            want = M.mix_images(src, nchw, 1.0, zero, one, plan, layout)
            assert got.dtype == torch.bfloat16 and got.shape == want.shape
            assert torch.equal(got, want.to(torch.bfloat16)), (kind, plan)
            cq = M.LAYOUTS[layout][1]
            if cq > 3:  # the 4x4 layout has three channel slots: no pad
                pads = got.reshape(*got.shape[:3], -1, cq)[..., 3:]
                assert pads.numel() > 0 and (pads == 0).all()
            # and with no mean / std tensors at all
            assert torch.equal(_run(src, nchw, layout, plan).cpu(), got)


@pytest.mark.parametrize("N", [5, 1])
@pytest.mark.parametrize("layout,H,W", SHAPES)
def test_imagenet_stats_select_between_the_unmixed_outputs(layout, H, W, N):
    for kind in SOURCES:
        src, nchw = _source(kind, N, H, W, 20 + W)
        A = _run(src, nchw, layout, None, MEAN, STD, 1 / 255.0).cpu()
        ident = tuple(torch.from_numpy(a) for a in identity_plan(N)[:3])
        assert torch.equal(_run(src, nchw, layout, ident, MEAN, STD, 1 / 255.0).cpu(), A), kind
        for partner, blend, box in _plans(N, H, W, [1.0, 0.0, 1.0]):
            got = _run(src, nchw, layout, (partner, blend, box), MEAN, STD, 1 / 255.0).cpu()
            B = A[partner.long()]
            outside = torch.where((blend == 1).view(N, 1, 1, 1), A, B)
            want = torch.where(M.inside_layout(box, N, H, W, layout), B, outside)
            assert torch.equal(got, want), (kind, blend, box)


def _general_blend_worst(layout, H, W, N, rel):
    """Worst |out - (blend A + (1 - blend) B)| / (rel (blend |A| + (1 - blend) |B|) + 2^-20) outside the
    boxes; inside them the output must be B exactly."""
    worst = 0.0
    for kind in SOURCES:
        src, nchw = _source(kind, N, H, W, 30 + H + W)
        A = _run(src, nchw, layout, None, MEAN, STD, 1 / 255.0).cpu()
        for partner, blend, box in _plans(N, H, W, [0.3, 0.77]):
            got = _run(src, nchw, layout, (partner, blend, box), MEAN, STD, 1 / 255.0).cpu()
            B = A[partner.long()]
            bl = blend.double().view(N, 1, 1, 1)
            ins = M.inside_layout(box, N, H, W, layout)
            assert torch.equal(got[ins], B[ins]), kind
            Ad, Bd = A.double(), B.double()
            err = (got.double() - (bl * Ad + (1 - bl) * Bd)).abs()
            bound = rel * (bl * Ad.abs() + (1 - bl) * Bd.abs()) + 2.0 ** -20
            worst = max(worst, (err / bound)[~ins].max().item() if (~ins).any() else 0.0)
    return worst


@pytest.mark.parametrize("N", [5, 1])
@pytest.mark.parametrize("layout,H,W", SHAPES)
def test_general_blend_within_the_rounding_bound(layout, H, W, N):
    """2^-8 m + 2^-20 against the blend of the unmixed bf16 outputs (module docstring)."""
    worst = _general_blend_worst(layout, H, W, N, 2.0 ** -8)
    print(f"mix general blend {layout} {H}x{W} N={N}: worst err / (2^-8 m + 2^-20) {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_the_samplers_own_plans_on_the_lattice(mode):
    N, H, W = 5, 12, 20
    sampler = MixSampler(0.8, 1.0, mode=mode, seed=21)
    zero, one = torch.zeros(3), torch.ones(3)
    src, nchw = _source("u8-nhwc", N, H, W, 40)
    e = 3 * 2.0 ** -24 * 255
    seen, worst = set(), 0.0
    for step in range(20):
        p = sampler.draw(N, H, W, step)
        plan = tuple(torch.from_numpy(a) for a in p[:3])
        for layout in ("plain", "s2d2", "s2d4"):
            got = _run(src, nchw, layout, plan, zero, one).cpu()
            want = M.mix_images(src, nchw, 1.0, zero, one, plan, layout)
            exact = plan[1] == 1
            assert torch.equal(got[exact], want.to(torch.bfloat16)[exact]), (step, layout)
            if (~exact).any():
                err = (got.double() - want).abs()[~exact]
                bound = 2.0 ** -8 * want.abs()[~exact] + 2 * e
                worst = max(worst, (err / bound).max().item())
        seen.add("cutmix" if (p.box != 0).any() else "mixup")
    print(f"mix sampler plans ({mode}): worst Mixup err / bound {worst:.4f}")
    assert seen == {"cutmix", "mixup"} and worst <= 1.0


def test_ops_refuse_what_they_cannot_mix():
    K = _ext.hip_ops()
    src = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device=DEV)
    partner, blend, box = _dev(tuple(torch.from_numpy(a) for a in identity_plan(2)[:3]))
    with pytest.raises(RuntimeError, match="8-slot"):
        K.to_nhwc_mix(src, False, 16, 1.0, None, None, partner, blend, box)
    with pytest.raises(ValueError, match="mix plan"):
        Fn.to_device_nhwc(src, None, None, cpad=3, nchw=False, mix=(partner, blend, box))
    with pytest.raises(RuntimeError, match="partner int32"):
        K.to_nhwc_mix(src, False, 8, 1.0, None, None, partner.long(), blend, box)
    with pytest.raises(RuntimeError, match="box int32"):
        K.to_nhwc_s2d_mix(src, False, 1.0, None, None, partner, blend, box[:1], 2)
