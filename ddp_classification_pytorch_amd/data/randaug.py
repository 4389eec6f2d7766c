"""RandAugment (Cubuk et al. 2020) for the shard loader: the definition, in Pillow calls, and the plans.

The op space is torchvision's ``RandAugment``: 14 ops, 31 bins, a level ``L = magnitude`` in 0..30 and
``f = L / 30``.  :func:`apply_pil` is the definition -- every op is one literal Pillow call -- and the CPU
path of ``Fn.rand_augment``; the device kernel (``dcp::rand_augment``, csrc/randaug.hip) redoes Pillow's C
arithmetic and is held to these bytes with ``torch.equal``.

==  =========================  ====================  ===========================================================
id  op                         parameter             Pillow call
==  =========================  ====================  ===========================================================
0   Identity                   --                    --
1   ShearX                     v = +-0.3 f           transform(size, AFFINE, (1, v, 0, 0, 1, 0), NEAREST, fill 0)
2   ShearY                     v = +-0.3 f           transform(size, AFFINE, (1, 0, 0, v, 1, 0), NEAREST, fill 0)
3   TranslateX                 px = +-int(f 150/331 W)  transform(size, AFFINE, (1, 0, px, 0, 1, 0), NEAREST, fill 0)
4   TranslateY                 px = +-int(f 150/331 H)  transform(size, AFFINE, (1, 0, 0, 0, 1, px), NEAREST, fill 0)
5   Rotate                     deg = +-30 f          rotate(deg, NEAREST, fillcolor 0)
6   Brightness                 factor = 1 +- 0.9 f   ImageEnhance.Brightness(img).enhance(factor)
7   Color                      factor                ImageEnhance.Color(img).enhance(factor)
8   Contrast                   factor                ImageEnhance.Contrast(img).enhance(factor)
9   Sharpness                  factor                ImageEnhance.Sharpness(img).enhance(factor)
10  Posterize                  bits = 8 - round(4 f)    ImageOps.posterize(img, bits)
11  Solarize                   thr = 255 - round(255 f) ImageOps.solarize(img, thr)
12  AutoContrast               --                    ImageOps.autocontrast(img)
13  Equalize                   --                    ImageOps.equalize(img)
==  =========================  ====================  ===========================================================

A signed parameter is negative with probability 1/2; every slot draws its op uniformly from the 14.  A
float parameter is computed in fp64 and rounded once to fp32; that value, as a Python float, is what
Pillow receives and what the device reads.

A plan (:class:`RandAugPlan`) holds, for N images x K ops, the op id, the fp32 parameter, the integer
parameter and -- for the five geometric ops -- the six 16.16 integers of Pillow's nearest affine path,
computed here as ``Image.py`` and ``Geometry.c`` compute them (Python floats are C doubles), so the device
needs no trigonometry.  :func:`pack` lays it out as int32 ``[N, K, 8]`` = {op, parameter bits, a0..a5}.
Draws are a pure function of (seed, epoch, step, rank), as in data/mix.py.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

NUM_OPS = 14
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE,
 SOLARIZE, AUTOCONTRAST, EQUALIZE) = range(NUM_OPS)
OP_NAMES = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
            "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
SIGNED = frozenset(range(SHEAR_X, SHARPNESS + 1))
GEOMETRIC = frozenset(range(SHEAR_X, ROTATE + 1))
MAX_LEVEL = 30
MAX_CHAIN = 4
# bytes of one image the kernel's LDS plan holds (csrc/randaug.hip: RA_CAP); 224 x 224 x 3 = 150528
MAX_IMAGE_BYTES = 155136


class RandAugPlan(NamedTuple):
    """Host arrays for N images x K ops."""
    op: np.ndarray    # int32 [N, K]
    fval: np.ndarray  # fp32 [N, K]: v, deg or factor (0 where the op has none)
    ival: np.ndarray  # int32 [N, K]: px, bits or thr (0 where the op has none)
    coef: np.ndarray  # int32 [N, K, 6]: a0..a5 of the geometric ops, output (x, y) reads source
    #                   ((a2 + a1 y + a0 x) >> 16, (a5 + a4 y + a3 x) >> 16); zero elsewhere

    def row(self, n: int):
        """The chain of image ``n`` for :func:`apply_pil`: K tuples (op, float parameter, int parameter)."""
        return [(int(o), float(f), int(i)) for o, f, i in zip(self.op[n], self.fval[n], self.ival[n])]


def _fix(v: float) -> int:
    """Geometry.c's FIX: FLOOR(v * 65536.0 + 0.5)."""
    return int(math.floor(v * 65536.0 + 0.5))


def affine_fix16(m):
    """The 16.16 integers ``affine_fixed`` derives from the inverse matrix ``m`` of ``Image.transform``.  A
    matrix without shear terms takes Pillow's ``ImagingScaleAffine`` instead; with the unit scales used
    here its COORD() picks the same source pixels as these integers do."""
    a0, a1, a2, a3, a4, a5 = (float(v) for v in m)
    return (_fix(a0), _fix(a1), _fix(a2 + a0 * 0.5 + a1 * 0.5), _fix(a3), _fix(a4), _fix(a5 + a3 * 0.5 + a4 * 0.5))


def rotate_matrix(deg: float, W: int, H: int):
    """``Image.rotate(deg)``'s inverse matrix about the image centre, line by line as Image.py builds it."""
    angle = -math.radians(deg % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def op_params(op: int, level: int, neg: bool, H: int, W: int):
    """(fp32 parameter, int parameter, a0..a5) of ``op`` at ``level``, negated when ``neg`` and signed."""
    if not 0 <= op < NUM_OPS:
        raise ValueError(f"rand_augment covers op ids 0..{NUM_OPS - 1}, not {op}")
    if not 0 <= level <= MAX_LEVEL:
        raise ValueError(f"RandAugment magnitude {level}: 0..{MAX_LEVEL}")
    f = level / MAX_LEVEL
    s = -1.0 if neg and op in SIGNED else 1.0
    fval, ival, coef = 0.0, 0, (0,) * 6
    if op in (SHEAR_X, SHEAR_Y):
        fval = float(np.float32(s * 0.3 * f))
        coef = affine_fix16((1, fval, 0, 0, 1, 0) if op == SHEAR_X else (1, 0, 0, fval, 1, 0))
    elif op in (TRANSLATE_X, TRANSLATE_Y):
        ival = int(s) * int(f * 150 / 331 * (W if op == TRANSLATE_X else H))
        coef = affine_fix16((1, 0, ival, 0, 1, 0) if op == TRANSLATE_X else (1, 0, 0, 0, 1, ival))
    elif op == ROTATE:
        fval = float(np.float32(s * 30.0 * f))
        # Image.rotate returns a copy at 0 degrees; the identity map says the same
        coef = affine_fix16(rotate_matrix(fval, W, H) if fval % 360.0 != 0 else (1, 0, 0, 0, 1, 0))
    elif op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        fval = float(np.float32(1.0 + s * 0.9 * f))
    elif op == POSTERIZE:
        ival = 8 - round(4 * f)
    elif op == SOLARIZE:
        ival = 255 - round(255 * f)
    return fval, ival, coef


def make_plan(ops, level, neg, H: int, W: int) -> RandAugPlan:
    """The plan of explicit choices: ``ops`` [N, K] op ids, one ``level`` (or [N, K]), ``neg`` [N, K] signs."""
    ops = np.asarray(ops, dtype=np.int64)
    if ops.ndim != 2 or not 1 <= ops.shape[1] <= MAX_CHAIN:
        raise ValueError(f"rand_augment covers 1 <= num_ops <= {MAX_CHAIN} as an [N, num_ops] plan, not {ops.shape}")
    level = np.broadcast_to(np.asarray(level, dtype=np.int64), ops.shape)
    neg = np.broadcast_to(np.asarray(neg, dtype=bool), ops.shape)
    N, K = ops.shape
    plan = RandAugPlan(np.zeros((N, K), np.int32), np.zeros((N, K), np.float32), np.zeros((N, K), np.int32),
                       np.zeros((N, K, 6), np.int32))
    for n in range(N):
        for k in range(K):
            plan.op[n, k] = ops[n, k]
            plan.fval[n, k], plan.ival[n, k], plan.coef[n, k] = op_params(int(ops[n, k]), int(level[n, k]),
                                                                          bool(neg[n, k]), H, W)
    return plan


def identity_plan(n: int, num_ops: int = 1) -> RandAugPlan:
    return make_plan(np.zeros((n, num_ops), np.int64), 0, False, 1, 1)


def check_plan(plan: RandAugPlan, n: int):
    op = np.asarray(plan.op)
    if op.ndim != 2 or op.shape[0] != n or not 1 <= op.shape[1] <= MAX_CHAIN:
        raise ValueError(f"rand_augment covers 1 <= num_ops <= {MAX_CHAIN} for each of the batch's {n} images, "
                         f"not a plan of shape {op.shape}")
    if op.size and (op.min() < 0 or op.max() >= NUM_OPS):
        raise ValueError(f"rand_augment covers op ids 0..{NUM_OPS - 1}, not {int(op.min())}..{int(op.max())}")


def pack(plan: RandAugPlan, pin: bool = False) -> torch.Tensor:
    """int32 [N, K, 8] = {op, parameter, a0..a5}; the parameter is the fp32 bit pattern of ``fval`` for
    the enhance ops and ``ival`` otherwise.  ``pin=True`` allocates it in pinned host memory."""
    N, K = plan.op.shape
    host = torch.empty((N, K, 8), dtype=torch.int32, pin_memory=pin)
    buf = host.numpy()
    buf[:, :, 0] = plan.op
    enh = (plan.op >= BRIGHTNESS) & (plan.op <= SHARPNESS)
    buf[:, :, 1] = np.where(enh, np.ascontiguousarray(plan.fval, dtype=np.float32).view(np.int32), plan.ival)
    buf[:, :, 2:] = plan.coef
    return host


def plan_to_device(plan: RandAugPlan, device) -> torch.Tensor:
    """:func:`pack` on ``device``: one pinned buffer, one ``non_blocking`` copy on the current stream, no
    synchronisation (torch's caching host allocator reuses the block only after the copy has completed)."""
    device = torch.device(device)
    host = pack(plan, pin=device.type == "cuda")
    return host.to(device, non_blocking=True) if device.type == "cuda" else host


def apply_pil(img, ops_row):
    """The definition: ``ops_row`` (:meth:`RandAugPlan.row`) applied in order to an RGB PIL image."""
    from PIL import Image, ImageEnhance, ImageOps

    def affine(m):
        return img.transform(img.size, Image.AFFINE, m, Image.NEAREST, fillcolor=(0, 0, 0))

    for op, fval, ival in ops_row:
        if op == IDENTITY:
            pass
        elif op == SHEAR_X:
            img = affine((1, fval, 0, 0, 1, 0))
        elif op == SHEAR_Y:
            img = affine((1, 0, 0, fval, 1, 0))
        elif op == TRANSLATE_X:
            img = affine((1, 0, ival, 0, 1, 0))
        elif op == TRANSLATE_Y:
            img = affine((1, 0, 0, 0, 1, ival))
        elif op == ROTATE:
            img = img.rotate(fval, Image.NEAREST, fillcolor=(0, 0, 0))
        elif op == BRIGHTNESS:
            img = ImageEnhance.Brightness(img).enhance(fval)
        elif op == COLOR:
            img = ImageEnhance.Color(img).enhance(fval)
        elif op == CONTRAST:
            img = ImageEnhance.Contrast(img).enhance(fval)
        elif op == SHARPNESS:
            img = ImageEnhance.Sharpness(img).enhance(fval)
        elif op == POSTERIZE:
            img = ImageOps.posterize(img, ival)
        elif op == SOLARIZE:
            img = ImageOps.solarize(img, ival)
        elif op == AUTOCONTRAST:
            img = ImageOps.autocontrast(img)
        elif op == EQUALIZE:
            img = ImageOps.equalize(img)
        else:
            raise ValueError(f"rand_augment covers op ids 0..{NUM_OPS - 1}, not {op}")
    return img


def apply_pil_batch(imgs: torch.Tensor, plan: RandAugPlan) -> torch.Tensor:
    """:func:`apply_pil` over a uint8 [N, H, W, 3] host batch."""
    from PIL import Image

    out = torch.empty_like(imgs)
    for n in range(imgs.shape[0]):
        res = apply_pil(Image.fromarray(imgs[n].numpy()), plan.row(n))
        out[n] = torch.from_numpy(np.asarray(res, dtype=np.uint8).copy())
    return out


class RandAugSampler:
    def __init__(self, num_ops: int = 2, magnitude: int = 9, seed: int = 0, rank: int = 0):
        if not 1 <= int(num_ops) <= MAX_CHAIN:
            raise ValueError(f"RandAugment num_ops {num_ops}: 1..{MAX_CHAIN}")
        if not 0 <= int(magnitude) <= MAX_LEVEL:
            raise ValueError(f"RandAugment magnitude {magnitude}: 0..{MAX_LEVEL}")
        self.num_ops, self.magnitude, self.seed, self.rank = int(num_ops), int(magnitude), int(seed), int(rank)

    def plan(self, N: int, H: int, W: int, step: int, epoch: int = 0, rank: int = None) -> RandAugPlan:
        """The host plan of batch ``step`` of ``epoch`` on ``rank`` (default: the sampler's own)."""
        rank = self.rank if rank is None else rank
        mask = (1 << 64) - 1
        # key word 1 carries the rank as data/mix.py does, xor a constant so the two samplers of a run
        # with one seed do not share a stream
        rng = np.random.Generator(np.random.Philox(key=[self.seed & mask, (int(rank) ^ 0x52414E44415547) & mask],
                                                   counter=[0, 0, int(step) & mask, int(epoch) & mask]))
        ops = rng.integers(0, NUM_OPS, size=(N, self.num_ops))
        neg = rng.integers(0, 2, size=(N, self.num_ops)).astype(bool)
        return make_plan(ops, self.magnitude, neg, H, W)


def parse_flag(text: str) -> RandAugSampler:
    """``--randaugment N,M`` -> a sampler with ``num_ops = N`` and ``magnitude = M`` (the seed is set by the caller)."""
    parts = str(text).split(",")
    try:
        n, m = (int(p) for p in parts)
    except ValueError:
        raise ValueError(f"--randaugment {text!r}: two integers N,M (ops per image, magnitude 0..{MAX_LEVEL})") from None
    return RandAugSampler(n, m)
