"""Shared cases of the `pil` resampling tests (tests/test_resample_ref_cpu.py, test_resample_gpu.py):
hand-built meta / geo batches for the two exact ops, the PIL chain of a loader spec composed from
Pillow calls alone, and the small shard both files load.  Nothing here calls the code under test
except ``_ref.pil_rotate_fix16`` for the six rotation integers of hand-built batches, which
test_resample_ref_cpu.py pins against ``Image.rotate`` itself."""
import struct

import numpy as np
import torch
from PIL import Image

from ddp_classification_pytorch_amd.data import shards
from ddp_classification_pytorch_amd.ops import _ref

PRESETS = ("baseline", "arcface", "nested", "cdr", "plc")


def records(seed=11):
    """8..90 px records: random ones, a square, 9 x 8 and 8 x 9 (Resize(20) gives a long side of
    22.5 before rounding), 30 x 31 (Resize(256) -> 265, and 265 - 224 is odd), a 0/255 image."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(8, 91)), int(rng.integers(8, 91))) for _ in range(7)]
    sizes += [(40, 40), (9, 8), (8, 9), (30, 31), (90, 8), (8, 90), (57, 23)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    imgs[3] = (rng.integers(0, 2, imgs[3].shape) * 255).astype(np.uint8)
    return imgs


def pack(imgs):
    """Gathered buffer + meta rows (whole-record boxes, no flip) as dcpl_submit lays them out."""
    stride = max(a.nbytes for a in imgs)
    src = np.zeros(stride * len(imgs), dtype=np.uint8)
    meta = torch.zeros((len(imgs), 8), dtype=torch.int64)
    for b, a in enumerate(imgs):
        src[b * stride:b * stride + a.nbytes] = a.reshape(-1)
        meta[b] = torch.tensor([b * stride, a.shape[0], a.shape[1], 0, 0, a.shape[0], a.shape[1], 0])
    return torch.from_numpy(src), meta


def make_geo(B, Sh, Sw, dy=0, dx=0, theta=None):
    """geo rows for hand-built batches; ``theta`` (one angle or a list) adds the rotate step."""
    geo = torch.zeros((B, 12), dtype=torch.int32)
    for b in range(B):
        sh = Sh[b] if isinstance(Sh, (list, tuple)) else Sh
        sw = Sw[b] if isinstance(Sw, (list, tuple)) else Sw
        geo[b, 0], geo[b, 1] = sh, sw
        geo[b, 2] = dy[b] if isinstance(dy, (list, tuple)) else dy
        geo[b, 3] = dx[b] if isinstance(dx, (list, tuple)) else dx
        th = 0.0 if theta is None else float(np.float32(theta[b] if isinstance(theta, (list, tuple)) else theta))
        geo[b, 4:10] = torch.tensor(_ref.pil_rotate_fix16(th, sh, sw), dtype=torch.int32)
        geo[b, 10] = 0 if theta is None else 1
        geo[b, 11] = struct.unpack("<i", struct.pack("<f", th))[0]
    return geo


def angles(geo):
    """The float32 angles a geo tensor carries (column 11 holds their bits)."""
    return geo[:, 11].contiguous().view(torch.float32).tolist()


def pil_window(img, dy, dx, Ho, Wo):
    return img.crop((dx, dy, dx + Wo, dy + Ho))  # Image.crop fills 0 outside the image


def pil_op_chain(rec, m, Sh, Sw, dy, dx, Ho, Wo, bicubic=False, theta=None):
    """crop -> resize -> [rotate] -> [transpose] -> crop, from Pillow calls alone."""
    _, _, _, y0, x0, h, w, flip = (int(v) for v in m)
    img = Image.fromarray(rec).crop((x0, y0, x0 + w, y0 + h))
    img = img.resize((Sw, Sh), Image.BICUBIC if bicubic else Image.BILINEAR)
    if theta is not None:
        img = img.rotate(theta, resample=Image.NEAREST)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(pil_window(img, dy, dx, Ho, Wo))


def pil_spec_chain(rec, m, theta, aug, Ho, Wo):
    """What the transform pipeline a loader spec stands for computes on record ``rec`` with the box
    and flip of meta row ``m`` and the angle ``theta``: Resize / CenterCrop roundings as
    data/transforms.py (and torchvision) write them, every pixel from Pillow."""
    H, W = rec.shape[:2]
    if aug.mode == shards.MODE_CENTER:  # transforms.Resize(int)
        if W <= H:
            Sw, Sh = aug.resize, int(round(aug.resize * H / W))
        else:
            Sw, Sh = int(round(aug.resize * W / H)), aug.resize
    else:
        Sh, Sw = aug.canvas_h or Ho, aug.canvas_w or Wo
    dy, dx = int(round((Sh - Ho) / 2.0)), int(round((Sw - Wo) / 2.0))  # transforms.CenterCrop
    return pil_op_chain(rec, m, Sh, Sw, dy, dx, Ho, Wo, aug.filter == 1, theta if aug.rot_deg > 0 else None)


def small_specs():
    """Specs small enough that 8..90 px records are DOWNscaled through the entry point, up to ~4.5x:
    an RRC -> rotate -> flip -> centre-crop chain, a bicubic stretch, and Resize(20) + CenterCrop(16)
    (the 9 x 8 record's long side is 22.5 before rounding: half to even gives 22)."""
    A = shards.AugSpec
    return {"rot_small": (A(shards.MODE_RRC, 0, 0, 0.3, 1.0, 3 / 4, 4 / 3, 0.5, 15.0, 0, 20, 24), (16, 18)),
            "stretch_bicubic": (A(shards.MODE_STRETCH, 0, 0, 1, 1, 1, 1, 0.5, 0.0, 0, 21, 20, 1), (16, 17)),
            "center_small": (A(shards.MODE_CENTER, 20, 16, 0, 0, 1, 1, 0.0), (16, 16)),
            "whole_small": (A(shards.MODE_WHOLE, 0, 0, 1, 1, 1, 1, 0.5), (12, 12))}
