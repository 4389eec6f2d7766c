"""fp64 oracle of the shard loader's affine warp (csrc/augment.hip:warp_crop_kernel,
csrc/host/loader.cpp:affine_matrix), written from the definition and from nothing in the package.

One image: an ``h x w`` box of a stored record is resized to an ``Sh x Sw`` canvas, the canvas is
rotated by ``theta`` degrees about its centre (PIL ``Image.rotate``: counter-clockwise, cos/sin
rounded to 15 digits), flipped, and ``Ho x Wo`` pixels are cut at offset ``(dx, dy)``; whatever
falls outside the canvas is 0.  For output pixel ``(ox, oy)``::

    ox' = Wo-1-ox if flip else ox
    p   = (ox' + 0.5 + dx, oy + 0.5 + dy)               canvas position of the pixel centre
    a   = -theta * pi / 180,  c = (Sw/2, Sh/2)
    u   = cx + cos a (px-cx) + sin a (py-cy)            canvas position before the rotation
    v   = cy - sin a (px-cx) + cos a (py-cy)
    sx  = u * w/Sw - 0.5,  sy = v * h/Sh - 0.5          box position, pixel k centred at k
    inside  <=>  -0.5 <= sx < w-0.5 and -0.5 <= sy < h-0.5   (<=> 0 <= u < Sw and 0 <= v < Sh)

Inside, the value is bilinear at ``(clamp(sx, 0, w-1), clamp(sy, 0, h-1))`` with taps clamped to
the box, rounded half up.  ``nearest=True`` reads box pixel ``(floor(u w/Sw), floor(v h/Sh))``
instead -- PIL's NEAREST lookup -- and exists only to pin the geometry against PIL, whose rotation
is nearest-neighbour.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

# |fp32 - fp64| of a source coordinate, in canvas pixels: the terms of sx are below 512 in
# magnitude (fp32 ulp 6e-5 at 512) and the kernel spends two multiplies and two adds on each, so
# an fp32 evaluation may put a pixel whose exact (u, v) is within 2^-10 px of a canvas edge on the
# other side of it.  Fill/sample agreement is not asserted inside this band.
BAND = 2.0 ** -10


@dataclass(frozen=True)
class Geo:
    h: int          # box
    w: int
    Sh: int         # canvas
    Sw: int
    Ho: int         # output
    Wo: int
    dx: float       # crop offset on the canvas (CenterCrop: int(round((S - out) / 2.0)))
    dy: float
    theta: float = 0.0
    flip: bool = False


def center_offset(S, out):
    return int(round((S - out) / 2.0))


def _trig(theta):
    a = -math.radians(theta)
    return round(math.cos(a), 15), round(math.sin(a), 15)


def coords(g: Geo):
    """(u, v, sx, sy), each float64 [Ho, Wo]."""
    ox = np.arange(g.Wo, dtype=np.float64)[None, :]
    oy = np.arange(g.Ho, dtype=np.float64)[:, None]
    oxp = (g.Wo - 1 - ox) if g.flip else ox
    px, py = oxp + 0.5 + g.dx, oy + 0.5 + g.dy
    ca, sa = _trig(g.theta)
    cx, cy = g.Sw / 2.0, g.Sh / 2.0
    u = cx + ca * (px - cx) + sa * (py - cy)
    v = cy - sa * (px - cx) + ca * (py - cy)
    return u, v, u * g.w / g.Sw - 0.5, v * g.h / g.Sh - 0.5


def inside(g: Geo):
    _, _, sx, sy = coords(g)
    return (sx >= -0.5) & (sx < g.w - 0.5) & (sy >= -0.5) & (sy < g.h - 0.5)


def band(g: Geo, width=BAND):
    """Pixels whose exact (u, v) lies within ``width`` canvas pixels of a canvas edge."""
    u, v, _, _ = coords(g)
    return ((np.abs(u) < width) | (np.abs(u - g.Sw) < width) | (np.abs(v) < width) | (np.abs(v - g.Sh) < width))


def warp(box: np.ndarray, g: Geo, nearest=False):
    """uint8 [Ho, Wo, 3] of the uint8 [h, w, 3] ``box``."""
    assert box.shape == (g.h, g.w, 3)
    u, v, sx, sy = coords(g)
    ins = inside(g)
    img = box.astype(np.float64)
    if nearest:
        xi = np.clip(np.floor(u * g.w / g.Sw), 0, g.w - 1).astype(np.int64)
        yi = np.clip(np.floor(v * g.h / g.Sh), 0, g.h - 1).astype(np.int64)
        val = img[yi, xi]
    else:
        x = np.clip(sx, 0, g.w - 1)
        y = np.clip(sy, 0, g.h - 1)
        x0 = np.minimum(np.floor(x), g.w - 1).astype(np.int64)
        y0 = np.minimum(np.floor(y), g.h - 1).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, g.w - 1), np.minimum(y0 + 1, g.h - 1)
        lx, ly = (x - x0)[..., None], (y - y0)[..., None]
        top = img[y0, x0] * (1 - lx) + img[y0, x1] * lx
        bot = img[y1, x0] * (1 - lx) + img[y1, x1] * lx
        val = np.floor(top * (1 - ly) + bot * ly + 0.5)
    return np.where(ins[..., None], np.clip(val, 0, 255), 0).astype(np.uint8)


def matrix(g: Geo) -> np.ndarray:
    """The 2x3 map (sx, sy) = M (ox, oy, 1) of the definition, composed in double, as float32 [6]."""
    ca, sa = _trig(g.theta)
    cx, cy, kx, ky = g.Sw / 2.0, g.Sh / 2.0, g.w / g.Sw, g.h / g.Sh
    fs, f0 = (-1.0, g.Wo - 1.0) if g.flip else (1.0, 0.0)
    px0, py0 = f0 + 0.5 + g.dx - cx, 0.5 + g.dy - cy
    return np.array([ca * fs * kx, sa * kx, (cx + ca * px0 + sa * py0) * kx - 0.5,
                     -sa * fs * ky, ca * ky, (cy - sa * px0 + ca * py0) * ky - 0.5]).astype(np.float32)


# ----------------------------------------------------------------------------- shared batches
def _pack(recs, boxes, geos):
    """Records (uint8 [H, W, 3]) + boxes (y0, x0) + geometries -> (src, meta, xf) as the ops take them."""
    metas, xfs, off = [], [], 0
    for rec, (y0, x0), g in zip(recs, boxes, geos):
        H, W = rec.shape[:2]
        metas.append([off, H, W, y0, x0, g.h, g.w, int(g.flip)])
        xfs.append(list(matrix(g)) + [g.theta, 0.0])
        off += rec.size
    src = torch.from_numpy(np.concatenate([r.reshape(-1) for r in recs]))
    return src, torch.tensor(metas, dtype=torch.int64), torch.tensor(np.array(xfs, dtype=np.float32))


def random_batch(Ho, Wo, B=9, seed=0):
    """B records of 8-90 px with random boxes; canvases larger and smaller than the output (so crop
    offsets of both signs), angles 0 / +-15 / 90 and both flips.  The 90-degree canvases have
    Sh + Sw even: with an odd sum a whole output row sits exactly on a canvas edge."""
    rng = np.random.default_rng(seed)
    recs, boxes, geos = [], [], []
    for b in range(B):
        H, W = int(rng.integers(8, 91)), int(rng.integers(8, 91))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        theta = (0.0, 15.0, -15.0, 90.0)[b % 4]
        Sh, Sw = Ho + int(rng.integers(-6, 40)), Wo + int(rng.integers(-6, 40))
        if theta == 90.0 and (Sh + Sw) % 2:
            Sw += 1
        if b % 3 == 2:   # RandomCrop-style offsets, reaching past the canvas on either side
            dx, dy = float(rng.integers(-5, 6)), float(rng.integers(-5, 6))
        else:
            dx, dy = float(center_offset(Sw, Wo)), float(center_offset(Sh, Ho))
        recs.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        boxes.append((y0, x0))
        geos.append(Geo(h, w, Sh, Sw, Ho, Wo, dx, dy, theta, bool((b // 2) % 2)))
    return recs, boxes, geos


def lattice_batch():
    """Geometries whose source positions are integers or half-integers, where fp32 and fp64
    agree bit for bit: the CIFAR chain (scale 1, theta 0, integer offsets in [-4, 4], both flips)
    and 90-degree rotations at scale 1 (square and non-square canvases)."""
    rng = np.random.default_rng(5)
    recs, boxes, geos = [], [], []
    for dy, dx, flip in [(-4, -4, False), (4, 4, True), (-1, 1, True), (0, 0, False), (3, -4, False)]:
        recs.append(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8))
        boxes.append((0, 0))
        geos.append(Geo(32, 32, 32, 32, 32, 32, float(dx), float(dy), 0.0, flip))
    for (h, w), flip, theta in [((32, 32), False, 90.0), ((40, 36), True, 90.0), ((35, 38), False, -90.0),
                                ((33, 33), True, 180.0)]:
        recs.append(rng.integers(0, 256, (h + 3, w + 5, 3), dtype=np.uint8))
        boxes.append((2, 4))
        geos.append(Geo(h, w, h, w, 32, 32, float(center_offset(w, 32)), float(center_offset(h, 32)), theta, flip))
    return recs, boxes, geos


def expected(recs, boxes, geos, nearest=False):
    """Oracle outputs [B, Ho, Wo, 3] plus the inside and band masks [B, Ho, Wo]."""
    outs, ins, bnd = [], [], []
    for rec, (y0, x0), g in zip(recs, boxes, geos):
        outs.append(warp(rec[y0:y0 + g.h, x0:x0 + g.w], g, nearest))
        ins.append(inside(g))
        bnd.append(band(g))
    return np.stack(outs), np.stack(ins), np.stack(bnd)


def check_against_oracle(got: torch.Tensor, recs, boxes, geos):
    """The criteria shared by the reference-math and the kernel tests: outside the band fill and
    sample agree with the oracle everywhere and every channel is within one level; inside it a
    pixel may be fill on one side and a sample on the other, and only there.  Returns the
    fraction of pixels in the band."""
    ref, ins, bnd = expected(recs, boxes, geos)
    assert bnd.mean() <= 1e-3, f"band holds {bnd.mean():.2e} of the pixels"  # from the oracle alone
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.uint8
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32)).max(-1)
    print(f"max level difference outside the band {d[~bnd].max()}, band pixels {int(bnd.sum())} of {bnd.size}, "
          f"exact {float((d == 0).mean()):.5f}")
    assert d[~bnd].max() <= 1
    # far outside: exactly 0 in all three channels
    assert got[~ins & ~bnd].max(initial=0) == 0
    # a band pixel is either within one level of the oracle's sample or the fill
    assert ((d <= 1) | (got.max(-1) == 0) | ~ins)[bnd].all()
    return float(bnd.mean())
