"""The `pil` resampling mode of the shard loader, GPU half: resample_crop_kernel and
rotate_nearest_crop_kernel (csrc/augment.hip) against the integer reference math (ops/_ref.py) and
against Pillow itself, ``torch.equal`` with no tolerance; then a ShardLoader epoch per preset in
`pil` mode against the PIL chain built from its own meta, and in `fast` mode against the ops it
has always used."""
import math

import numpy as np
import pytest
import torch

from ddp_classification_pytorch_amd.data import shards
from ddp_classification_pytorch_amd.ops import functional as Fn

from . import resample_cases as rc

pytestmark = pytest.mark.gpu


def _check(imgs, src, meta, geo, Ho, Wo, bicubic=False):
    """GPU == reference math == Pillow, for a resample (+ rotate when geo says so) batch."""
    out = Fn.resample_exact(src.cuda(), meta, geo, Ho, Wo, bicubic).cpu()
    ref = Fn.resample_exact(src, meta, geo, Ho, Wo, bicubic)
    assert out.shape == (len(imgs), Ho, Wo, 3) and out.dtype == torch.uint8
    assert torch.equal(out, ref), [b for b in range(len(imgs)) if not torch.equal(out[b], ref[b])]
    rot = bool(geo[:, 10].any())
    for b, th in enumerate(rc.angles(geo)):
        Sh, Sw, dy, dx = geo[b, :4].tolist()
        pil = rc.pil_op_chain(imgs[b], meta[b].tolist(), Sh, Sw, dy, dx, Ho, Wo, bicubic, th if rot else None)
        assert np.array_equal(out[b].numpy(), pil), (b, meta[b].tolist(), geo[b].tolist())


@pytest.fixture(scope="module")
def batch():
    imgs = rc.records()
    src, meta = rc.pack(imgs)
    meta[:, 3:7] = torch.tensor([[1, 2, a.shape[0] - 3, a.shape[1] - 2] for a in imgs])  # boxes inside the records
    meta[::2, 7] = 1
    return imgs, src, meta


@pytest.mark.parametrize("bicubic", [False, True], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("Ho,Wo", [(32, 32), (24, 40)])
def test_resample_kernel_scales_windows_flips(batch, Ho, Wo, bicubic):
    """Canvases from 1/7 to 7x the box per axis, windows of both offset signs and partly off the
    canvas, both flips."""
    imgs, src, meta = batch
    fac = [1 / 7, 1 / 3, 1 / 2, 1.0, 1.5, 3.0, 7.0]
    B = len(imgs)
    Sh = [math.ceil(int(meta[b, 5]) * fac[b % 7] - 1e-9) for b in range(B)]
    Sw = [math.ceil(int(meta[b, 6]) * fac[(b * 3 + 2) % 7] - 1e-9) for b in range(B)]
    dy = [(-5, 0, min(3, Sh[b] - 1), max(Sh[b] - 10, 1 - Ho))[b % 4] for b in range(B)]
    dx = [(min(3, Sw[b] - 1), max(Sw[b] - 10, 1 - Wo), -5, 0)[b % 4] for b in range(B)]
    _check(imgs, src, meta, rc.make_geo(B, Sh, Sw, dy, dx), Ho, Wo, bicubic)


@pytest.mark.parametrize("Wo", [40, 130])  # not a multiple of the wave; more than one 128-column tile
@pytest.mark.parametrize("Ho", [15, 16, 17])  # the row tile, one less, one more
def test_resample_kernel_tile_edges(Ho, Wo):
    """90 rows into 17 (5.3x): one 16-row tile needs more source rows than the staging buffer holds,
    so the tile runs in several groups; 8 columns into 130 is a 16x upscale across two column tiles."""
    allr = rc.records()
    imgs = [allr[11], allr[12], allr[13], allr[7]]  # 90 x 8, 8 x 90, 57 x 23, 40 x 40
    src, meta = rc.pack(imgs)
    meta[1::2, 7] = 1
    geo = rc.make_geo(4, [17, 20, Ho, 16], [Wo, 17, 130, 40], [0, 2, 0, -1], [0, -3, 0, 1])
    _check(imgs, src, meta, geo, Ho, Wo, bicubic=Ho != 16)


def test_resample_kernel_eight_times_and_one_pixel_boxes():
    allr = rc.records()
    imgs = [allr[11], allr[12], allr[7], allr[7], allr[7]]
    src, meta = rc.pack(imgs)
    meta[0, 3:7] = torch.tensor([1, 0, 88, 8])   # 88 rows into 11: exactly 8x
    meta[1, 3:7] = torch.tensor([0, 2, 8, 88])
    meta[2, 3:7] = torch.tensor([3, 5, 30, 1])   # a 1-pixel-wide box
    meta[3, 3:7] = torch.tensor([7, 4, 1, 33])   # a 1-pixel-high box
    meta[4, 3:7] = torch.tensor([9, 9, 1, 1])
    meta[2:, 7] = 1
    geo = rc.make_geo(5, [11, 33, 32, 32, 20], [33, 11, 32, 32, 20], [0, 0, 0, 0, -2], [0, 0, 0, 0, -3])
    for bicubic in (False, True):
        _check(imgs, src, meta, geo, 32, 32, bicubic)


@pytest.mark.parametrize("window", [(32, 30, 4, 3), (24, 40, -2, 10)], ids=["centre", "partly-off"])
def test_cdr_chain_small(batch, window):
    """resize -> nearest rotation -> flip -> window at +-15 degrees, 0, 1e-3 and angles between."""
    imgs, src, meta = batch
    Ho, Wo, dy, dx = window
    B = len(imgs)
    th = [15.0, -15.0, 0.0, 1e-3, -1e-3, 7.25, -3.5, 14.999, 0.5, -9.0, 2.0, -14.0, 11.0, -0.25][:B]
    _check(imgs, src, meta, rc.make_geo(B, 40, 36, dy, dx, th), Ho, Wo)


def test_production_configuration_cdr_and_plc():
    """One 256 x 300 record into the real 256 canvas and 224 output: CDR's rotate chain and PLC's
    bicubic stretch, flipped and not."""
    rng = np.random.default_rng(2)
    rec = rng.integers(0, 256, (256, 300, 3), dtype=np.uint8)
    imgs = [rec, rec]
    src, meta = rc.pack(imgs)
    meta[1, 7] = 1
    _check(imgs, src, meta, rc.make_geo(2, 256, 256, 16, 16), 224, 224, bicubic=True)  # PLC
    meta[:, 3:7] = torch.tensor([[10, 20, 200, 260], [0, 0, 256, 300]])
    _check(imgs, src, meta, rc.make_geo(2, 256, 256, 16, 16, [7.3, -15.0]), 224, 224)  # CDR


def test_refusals_on_the_device_path(batch):
    imgs, src, meta = batch
    B = len(imgs)
    d = src.cuda()
    with pytest.raises(RuntimeError, match="8x"):
        Fn.resample_crop(d, meta, rc.make_geo(B, 10, 10), 8, 8)
    with pytest.raises(RuntimeError, match="off the canvas"):
        Fn.resample_crop(d, meta, rc.make_geo(B, 30, 30, 30, 0), 8, 8)
    with pytest.raises(RuntimeError):
        Fn.resample_crop(d, meta, rc.make_geo(B, 30, 30)[:1], 8, 8)
    with pytest.raises(RuntimeError):
        Fn.resample_crop(d, meta, rc.make_geo(B, 30, 30), 8, 8, canvas=True)
    bad = meta.clone()
    bad[0, 5] = bad[0, 1] + 1  # box taller than its record
    with pytest.raises(RuntimeError):
        Fn.resample_crop(d, bad, rc.make_geo(B, 30, 30), 8, 8)
    with pytest.raises(RuntimeError, match="off the canvas"):
        Fn.rotate_nearest_crop(torch.zeros((B, 30, 30, 3), dtype=torch.uint8).cuda(), meta,
                               rc.make_geo(B, 30, 30, 0, -8, 1.0), 8, 8)


# ------------------------------------------------------------------ the loader end to end
@pytest.fixture(scope="module")
def shard_path(tmp_path_factory):
    imgs = rc.records()
    p = str(tmp_path_factory.mktemp("resample_gpu") / "r.dcps")
    shards.write_shard(p, [(a, i) for i, a in enumerate(imgs)])
    return p, imgs


def _epoch(ld):
    """One epoch of ``ld`` with the tap on: [(uint8 images, meta, xf / geo / None)] per batch."""
    seen = []
    ld.tap = lambda imgs, meta, extra: seen.append((imgs.cpu(), meta.clone(), None if extra is None else extra.clone()))
    ld.set_epoch(2)
    n = sum(batch[1].numel() for batch in ld)
    torch.cuda.synchronize()
    return seen, n


@pytest.mark.parametrize("train", [True, False], ids=["train", "val"])
@pytest.mark.parametrize("name", rc.PRESETS)
def test_shard_loader_pil_mode_delivers_the_pil_chain(shard_path, name, train):
    path, imgs = shard_path
    aug, size = shards.aug_preset(name, train, 224, resample="pil")
    ld = shards.ShardLoader(path, 8, aug=aug, out_size=size, device="cuda", threads=3, seed=5, resample="pil")
    try:
        seen, n = _epoch(ld)
    finally:
        ld.close()
    assert n == len(imgs) and len(seen) == 2
    k = 0
    for out, meta, geo in seen:
        assert geo is not None and geo.dtype == torch.int32
        for b, th in enumerate(rc.angles(geo)):
            ref = rc.pil_spec_chain(imgs[k], meta[b].tolist(), th, aug, size, size)
            assert np.array_equal(out[b].numpy(), ref), (name, train, k)
            k += 1


@pytest.mark.parametrize("name", ["nested", "cdr", "plc", "cifar"])
def test_shard_loader_fast_mode_is_unchanged(shard_path, name):
    """Without the flag the loader runs what it ran before: the plain gather + crop_resize, or the
    affine gather + warp_crop, bit for bit -- and in `pil` mode the pad-crop keeps the affine route."""
    path, imgs = shard_path
    aug, size = shards.aug_preset(name, True, 224)
    size = 8 if name == "cifar" else size  # the pad-crop needs records >= the output
    n = len(imgs)
    for mode in ("fast", "pil") if name == "cifar" else ("fast",):
        ld = shards.ShardLoader(path, n, aug=aug, out_size=size, device="cuda", threads=3, seed=5, resample=mode)
        try:
            seen, _ = _epoch(ld)
            g = ld.gather
            idx = torch.arange(n, dtype=torch.int64)
            buf = torch.empty(n * int(g.hdr["max_bytes"]), dtype=torch.uint8)
            meta, labels = torch.empty((n, 8), dtype=torch.int64), torch.empty(n, dtype=torch.int64)
            xf = torch.empty((n, 8), dtype=torch.float32) if aug.affine else None
            g.wait(g.submit(idx, buf, meta, labels, aug, 5, 2, xf, (size, size)))
        finally:
            ld.close()
        out, m, extra = seen[0]
        assert torch.equal(m, meta)
        if xf is None:
            assert extra is None
            want = Fn.crop_resize(buf.cuda(), meta, size, size)
        else:
            assert torch.equal(extra, xf)
            want = Fn.warp_crop(buf.cuda(), meta, xf, size, size)
        assert torch.equal(out, want.cpu())
