"""CPU half of the shard loader's affine route: the fp32 reference math (ops/_ref.py:warp_crop)
against the fp64 oracle, the host entry point dcpl_submit_affine (determinism, ranges, the matrix
it composes), the new presets through ShardLoader, and the CLI path for CDR and CIFAR."""
import os

import numpy as np
import pytest
import torch

from ddp_classification_pytorch_amd.data import ShardSampler, make_fake_image_folder
from ddp_classification_pytorch_amd.data.shards import (MODE_CENTER, MODE_PADCROP, MODE_RRC, MODE_STRETCH, MODE_WHOLE,
                                                        AugSpec, NativeGather, ShardLoader, aug_preset, write_shard)
from ddp_classification_pytorch_amd.ops import _ref

from . import warp_oracle as wo

SIZES = [(37, 53), (32, 32), (224, 224)]


# ----------------------------------------------------------------------------- reference math
@pytest.mark.parametrize("Ho,Wo", SIZES)
def test_ref_warp_matches_oracle(Ho, Wo):
    recs, boxes, geos = wo.random_batch(Ho, Wo)
    src, meta, xf = wo._pack(recs, boxes, geos)
    wo.check_against_oracle(_ref.warp_crop(src, meta, xf, Ho, Wo), recs, boxes, geos)


def test_ref_warp_exact_on_the_lattice():
    recs, boxes, geos = wo.lattice_batch()
    src, meta, xf = wo._pack(recs, boxes, geos)
    ref, ins, _ = wo.expected(recs, boxes, geos)
    out = _ref.warp_crop(src, meta, xf, 32, 32)
    assert np.array_equal(out.numpy(), ref)
    assert 0.3 < ins[:5].mean() < 1 and ins[5].all()  # the padded border is in the cases


def test_ref_warp_nan_matrix_is_fill():
    recs, boxes, geos = wo.lattice_batch()
    src, meta, xf = wo._pack(recs[:2], boxes[:2], geos[:2])
    xf[0, 2] = float("nan")
    xf[1, :6] = float("inf")
    assert _ref.warp_crop(src, meta, xf, 32, 32).max().item() == 0


# ----------------------------------------------------------------------------- host entry point
def _images(n, lo=20, hi=70, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (int(rng.integers(lo, hi)), int(rng.integers(lo, hi)), 3), dtype=np.uint8), i % 5)
            for i in range(n)]


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    imgs = _images(37)
    p = str(tmp_path_factory.mktemp("warp") / "s.dcps")
    assert write_shard(p, imgs) == 37
    return p, imgs


def _gather(p, order, aug, out_hw=None, threads=4, seed=1, epoch=0):
    g = NativeGather(p, threads)
    B = len(order)
    buf = torch.zeros(B * int(g.hdr["max_bytes"]), dtype=torch.uint8)  # zeros: the gaps between records compare too
    meta = torch.empty((B, 8), dtype=torch.int64)
    labels = torch.empty(B, dtype=torch.int64)
    xf = torch.full((B, 8), -7.0) if out_hw is not None else None
    t = g.submit(torch.tensor(order, dtype=torch.int64), buf, meta, labels, aug, seed, epoch, xf, out_hw)
    g.wait(t)
    g.close()
    return buf, meta, labels, xf


CDR = AugSpec(MODE_RRC, 0, 0, 0.08, 1.0, 3 / 4, 4 / 3, 0.5, 15.0, 0, 36, 40)
CIFAR = AugSpec(MODE_PADCROP, 0, 0, 1, 1, 1, 1, 0.5, 0.0, 4, 0, 0)
PLC = AugSpec(MODE_STRETCH, 0, 0, 1, 1, 1, 1, 0.5, 0.0, 0, 36, 36)
SPECS = {"cdr": (CDR, (32, 32)), "cifar": (CIFAR, (16, 24)), "plc": (PLC, (32, 32))}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_affine_deterministic_and_keyed_by_seed_epoch_index(shard, name):
    p, _ = shard
    aug, hw = SPECS[name]
    order = list(range(37))
    runs = [_gather(p, order, aug, hw, threads=t, seed=7, epoch=3) for t in (1, 3, 8)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) and torch.equal(r[3], runs[0][3])
    m1, x1 = runs[0][1], runs[0][3]
    other_epoch = _gather(p, order, aug, hw, seed=7, epoch=4)
    other_seed = _gather(p, order, aug, hw, seed=8, epoch=3)
    assert not torch.equal(other_epoch[3], x1) and not torch.equal(other_seed[3], x1)
    # the draws depend on the dataset index, not on the batch position or the batch's composition
    rev = _gather(p, order[::-1], aug, hw, threads=3, seed=7, epoch=3)
    assert torch.equal(rev[1].flip(0)[:, 1:], m1[:, 1:]) and torch.equal(rev[3].flip(0), x1)
    part = _gather(p, [30, 4], aug, hw, seed=7, epoch=3)
    assert torch.equal(part[3], x1[[30, 4]])


def _geo_of(meta_row, xf_row, aug, hw, dx=None, dy=None):
    """The geometry a spec implies for one gathered image, recomputed here from its meta and angle."""
    _, H, W, _, _, h, w, flip = (int(v) for v in meta_row.tolist())
    Ho, Wo = hw
    if aug.mode == MODE_PADCROP:
        Sh, Sw = H, W
    else:
        Sh, Sw = aug.canvas_h or Ho, aug.canvas_w or Wo
        dx, dy = wo.center_offset(Sw, Wo), wo.center_offset(Sh, Ho)
    return wo.Geo(h, w, Sh, Sw, Ho, Wo, float(dx), float(dy), float(xf_row[6]), bool(flip))


def _assert_fp32_equal(got, want):
    """Equal up to the rounding of one fp32 store (the double compositions may differ in their last bit)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.maximum(np.abs(got), np.abs(want)) + 1e-12), (got, want)


@pytest.mark.parametrize("name", ["cdr", "plc"])
def test_affine_matrix_equals_python_recomputation(shard, name):
    p, _ = shard
    aug, hw = SPECS[name]
    order = list(range(37)) * 3
    _, meta, _, xf = _gather(p, order, aug, hw, seed=5, epoch=1)
    assert xf[:, 7].abs().max().item() == 0
    ang = xf[:, 6]
    if aug.rot_deg > 0:
        assert ang.abs().max().item() <= aug.rot_deg and ang.min().item() < -5 and ang.max().item() > 5
        assert ang.unique().numel() > 30
    else:
        assert ang.abs().max().item() == 0
    assert 0.2 < meta[:, 7].float().mean().item() < 0.8
    for b in range(len(order)):
        H, W, y0, x0, h, w = (int(v) for v in meta[b, 1:7])
        assert 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W and h > 0 and w > 0
        if aug.mode == MODE_STRETCH:
            assert (y0, x0, h, w) == (0, 0, H, W)
        _assert_fp32_equal(xf[b, :6].numpy(), wo.matrix(_geo_of(meta[b], xf[b], aug, hw)))


def test_padcrop_offsets_in_range_and_matrix(shard):
    p, imgs = shard
    aug, (Ho, Wo) = SPECS["cifar"]
    order = list(range(37)) * 6
    _, meta, _, xf = _gather(p, order, aug, (Ho, Wo), seed=2, epoch=0)
    seen_lo = seen_hi = 0
    for b, i in enumerate(order):
        H, W = imgs[i][0].shape[:2]
        assert meta[b, 1:7].tolist() == [H, W, 0, 0, H, W] and xf[b, 6].item() == 0
        flip = int(meta[b, 7])
        m = xf[b, :6].tolist()
        # scale 1, no rotation: sx = +-ox + (dx or Wo-1+dx), sy = oy + dy
        assert m[0] == (-1.0 if flip else 1.0) and m[1] == 0 and m[3] == 0 and m[4] == 1.0
        dx, dy = (m[2] - (Wo - 1) if flip else m[2]), m[5]
        assert dx == int(dx) and dy == int(dy)
        # RandomCrop(out, padding=4): top-left corner i in [0, H + 8 - Ho], shifted by the padding
        assert -4 <= dy <= H + 4 - Ho and -4 <= dx <= W + 4 - Wo
        seen_lo += dy == -4 or dx == -4
        seen_hi += dy == H + 4 - Ho or dx == W + 4 - Wo
        _assert_fp32_equal(m, wo.matrix(_geo_of(meta[b], xf[b], aug, (Ho, Wo), dx, dy)))
    assert seen_lo and seen_hi  # both ends of the range are reached
    assert 0.2 < meta[:, 7].float().mean().item() < 0.8


def test_padcrop_of_too_small_an_image_is_an_error(shard):
    p, _ = shard
    with pytest.raises(RuntimeError, match="gather failed"):
        _gather(p, [0, 1, 2], CIFAR, (200, 200))


@pytest.mark.parametrize("aug", [AugSpec(MODE_RRC, 0, 0, 0.08, 1.0, 3 / 4, 4 / 3, 0.5),
                                 AugSpec(MODE_CENTER, 40, 32, 0, 0, 1, 1, 0.0),
                                 AugSpec(MODE_WHOLE, 0, 0, 1, 1, 1, 1, 0.5)], ids=["rrc", "center", "whole"])
def test_plain_spec_gives_the_meta_of_dcpl_submit(shard, aug):
    p, _ = shard
    assert not aug.affine and aug.rot_deg == 0 and aug.pad == 0 and aug.canvas_h == 0
    order = list(range(37))
    buf0, meta0, lab0, _ = _gather(p, order, aug, None, seed=9, epoch=2)
    buf1, meta1, lab1, xf = _gather(p, order, aug, (24, 24), seed=9, epoch=2)
    assert torch.equal(meta0, meta1) and torch.equal(lab0, lab1) and torch.equal(buf0, buf1)
    # ...and its matrix is crop_resize's map: the box scaled onto the output, flipped by meta[7]
    for b in range(37):
        _assert_fp32_equal(xf[b, :6].numpy(), wo.matrix(_geo_of(meta1[b], xf[b], aug, (24, 24))))


def test_affine_spec_without_matrix_buffer_is_rejected(shard):
    p, _ = shard
    with pytest.raises(ValueError, match="xf"):
        _gather(p, [0, 1], CDR, None)


# ----------------------------------------------------------------------------- presets + loader
def test_presets_map_onto_the_modes(monkeypatch):
    monkeypatch.delenv("DCP_SHARD_AFFINE", raising=False)
    a, size = aug_preset("cdr", True)
    assert (a.mode, a.rot_deg, a.canvas_h, a.canvas_w, a.flip_p, size) == (MODE_RRC, 15.0, 256, 256, 0.5, 224)
    assert abs(a.scale_lo - 0.08) < 1e-6 and a.affine
    a, size = aug_preset("cdr", False)
    assert (a.mode, a.resize, a.crop, size) == (MODE_CENTER, 256, 224, 224) and not a.affine
    for name in ("cifar", "cifar10", "cifar100"):
        a, size = aug_preset(name, True)
        assert (a.mode, a.pad, a.flip_p, a.rot_deg, size) == (MODE_PADCROP, 4, 0.5, 0.0, 32) and a.affine
        a, size = aug_preset(name, False)
        assert (a.mode, a.flip_p, size) == (MODE_WHOLE, 0.0, 32) and not a.affine
    a, size = aug_preset("plc", True)
    assert (a.mode, a.canvas_h, a.canvas_w, a.flip_p, size) == (MODE_STRETCH, 256, 256, 0.5, 224)
    assert aug_preset("plc", False)[0].flip_p == 0.0
    for name in ("baseline", "arcface", "nested"):  # today's presets keep the plain route
        assert not aug_preset(name, True)[0].affine and not aug_preset(name, False)[0].affine
    monkeypatch.setenv("DCP_SHARD_AFFINE", "0")
    for name in ("cdr", "cifar", "plc"):
        with pytest.raises(ValueError, match="DCP_SHARD_AFFINE"):
            aug_preset(name, True)
    assert aug_preset("nested", True)[0].mode == MODE_RRC


@pytest.mark.parametrize("name", ["cdr", "cifar", "plc"])
@pytest.mark.parametrize("train", [True, False])
def test_shard_loader_cpu_epoch_new_presets(shard, name, train, monkeypatch):
    monkeypatch.delenv("DCP_SHARD_AFFINE", raising=False)
    p, imgs = shard
    sampler = ShardSampler(list(range(37)), num_replicas=2, rank=1, shuffle=True, seed=4)
    aug, size = aug_preset(name, train=train, size=16)
    assert size == (32 if name == "cifar" else 16)
    size = 16  # records of 20-70 px: RandomCrop(16, padding=4) fits every one
    ld = ShardLoader(p, batch_size=8, sampler=sampler, aug=aug, out_size=size, device="cpu", threads=3, prefetch=2,
                     return_index=True)
    ld.set_epoch(2)
    seen, batches = [], []
    for x, y, idx in ld:
        assert x.shape[1:] == (size, size, 8) and x.dtype == torch.float32 and torch.isfinite(x).all()
        assert x[..., 3:].abs().max().item() == 0
        for lab, i in zip(y.tolist(), idx.tolist()):
            assert lab == imgs[i][1]
        seen += idx.tolist()
        batches.append(x)
    assert seen == list(sampler) and len(seen) == 19 and len(ld) == 3
    again = [x for x, _, _ in ld]  # same (seed, epoch): same pixels
    assert all(torch.equal(a, b) for a, b in zip(batches, again))
    ld.close()


def test_cifar_loader_reproduces_pad_crop_flip_exactly(tmp_path):
    """32x32 records through ShardLoader with the CIFAR preset: every output is the zero-padded
    record cropped at the drawn offset and flipped, pixel for pixel (un-normalised here)."""
    rng = np.random.default_rng(8)
    imgs = [(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8), i) for i in range(10)]
    p = str(tmp_path / "c.dcps")
    write_shard(p, imgs)
    aug, size = aug_preset("cifar", True)
    _, meta, _, xf = _gather(p, list(range(10)), aug, (size, size), seed=3, epoch=1)
    ld = ShardLoader(p, batch_size=10, aug=aug, out_size=size, device="cpu", threads=2, seed=3, mean=(0, 0, 0),
                     std=(1, 1, 1), cpad=3)
    ld.set_epoch(1)
    (x, y), = list(ld)
    ld.close()
    got = torch.round(x * 255).to(torch.uint8).numpy()
    for b in range(10):
        flip = int(meta[b, 7])
        dx, dy = int(xf[b, 2]) - (31 if flip else 0), int(xf[b, 5])
        canvas = np.zeros((40, 40, 3), dtype=np.uint8)
        canvas[4:36, 4:36] = imgs[b][0]
        want = canvas[dy + 4:dy + 36, dx + 4:dx + 36]
        assert np.array_equal(got[b], want[:, ::-1] if flip else want)


# ----------------------------------------------------------------------------- CLI path
def _spy_shard_loaders(monkeypatch):
    from ddp_classification_pytorch_amd.engine import runtime

    seen = []
    real = runtime._shard_loaders

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(runtime, "_shard_loaders", spy)
    return seen


def test_main_cdr_with_shards_uses_the_native_loader(tmp_path, monkeypatch):
    import main as entry
    from tools import pack_shards

    monkeypatch.delenv("DCP_SHARD_AFFINE", raising=False)
    seen = _spy_shard_loaders(monkeypatch)
    root = make_fake_image_folder(str(tmp_path / "food"), num_classes=3, per_class=4, size=48)
    pack_shards.main(["--folder", root, "--short-side", "40", "--workers", "1"])
    out = str(tmp_path / "run")
    entry.main(["--workload", "cdr", "--model", "resnet18", "--data", "shards", "--folder", root,
                "--image-size", "32", "--num-classes", "3", "--batchsize", "4", "--epochs", "1", "--out-dir", out,
                "--device", "cpu", "--log-interval", "100", "--loader-threads", "2"])
    assert os.path.exists(os.path.join(out, "last.pth"))
    assert len(seen) == 1 and seen[0] is not None
    tr_l, va_l = seen[0]
    assert isinstance(tr_l, ShardLoader) and tr_l.aug.rot_deg == 15.0 and tr_l.aug.canvas_h == 36
    assert isinstance(va_l, ShardLoader) and va_l.aug.mode == MODE_CENTER


def test_main_cifar_with_shards_uses_the_native_loader(tmp_path, monkeypatch):
    import main as entry

    monkeypatch.delenv("DCP_SHARD_AFFINE", raising=False)
    seen = _spy_shard_loaders(monkeypatch)
    rng = np.random.default_rng(0)
    for split, n in (("train", 16), ("test", 8)):
        write_shard(str(tmp_path / f"{split}.dcps"),
                    [(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8), i % 10) for i in range(n)])
    out = str(tmp_path / "run")
    entry.main(["--workload", "nested", "--model", "resnet18", "--dataset", "CIFAR10", "--data", "shards",
                "--folder", str(tmp_path), "--batchsize", "4", "--epochs", "1", "--nested", "20", "--warmup-iters", "2",
                "--out-dir", out, "--device", "cpu", "--log-interval", "100", "--loader-threads", "2"])
    assert len(seen) == 1 and seen[0] is not None
    assert seen[0][0].aug.mode == MODE_PADCROP and seen[0][0].out_size == 32
    assert seen[0][1].aug.mode == MODE_WHOLE


def test_affine_switch_restores_the_pil_fallback(tmp_path, monkeypatch):
    """DCP_SHARD_AFFINE=0: _shard_loaders declines CDR again and build_data falls back to PIL workers."""
    from ddp_classification_pytorch_amd.config import parse_args
    from ddp_classification_pytorch_amd.data import DevicePrefetcher
    from ddp_classification_pytorch_amd.engine import runtime

    monkeypatch.setenv("DCP_SHARD_AFFINE", "0")
    for split in ("train", "test"):
        write_shard(str(tmp_path / f"{split}.dcps"), _images(6, 40, 50))
    args = parse_args(["--workload", "cdr", "--model", "resnet18", "--data", "shards", "--folder", str(tmp_path),
                       "--num-classes", "5", "--batchsize", "2", "--workers", "0", "--device", "cpu",
                       "--out-dir", str(tmp_path / "o")])
    rt = runtime.Runtime(0, 0, 1, torch.device("cpu"))
    tr_l, va_l, _, _ = runtime.build_data(args, rt)
    assert isinstance(tr_l, DevicePrefetcher) and isinstance(va_l, DevicePrefetcher)
