"""The `pil` resampling mode of the shard loader, CPU half: the integer reference math of the two
exact ops (ops/_ref.py: resample_crop, rotate_nearest_crop) and the exact entry point of the native
loader (csrc/host/loader.cpp:dcpl_submit_exact) against Pillow itself, ``np.array_equal`` with no
tolerance and nothing left out."""
import numpy as np
import pytest
import torch
from PIL import Image

from ddp_classification_pytorch_amd.data import shards
from ddp_classification_pytorch_amd.data.transforms import build_transform
from ddp_classification_pytorch_amd.ops import _ref
from ddp_classification_pytorch_amd.ops import functional as Fn

from . import resample_cases as rc


def _resize_cases():
    rng = np.random.default_rng(5)
    cases = []
    for i in range(220):
        h, w = int(rng.integers(1, 121)), int(rng.integers(1, 121))
        Sh, Sw = max(int(rng.integers(1, 71)), -(-h // 8)), max(int(rng.integers(1, 71)), -(-w // 8))
        if i % 10 == 0:
            Sh = h  # one axis unchanged
        if i % 10 == 5:
            Sw = w
        cases.append((h, w, Sh, Sw, i % 3 == 0))
    cases += [(1, 77, 5, 31, False), (77, 1, 31, 5, False), (1, 77, 1, 12, False), (77, 1, 12, 1, False),
              (1, 1, 7, 9, False), (120, 120, 15, 15, False), (120, 96, 15, 12, False), (119, 3, 15, 70, False)]
    return cases


@pytest.mark.parametrize("bicubic", [False, True], ids=["bilinear", "bicubic"])
def test_resize_equals_pillow(bicubic):
    rng = np.random.default_rng(6)
    for h, w, Sh, Sw, binary in _resize_cases():
        img = ((rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8) if binary
               else rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        ref = np.asarray(Image.fromarray(img).resize((Sw, Sh), Image.BICUBIC if bicubic else Image.BILINEAR))
        got = _ref.pil_resize(torch.from_numpy(img), Sh, Sw, bicubic).numpy()
        assert np.array_equal(got, ref), (h, w, Sh, Sw, binary)


def test_resample_crop_op_windows_and_flips():
    """The op itself on a batch: per-image canvases, windows of both offset signs, partly off the
    canvas, both flips, both filters."""
    imgs = rc.records()
    src, meta = rc.pack(imgs)
    B = len(imgs)
    meta[:, 3:7] = torch.tensor([[1, 2, a.shape[0] - 3, a.shape[1] - 2] for a in imgs])  # boxes inside the records
    meta[::2, 7] = 1
    Sh = [13 + 5 * b for b in range(B)]
    Sw = [70 - 4 * b for b in range(B)]
    dy = [(-3, 0, 4, 9)[b % 4] for b in range(B)]
    dx = [(5, -6, 0, 2)[b % 4] for b in range(B)]
    geo = rc.make_geo(B, Sh, Sw, dy, dx)
    for bicubic in (False, True):
        out = Fn.resample_crop(src, meta, geo, 24, 40, bicubic)
        for b in range(B):
            ref = rc.pil_op_chain(imgs[b], meta[b].tolist(), Sh[b], Sw[b], dy[b], dx[b], 24, 40, bicubic)
            assert np.array_equal(out[b].numpy(), ref), (b, bicubic)


def test_rotation_equals_pillow():
    rng = np.random.default_rng(7)
    thetas = [0.0, 1e-3, -1e-3, 15.0, -15.0, 90.5, 179.99]
    thetas += [float(rng.uniform(-15, 15)) for _ in range(110)] + [float(rng.uniform(-180, 180)) for _ in range(110)]
    for i, th in enumerate(thetas):
        th = float(np.float32(th))
        Sh, Sw = int(rng.integers(2, 301)), int(rng.integers(2, 301))
        img = rng.integers(0, 256, (Sh, Sw, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).rotate(th, resample=Image.NEAREST))
        meta = torch.zeros((1, 8), dtype=torch.int64)
        got = Fn.rotate_nearest_crop(torch.from_numpy(img)[None], meta, rc.make_geo(1, Sh, Sw, theta=th), Sh, Sw)
        assert np.array_equal(got[0].numpy(), ref), (Sh, Sw, th)


# ------------------------------------------------------------------ whole chains through the entry point
@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    imgs = rc.records()
    p = str(tmp_path_factory.mktemp("resample") / "r.dcps")
    shards.write_shard(p, [(a, i) for i, a in enumerate(imgs)])
    g = shards.NativeGather(p, threads=3)
    yield g, imgs
    g.close()


def _submit_exact(g, n, aug, out_hw, epoch=3):
    stride = int(g.hdr["max_bytes"])
    idx = torch.arange(n, dtype=torch.int64)
    buf = torch.empty(n * stride, dtype=torch.uint8)
    meta = torch.empty((n, 8), dtype=torch.int64)
    geo = torch.empty((n, 12), dtype=torch.int32)
    labels = torch.empty(n, dtype=torch.int64)
    g.wait(g.submit(idx, buf, meta, labels, aug, 17, epoch, None, out_hw, geo))
    return buf, meta, geo


def _chain_cases():
    cases = [(f"{name}-{'train' if train else 'val'}",) + shards.aug_preset(name, train, 224, resample="pil")
             for name in rc.PRESETS for train in (True, False)]
    return [(n, a, (o, o)) for n, a, o in cases] + [(n, a, o) for n, (a, o) in rc.small_specs().items()]


@pytest.mark.parametrize("name,aug,out_hw", _chain_cases(), ids=[c[0] for c in _chain_cases()])
def test_chain_equals_pillow(shard, name, aug, out_hw):
    g, imgs = shard
    for epoch in (3, 4):  # two sets of draws
        buf, meta, geo = _submit_exact(g, len(imgs), aug, out_hw, epoch)
        out = Fn.resample_exact(buf, meta, geo, out_hw[0], out_hw[1], bicubic=aug.filter == 1)
        for b, th in enumerate(rc.angles(geo)):
            ref = rc.pil_spec_chain(imgs[b], meta[b].tolist(), th, aug, *out_hw)
            assert np.array_equal(out[b].numpy(), ref), (name, b, meta[b].tolist(), geo[b].tolist())
        if aug.rot_deg > 0:
            assert int(geo[:, 10].min()) == 1 and max(abs(t) for t in rc.angles(geo)) <= aug.rot_deg
            assert len({round(t, 6) for t in rc.angles(geo)}) > 1
        else:
            assert int(geo[:, 10].max()) == 0 and not any(rc.angles(geo))


def test_rotate_chain_in_chunks(shard, monkeypatch):
    """resample_exact rotates ROTATE_CHUNK canvases at a time: 14 images in chunks of 5 are the same bytes."""
    g, imgs = shard
    aug, out_hw = rc.small_specs()["rot_small"]
    buf, meta, geo = _submit_exact(g, len(imgs), aug, out_hw)
    whole = Fn.resample_exact(buf, meta, geo, *out_hw)
    monkeypatch.setattr(Fn, "ROTATE_CHUNK", 5)
    assert torch.equal(Fn.resample_exact(buf, meta, geo, *out_hw), whole)


@pytest.mark.parametrize("name", ["baseline", "nested", "cdr", "plc"])
def test_deterministic_presets_equal_build_transform(shard, name):
    """The validation presets draw nothing, so the loader's bytes are build_transform's own."""
    g, imgs = shard
    aug, size = shards.aug_preset(name, False, 224, resample="pil")
    buf, meta, geo = _submit_exact(g, len(imgs), aug, (size, size))
    out = Fn.resample_exact(buf, meta, geo, size, size, bicubic=aug.filter == 1)
    tf = build_transform(name, False, 224)
    for b, a in enumerate(imgs):
        assert np.array_equal(out[b].numpy(), tf(Image.fromarray(a))), (name, b)


def test_exact_entry_draws_what_the_affine_entry_draws(shard):
    """Same (seed, epoch, index) streams: box, flip and angle agree with dcpl_submit_affine."""
    g, imgs = shard
    n = len(imgs)
    for name in ("cdr", "plc", "nested"):
        aug, size = shards.aug_preset(name, True, 224)
        _, meta, geo = _submit_exact(g, n, aug, (size, size))
        idx = torch.arange(n, dtype=torch.int64)
        buf = torch.empty(n * int(g.hdr["max_bytes"]), dtype=torch.uint8)
        meta2, xf = torch.empty((n, 8), dtype=torch.int64), torch.empty((n, 8), dtype=torch.float32)
        labels = torch.empty(n, dtype=torch.int64)  # alive until the wait: the pool writes into it
        g.wait(g.submit(idx, buf, meta2, labels, aug, 17, 3, xf, (size, size)))
        assert torch.equal(meta, meta2)
        assert rc.angles(geo) == xf[:, 6].tolist()


def test_center_geometry_roundings(shard):
    g, imgs = shard
    aug, out_hw = rc.small_specs()["center_small"]
    _, meta, geo = _submit_exact(g, len(imgs), aug, out_hw)
    sizes = {(a.shape[0], a.shape[1]): geo[b, :4].tolist() for b, a in enumerate(imgs)}
    assert sizes[(9, 8)] == [22, 20, 3, 2]    # 20 * 9 / 8 = 22.5 -> 22 (half to even); (22 - 16) / 2 = 3
    assert sizes[(8, 9)] == [20, 22, 2, 3]
    assert sizes[(40, 40)] == [20, 20, 2, 2]
    aug, size = shards.aug_preset("nested", False, 224, resample="pil")
    _, meta, geo = _submit_exact(g, len(imgs), aug, (size, size))
    b = [a.shape[:2] for a in imgs].index((30, 31))
    assert geo[b, :4].tolist() == [256, 265, 16, 20]  # (265 - 224) / 2 = 20.5 -> 20
    assert meta[b, 3:7].tolist() == [0, 0, 30, 31]    # the box is the whole record


# ------------------------------------------------------------------ refusals
def test_refusals_are_error_codes_not_crashes(shard):
    g, imgs = shard
    n = len(imgs)
    A = shards.AugSpec
    # more than 8x: the 90-px records into a 10-px canvas; the ticket fails, nothing is truncated
    aug = A(shards.MODE_STRETCH, 0, 0, 1, 1, 1, 1, 0.0, 0.0, 0, 10, 10)
    with pytest.raises(RuntimeError, match="gather failed"):
        _submit_exact(g, n, aug, (8, 8))
    # bad arguments: the pad-crop mode, an unknown mode, an empty output, a negative canvas, Resize(0)
    for bad, hw in [(A(shards.MODE_PADCROP, 0, 0, 1, 1, 1, 1, 0.5, 0.0, 4), (8, 8)),
                    (A(7, 0, 0, 1, 1, 1, 1, 0.5), (8, 8)),
                    (A(shards.MODE_WHOLE, 0, 0, 1, 1, 1, 1, 0.5), (0, 8)),
                    (A(shards.MODE_STRETCH, 0, 0, 1, 1, 1, 1, 0.5, 0.0, 0, -1, 8), (8, 8)),
                    (A(shards.MODE_CENTER, 0, 16, 0, 0, 1, 1, 0.0), (16, 16))]:
        with pytest.raises(ValueError, match="-4"):
            _submit_exact(g, n, bad, hw)
    ok = A(shards.MODE_WHOLE, 0, 0, 1, 1, 1, 1, 0.5)
    idx = torch.arange(n, dtype=torch.int64)
    meta, geo, lab = torch.empty((n, 8), dtype=torch.int64), torch.empty((n, 12), dtype=torch.int32), torch.empty(
        n, dtype=torch.int64)
    with pytest.raises(ValueError, match="-2"):  # capacity
        g.submit(idx, torch.empty(16, dtype=torch.uint8), meta, lab, ok, 1, 0, None, (16, 16), geo)
    with pytest.raises(ValueError, match="-3"):  # index outside the shard
        g.submit(idx + 1, torch.empty(n * int(g.hdr["max_bytes"]), dtype=torch.uint8), meta, lab, ok, 1, 0, None,
                 (16, 16), geo)
    # the ops: > 8x, a window off the canvas on each side, a canvas that is not the output, bad geo
    src, meta = rc.pack([imgs[11], imgs[12]])  # 90 x 8 and 8 x 90
    with pytest.raises(RuntimeError, match="8x"):
        Fn.resample_crop(src, meta, rc.make_geo(2, 11, 30), 8, 8)
    for dy, dx in [(30, 0), (0, 30), (-8, 0), (0, -8)]:
        with pytest.raises(RuntimeError, match="off"):
            Fn.resample_crop(src, meta, rc.make_geo(2, 30, 30, dy, dx), 8, 8)
    with pytest.raises(RuntimeError):
        Fn.resample_crop(src, meta, rc.make_geo(2, 30, 30), 8, 8, canvas=True)
    with pytest.raises(RuntimeError):
        Fn.resample_crop(src, meta, rc.make_geo(2, 30, 30)[:1], 8, 8)
    with pytest.raises(RuntimeError):
        Fn.resample_crop(src, meta, rc.make_geo(2, 0, 30), 8, 8)
    with pytest.raises(RuntimeError, match="off"):
        Fn.rotate_nearest_crop(torch.zeros((2, 30, 30, 3), dtype=torch.uint8), meta, rc.make_geo(2, 30, 30, 30, 0, 1.0),
                               8, 8)


def test_cli_flag_and_environment(monkeypatch):
    from ddp_classification_pytorch_amd import config

    monkeypatch.delenv("DCP_SHARD_RESAMPLE", raising=False)
    assert config.parse_args(["--workload", "cdr"]).shard_resample == "fast"
    assert config.parse_args(["--workload", "cdr", "--shard-resample", "pil"]).shard_resample == "pil"
    monkeypatch.setenv("DCP_SHARD_RESAMPLE", "pil")
    assert config.parse_args(["--workload", "cdr"]).shard_resample == "pil"
    # the flag wins
    assert config.parse_args(["--workload", "cdr", "--shard-resample", "fast"]).shard_resample == "fast"
    monkeypatch.setenv("DCP_SHARD_RESAMPLE", "lanczos")
    with pytest.raises(ValueError):
        config.parse_args(["--workload", "cdr"])


def test_resample_argument_is_validated():
    with pytest.raises(ValueError):
        shards.aug_preset("nested", True, 224, resample="lanczos")
    assert shards.aug_preset("plc", True, 224, resample="pil")[0].filter == 1
    assert shards.aug_preset("plc", True, 224)[0].filter == 0
