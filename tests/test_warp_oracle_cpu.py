"""The fp64 warp oracle (tests/warp_oracle.py) against PIL, so that everything pinned to the
oracle -- ops/_ref.py:warp_crop, warp_crop_kernel, the host matrix -- is pinned to the reference
pipelines' geometry: CIFAR's pad-crop-flip exactly, quarter turns exactly, and arbitrary angles
in nearest mode up to PIL's rounding ties."""
from dataclasses import replace

import numpy as np
import pytest
from PIL import Image

from ddp_classification_pytorch_amd.data import transforms as T
from ddp_classification_pytorch_amd.data.shards import aug_preset

from .warp_oracle import Geo, center_offset, warp

# the numbers of the chains come from the shard presets, so that what is pinned to PIL here is
# what the native loader is told to do: CIFAR's padding and output, CDR's canvas, output and angles
CIFAR, CIFAR_OUT = aug_preset("cifar", train=True)
CDR, CDR_OUT = aug_preset("cdr", train=True, size=112)
ANGLES = [15.0, -15.0, 7.3, -3.1, 0.5, 11.0, -14.2]


class _Draws:
    """Stands in for the ``random`` module inside data/transforms.py: fixed crop offsets and flip."""

    def __init__(self, ints, flip):
        self.ints, self.flip = list(ints), flip

    def randint(self, lo, hi):
        v = self.ints.pop(0)
        assert lo <= v <= hi
        return v

    def random(self):
        return 0.0 if self.flip else 0.99

    def uniform(self, lo, hi):
        raise AssertionError("the CIFAR chain draws no float range")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("i,j", [(0, 0), (8, 8), (3, 5), (4, 4), (7, 0)])
def test_oracle_equals_cifar_pad_crop_flip(monkeypatch, i, j, flip):
    img = np.random.default_rng(i * 9 + j).integers(0, 256, (32, 32, 3), dtype=np.uint8)
    monkeypatch.setattr(T, "random", _Draws([i, j], flip))
    ref = T.build_transform("cifar", train=True)(Image.fromarray(img))
    assert (CIFAR.pad, CIFAR_OUT) == (4, 32) and ref.shape == (CIFAR_OUT, CIFAR_OUT, 3)
    got = warp(img, Geo(32, 32, 32, 32, CIFAR_OUT, CIFAR_OUT, dx=j - CIFAR.pad, dy=i - CIFAR.pad, theta=0.0,
                        flip=flip))
    assert np.array_equal(got, ref)
    if (i, j) == (0, 0) and not flip:
        assert not ref[:4].any() and not ref[:, :4].any() and np.array_equal(ref[4:, 4:], img[:28, :28])


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("theta", [90.0, -90.0, 180.0])
@pytest.mark.parametrize("H,W", [(24, 24), (31, 31), (20, 26)])
def test_oracle_equals_pil_quarter_turns(H, W, theta, nearest):
    """Image.rotate keeps the canvas, so on a non-square image a quarter turn leaves a zero border;
    (20, 26) has H + W even, which keeps every source position on a pixel centre."""
    img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).rotate(theta, resample=Image.NEAREST))
    got = warp(img, Geo(H, W, H, W, H, W, 0.0, 0.0, theta), nearest=nearest)
    assert np.array_equal(got, ref)


def _pil_chain(img, theta, flip, out):
    pil = Image.fromarray(img).rotate(theta, resample=Image.NEAREST)
    if flip:
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(T.CenterCrop(out)(pil))


def _mismatch(a, b):
    return float((a != b).any(-1).mean())


@pytest.fixture(scope="module")
def canvas():
    """CDR's 256 canvas / 224 output at half size: the preset keeps the 8:7 ratio."""
    assert (CDR.canvas_h, CDR.canvas_w, CDR_OUT) == (128, 128, 112) and max(map(abs, ANGLES)) <= CDR.rot_deg
    return np.random.default_rng(11).integers(0, 256, (CDR.canvas_h, CDR.canvas_w, 3), dtype=np.uint8)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("theta", ANGLES)
def test_oracle_nearest_matches_pil_rotate_flip_crop(canvas, theta, flip):
    """CDR's rotation -> flip -> CenterCrop on a canvas, at scale 1: the oracle in nearest mode
    reads the pixel PIL reads except where PIL's incremental fixed-order float sum lands on the
    other side of a pixel boundary (measured at most 0.22 % of the pixels); 1 % is the bound."""
    S, out = canvas.shape[0], CDR_OUT
    d = float(center_offset(S, out))
    got = warp(canvas, Geo(S, S, S, S, out, out, d, d, theta, flip), nearest=True)
    m = _mismatch(got, _pil_chain(canvas, theta, flip, out))
    print(f"theta {theta} flip {flip}: mismatch {m:.5f}")
    assert m <= 0.01


def test_geometry_errors_do_not_hide_in_the_bound(canvas):
    """What the 1 % bound rejects.  On a random image two different source pixels differ with
    probability 1 - 2^-24, so the mismatch rate is the fraction of pixels whose lookup moved:
    a rotation of the wrong sign moves every pixel further than 0.5 px from the centre's
    neighbourhood (all but a few of 112^2); a half-pixel centre error in both axes moves
    floor() in either axis for 3/4 of the pixels."""
    S, out, theta = canvas.shape[0], CDR_OUT, 15.0
    d = float(center_offset(S, out))
    good = Geo(S, S, S, S, out, out, d, d, theta, False)
    ref = _pil_chain(canvas, theta, False, out)
    assert _mismatch(warp(canvas, good, nearest=True), ref) <= 0.01
    assert _mismatch(warp(canvas, replace(good, theta=-theta), nearest=True), ref) > 0.95
    assert _mismatch(warp(canvas, replace(good, dx=d + 0.5, dy=d + 0.5), nearest=True), ref) > 0.6
    assert _mismatch(warp(canvas, replace(good, flip=True), nearest=True), ref) > 0.95
