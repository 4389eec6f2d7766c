"""RandAugment on the host: the sampler's draws, the parameter table of data/randaug.py, the CPU path of
``Fn.rand_augment`` (Pillow itself) and the ``--randaugment`` flag's refusals."""
import numpy as np
import pytest
import torch

from ddp_classification_pytorch_amd.data import randaug as ra
from ddp_classification_pytorch_amd.ops import functional as Fn


def test_plan_is_a_pure_function_of_seed_epoch_step_rank():
    base = dict(step=3, epoch=2, rank=1)
    draw = lambda seed=7, **kw: ra.RandAugSampler(2, 9, seed=seed).plan(64, 32, 48, **{**base, **kw})
    same = lambda p, q: all(np.array_equal(a, b) for a, b in zip(p, q))
    ref = draw()
    assert same(ref, draw())
    assert ref.op.shape == (64, 2) and ref.coef.shape == (64, 2, 6) and set(ref.op.flatten()) == set(range(14))
    for other in (draw(seed=8), draw(step=4), draw(epoch=3), draw(rank=0)):
        assert not same(ref, other)


F32 = lambda v: float(np.float32(v))
TABLE = {  # level -> the expected (positive) parameters at H x W = 40 x 100; factor = (plus, minus)
    0: dict(shear=0.0, tx=0, ty=0, deg=0.0, factor=(1.0, 1.0), bits=8, thr=255),
    9: dict(shear=F32(0.09), tx=13, ty=5, deg=F32(9.0), factor=(F32(1.27), F32(0.73)), bits=7, thr=179),
    30: dict(shear=F32(0.3), tx=45, ty=18, deg=F32(30.0), factor=(F32(1.9), F32(0.1)), bits=4, thr=0),
}


@pytest.mark.parametrize("level", [0, 9, 30])
def test_parameter_table(level):
    t, H, W = TABLE[level], 40, 100
    for neg in (False, True):
        s = -1 if neg else 1
        for op in (ra.SHEAR_X, ra.SHEAR_Y):
            assert ra.op_params(op, level, neg, H, W)[0] == s * t["shear"]
        assert ra.op_params(ra.TRANSLATE_X, level, neg, H, W)[1] == s * t["tx"]
        assert ra.op_params(ra.TRANSLATE_Y, level, neg, H, W)[1] == s * t["ty"]
        assert ra.op_params(ra.ROTATE, level, neg, H, W)[0] == s * t["deg"]
        for op in (ra.BRIGHTNESS, ra.COLOR, ra.CONTRAST, ra.SHARPNESS):
            assert ra.op_params(op, level, neg, H, W)[0] == t["factor"][neg]
        assert ra.op_params(ra.POSTERIZE, level, neg, H, W)[1] == t["bits"]
        assert ra.op_params(ra.SOLARIZE, level, neg, H, W)[1] == t["thr"]
        for op in (ra.IDENTITY, ra.AUTOCONTRAST, ra.EQUALIZE):
            assert ra.op_params(op, level, neg, H, W) == (0.0, 0, (0,) * 6)
    # the 16.16 integers of a translation and of the identity shear, by hand
    assert ra.op_params(ra.TRANSLATE_X, 30, True, H, W)[2] == (65536, 0, -45 * 65536 + 32768, 0, 65536, 32768)
    assert ra.op_params(ra.SHEAR_Y, 0, False, H, W)[2] == (65536, 0, 32768, 0, 65536, 32768)


def test_cpu_path_is_apply_pil():
    from PIL import Image

    imgs = torch.randint(0, 256, (6, 21, 34, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    plan = ra.RandAugSampler(3, 12, seed=1).plan(6, 21, 34, step=0)
    got = Fn.rand_augment(imgs, plan)
    for n in range(6):
        want = np.asarray(ra.apply_pil(Image.fromarray(imgs[n].numpy()), plan.row(n)))
        assert torch.equal(got[n], torch.from_numpy(want.copy()))
    assert not torch.equal(got, imgs)
    assert torch.equal(Fn.rand_augment(imgs, ra.identity_plan(6, 2)), imgs)
    with pytest.raises(ValueError, match="rand_augment covers"):
        Fn.rand_augment(imgs.float(), plan)


SMALL = ["--device", "cpu", "--image-size", "64", "--batchsize", "4", "--synthetic-train-size", "16",
         "--synthetic-val-size", "8", "--workers", "0", "--model", "resnet18", "--num-classes", "10", "--epochs", "1"]


@pytest.mark.parametrize("extra, match", [
    (["--workload", "arcface", "--data", "shards", "--randaugment", "2,9"], "baseline only"),
    (["--workload", "cdr", "--data", "shards", "--randaugment", "2,9"], "baseline only"),
    (["--workload", "baseline", "--data", "synthetic", "--randaugment", "2,9"], "--data shards"),
    (["--workload", "baseline", "--data", "folder", "--randaugment", "2,9"], "--data shards"),
    (["--workload", "baseline", "--data", "shards", "--randaugment", "2"], "two integers"),
    (["--workload", "baseline", "--data", "shards", "--randaugment", "2,x"], "two integers"),
    (["--workload", "baseline", "--data", "shards", "--randaugment", "5,9"], "num_ops"),
    (["--workload", "baseline", "--data", "shards", "--randaugment", "2,31"], "magnitude"),
])
def test_flag_is_refused_at_start_up(tmp_path, extra, match):
    import main as entry

    with pytest.raises(ValueError, match=match):
        entry.main(extra + ["--out-dir", str(tmp_path)] + SMALL)
