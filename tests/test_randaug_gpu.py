"""``Fn.rand_augment`` on the device against Pillow itself (``data.randaug.apply_pil``): every comparison is
``torch.equal``.  One-op plans per op, level and sign at three sizes on random and degenerate images, all
196 ordered pairs, sampled chains of three, the limits, and the shard loader's wiring."""
import itertools

import numpy as np
import pytest
import torch

from ddp_classification_pytorch_amd.data import randaug as ra
from ddp_classification_pytorch_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(224, 224), (32, 32), (37, 53)]
_POOL = {}


def pool(H, W):
    """8 host images of H x W, made once: 4 of random bytes, then a constant image, one with a constant
    channel, one of two grey levels, one whose extreme values sit in one corner pixel only."""
    if (H, W) not in _POOL:
        g = torch.Generator().manual_seed(H * 1000 + W)
        a = torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, generator=g)
        a[4] = 77
        a[5, :, :, 1] = 200
        a[6] = torch.where(a[6, :, :, :1] > 127, 190, 60).to(torch.uint8)
        a[7] = torch.randint(40, 200, (H, W, 3), dtype=torch.uint8, generator=g)
        a[7, 0, 0] = torch.tensor([0, 255, 0], dtype=torch.uint8)
        a[7, H - 1, W - 1] = torch.tensor([255, 0, 255], dtype=torch.uint8)
        _POOL[(H, W)] = a
    return _POOL[(H, W)]


def check(imgs, plan):
    got = Fn.rand_augment(imgs.to(DEV), plan).cpu()
    want = ra.apply_pil_batch(imgs, plan)
    bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
    assert torch.equal(got, want), f"images {bad} differ from Pillow; their ops: {[plan.op[n].tolist() for n in bad]}"


@pytest.mark.parametrize("level", [0, 9, 30])
@pytest.mark.parametrize("op", range(ra.NUM_OPS), ids=ra.OP_NAMES)
def test_one_op_equals_pillow(op, level):
    for (H, W), neg in itertools.product(SIZES, (False, True) if op in ra.SIGNED else (False,)):
        imgs = pool(H, W)
        plan = ra.make_plan(np.full((4, 1), op), level, neg, H, W)
        check(imgs[:4], plan)
        check(imgs[4:], plan)


def test_all_ordered_pairs_equal_pillow():
    pairs = np.array(list(itertools.product(range(ra.NUM_OPS), repeat=2)))
    imgs = pool(64, 64)[torch.arange(196) % 8]
    check(imgs, ra.make_plan(pairs, 9, np.arange(392).reshape(196, 2) % 3 == 0, 64, 64))


def test_sampled_chains_of_three_equal_pillow():
    out_of_place = lambda o: o in ra.GEOMETRIC or o == ra.SHARPNESS
    plan = ra.RandAugSampler(3, 9, seed=5).plan(16, 224, 224, step=0)
    rows = [r.tolist() for r in plan.op]
    # the draw of this seed holds the two restaging cases of a full LDS
    assert any(out_of_place(a) and out_of_place(b) for r in rows for a, b in zip(r, r[1:]))
    assert any(out_of_place(a) and b in (ra.CONTRAST, ra.AUTOCONTRAST, ra.EQUALIZE) for r in rows for a, b in zip(r, r[1:]))
    check(pool(224, 224)[torch.arange(16) % 8], plan)


def test_identity_plan_returns_the_input():
    imgs = pool(37, 53)
    for k in (1, 4):
        assert torch.equal(Fn.rand_augment(imgs.to(DEV), ra.identity_plan(8, k)).cpu(), imgs)


def test_limits_raise():
    small = pool(32, 32).to(DEV)
    with pytest.raises(ValueError, match="rand_augment covers"):
        Fn.rand_augment(torch.zeros(2, 256, 256, 3, dtype=torch.uint8, device=DEV), ra.identity_plan(2))
    with pytest.raises(ValueError, match="rand_augment covers"):
        Fn.rand_augment(small, ra.RandAugPlan(np.zeros((8, 5), np.int32), np.zeros((8, 5), np.float32),
                                              np.zeros((8, 5), np.int32), np.zeros((8, 5, 6), np.int32)))
    plan = ra.identity_plan(8)
    plan.op[3, 0] = 14
    with pytest.raises(ValueError, match="rand_augment covers"):
        Fn.rand_augment(small, plan)
    with pytest.raises(ValueError, match="rand_augment covers"):
        Fn.rand_augment(small.float(), ra.identity_plan(8))


@pytest.mark.parametrize("with_sampler", [True, False])
def test_shard_loader_applies_the_plan_of_each_step(tmp_path, with_sampler):
    from ddp_classification_pytorch_amd.data import ShardSampler
    from ddp_classification_pytorch_amd.data.shards import ShardLoader, aug_preset, write_shard

    rng = np.random.default_rng(1)
    recs = [(rng.integers(0, 256, (int(rng.integers(40, 80)), int(rng.integers(40, 80)), 3), dtype=np.uint8), i % 7)
            for i in range(40)]
    path = str(tmp_path / "r.dcps")
    write_shard(path, recs)
    aug, _ = aug_preset("nested", train=True, size=32)
    rand = ra.RandAugSampler(2, 9, seed=3) if with_sampler else None

    def loader(randaug):
        return ShardLoader(path, batch_size=16, sampler=ShardSampler(list(range(40)), num_replicas=1, rank=0,
                                                                     shuffle=True, seed=2),
                           aug=aug, out_size=32, device=DEV, threads=4, prefetch=2, s2d=True, randaug=randaug)

    ld = loader(rand)
    tapped = []
    ld.tap = lambda u8, meta, extra: tapped.append(u8.cpu())
    ld.set_epoch(1)
    batches = [b[0].cpu() for b in ld]
    ld.close()
    assert len(batches) == len(tapped) == 3
    for step, (x, u8) in enumerate(zip(batches, tapped)):
        u8 = u8.to(DEV)
        if with_sampler:
            u8 = Fn.rand_augment(u8, rand.plan(u8.shape[0], 32, 32, step, epoch=1))
        want = Fn.to_device_nhwc(u8, ld.mean, ld.std, cpad=8, nchw=False, in_scale=1.0 / 255.0, s2d=ld.s2d)
        assert torch.equal(x, want.cpu())
    if with_sampler:  # and the augmentation is not a no-op on this shard
        plain = loader(None)
        plain.set_epoch(1)
        assert not torch.equal(next(iter(plain))[0].cpu(), batches[0])
        plain.close()
