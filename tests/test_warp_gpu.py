"""GPU half of the shard loader's affine route: warp_crop_kernel (csrc/augment.hip) against the
fp64 oracle (tests/warp_oracle.py) with the criteria of the CPU test of the reference math, the
exact lattice cases, the host-side box check, and a ShardLoader epoch on cuda against cpu for the
CDR, CIFAR and PLC presets."""
import numpy as np
import pytest
import torch

from ddp_classification_pytorch_amd.data import ShardSampler
from ddp_classification_pytorch_amd.data.shards import ShardLoader, aug_preset, write_shard
from ddp_classification_pytorch_amd.ops import functional as Fn

from . import warp_oracle as wo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Ho,Wo", [(37, 53), (32, 32), (224, 224)])
def test_warp_kernel_matches_oracle(Ho, Wo):
    """Within one level everywhere outside the 2^-10 px band around the canvas edges, exactly 0 in
    all channels where the oracle is outside by more than the band, and fill-or-sample inside it."""
    recs, boxes, geos = wo.random_batch(Ho, Wo)
    src, meta, xf = wo._pack(recs, boxes, geos)
    out = Fn.warp_crop(src.cuda(), meta, xf, Ho, Wo)
    assert out.is_cuda and out.shape == (9, Ho, Wo, 3) and out.dtype == torch.uint8
    wo.check_against_oracle(out, recs, boxes, geos)


def test_warp_kernel_exact_on_the_lattice():
    """CIFAR's chain (theta 0, scale 1, integer offsets, both flips) and quarter turns at scale 1:
    every source position is an integer or a half-integer, so fp32 has nothing to round."""
    recs, boxes, geos = wo.lattice_batch()
    src, meta, xf = wo._pack(recs, boxes, geos)
    ref, ins, _ = wo.expected(recs, boxes, geos)
    out = Fn.warp_crop(src.cuda(), meta, xf, 32, 32).cpu()
    assert torch.equal(out, torch.from_numpy(ref))
    assert not ins.all() and out[torch.from_numpy(~ins)].max().item() == 0


def test_warp_kernel_nan_and_huge_matrices_are_fill():
    """NaN compares false and a huge coordinate is outside: both give the fill, and neither reads."""
    recs, boxes, geos = wo.lattice_batch()
    src, meta, xf = wo._pack(recs[:3], boxes[:3], geos[:3])
    xf[0, 2] = float("nan")
    xf[1, :6] = float("inf")
    xf[2, :6] = 3e38
    assert Fn.warp_crop(src.cuda(), meta, xf, 32, 32).max().item() == 0


def test_warp_rejects_out_of_bounds_box():
    recs, boxes, geos = wo.random_batch(16, 16, B=2)
    src, meta, xf = wo._pack(recs, boxes, geos)
    bad = meta.clone()
    bad[1, 5] = bad[1, 1] + 1  # box taller than the record
    with pytest.raises(RuntimeError, match="outside its record"):
        Fn.warp_crop(src.cuda(), bad, xf, 16, 16)
    bad = meta.clone()
    bad[1, 0] = src.numel() - 5  # record past the gathered buffer
    with pytest.raises(RuntimeError, match="outside the gathered buffer"):
        Fn.warp_crop(src.cuda(), bad, xf, 16, 16)
    with pytest.raises(RuntimeError, match="xf"):
        Fn.warp_crop(src.cuda(), meta, xf[:1], 16, 16)


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    rng = np.random.default_rng(1)
    imgs = [(rng.integers(0, 256, (int(rng.integers(40, 80)), int(rng.integers(40, 80)), 3), dtype=np.uint8), i % 7)
            for i in range(45)]
    p = str(tmp_path_factory.mktemp("warp_gpu") / "g.dcps")
    write_shard(p, imgs)
    return p


@pytest.mark.parametrize("name", ["cdr", "cifar", "plc"])
def test_shard_loader_gpu_matches_cpu_new_presets(shard, name):
    aug, size = aug_preset(name, train=True, size=32)
    assert size == 32 and aug.affine
    outs = {}
    for dev in ("cpu", "cuda"):
        sampler = ShardSampler(list(range(45)), num_replicas=1, rank=0, shuffle=True, seed=2)
        ld = ShardLoader(shard, batch_size=16, sampler=sampler, aug=aug, out_size=32, device=dev, threads=4,
                         prefetch=2, s2d=True, return_index=True)
        ld.set_epoch(1)
        outs[dev] = [(x.float().cpu(), y.cpu(), i.cpu()) for x, y, i in ld]
        ld.close()
    assert len(outs["cpu"]) == len(outs["cuda"]) == 3
    over = total = 0
    for (xc, yc, ic), (xg, yg, ig) in zip(outs["cpu"], outs["cuda"]):
        assert torch.equal(yc, yg) and torch.equal(ic, ig)
        assert xg.shape == xc.shape
        # one uint8 level of resample rounding + bf16 normalisation; a pixel in the band around a
        # canvas edge may be fill on one device and a sample on the other
        over += int(((xg - xc).abs() >= 0.06).sum())
        total += xc.numel()
    print(f"{name}: {over} of {total} elements differ by 0.06 or more")
    assert over <= 1e-4 * total
