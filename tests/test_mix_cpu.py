"""Mixup / CutMix on the CPU: the plan sampler (data/mix.py), the fp64 oracles (tests/mix_ref.py:
preconditions and sensitivity to seeded mistakes), the CPU reference math of the new ops (ops/_ref.py)
against the oracles and against torch's soft-target cross-entropy, and main.py end to end.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ddp_classification_pytorch_amd.data.mix import MixSampler, cutmix_box, identity_plan, plan_to_device
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import mix_ref as M

H, W = 12, 20


def _same(p, q):
    return all(np.array_equal(a, b) for a, b in zip(p, q))


def _is_identity(p):
    return _same(p, identity_plan(len(p.partner)))


# ----------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_plan_is_a_function_of_seed_epoch_step_rank(mode):
    kw = dict(mixup_alpha=0.4, cutmix_alpha=1.0, mode=mode)
    a = MixSampler(seed=7, rank=1, **kw)
    b = MixSampler(seed=7, rank=1, **kw)
    a.set_epoch(3)
    assert _same(a.draw(9, H, W, step=5), b.draw(9, H, W, step=5, epoch=3))
    assert _same(a.draw(9, H, W, step=5), a.draw(9, H, W, step=5))  # no state advances between draws
    base = a.draw(9, H, W, step=5)
    assert not _same(base, a.draw(9, H, W, step=6))
    assert not _same(base, a.draw(9, H, W, step=5, epoch=4))
    assert not _same(base, MixSampler(seed=7, rank=2, **kw).draw(9, H, W, step=5, epoch=3))
    assert not _same(base, MixSampler(seed=8, rank=1, **kw).draw(9, H, W, step=5, epoch=3))


def test_prob_zero_is_the_identity_plan():
    s = MixSampler(0.4, 1.0, prob=0.0, seed=1)
    for step in range(5):
        p = s.draw(6, H, W, step)
        assert _is_identity(p)
        assert p.partner.dtype == np.int32 and p.blend.dtype == np.float32
        assert p.box.dtype == np.int32 and p.box.shape == (6, 4) and p.wlab.dtype == np.float32


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_cutmix_boxes_lie_in_the_image_and_weigh_the_clipped_area(mode):
    s = MixSampler(0.0, 1.0, mode=mode, seed=3)
    clipped = boxed = 0
    for step in range(40):
        p = s.draw(5, H, W, step)
        y0, x0, y1, x1 = (p.box[:, k].astype(np.int64) for k in range(4))
        assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all()
        assert (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
        area = (y1 - y0) * (x1 - x0)
        assert np.array_equal(p.wlab, (1.0 - area.astype(np.float64) / float(H * W)).astype(np.float32))
        assert (p.blend == 1).all()
        assert np.array_equal(p.partner, np.arange(5)[::-1])
        boxed += int((area > 0).sum())
        clipped += int(((y0 == 0) | (x0 == 0) | (y1 == H) | (x1 == W))[area > 0].sum())
    assert boxed > 100 and clipped > 10  # boxes were drawn, and the clipping was exercised


def test_cutmix_box_definition():
    # lam = 0.75: r = 0.5, a 6 x 10 box around the centre pixel; clipped at the image's corner
    assert cutmix_box(0.75, 0.5, 0.5, H, W) == (3, 5, 9, 15)
    assert cutmix_box(0.75, 0.0, 0.0, H, W) == (0, 0, 3, 5)
    assert cutmix_box(0.75, 0.999, 0.999, H, W) == (8, 14, 12, 20)
    assert cutmix_box(1.0, 0.3, 0.3, H, W)[0] == cutmix_box(1.0, 0.3, 0.3, H, W)[2]  # lam = 1: empty
    assert cutmix_box(0.0, 0.5, 0.5, H, W) == (0, 0, H, W)


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_mixup_blends_image_and_label_alike_without_a_box(mode):
    s = MixSampler(0.8, 0.0, mode=mode, seed=5)
    for step in range(10):
        p = s.draw(6, H, W, step)
        assert np.array_equal(p.blend, p.wlab) and (p.box == 0).all()
        assert ((p.blend >= 0) & (p.blend <= 1)).all()
        assert np.array_equal(p.partner, np.arange(6)[::-1])
        if mode == "batch":
            assert len(set(p.blend.tolist())) == 1


def test_elem_mode_varies_per_row_and_switches_per_row():
    s = MixSampler(0.8, 1.0, mode="elem", seed=5)
    p = s.draw(16, H, W, step=0)
    mixup_rows = (p.box == 0).all(1) & (p.blend != 1)
    cutmix_rows = ~(p.box == 0).all(1)
    assert mixup_rows.sum() >= 2 and cutmix_rows.sum() >= 2
    assert len(set(p.blend[mixup_rows].tolist())) > 1
    s2 = MixSampler(0.8, 1.0, mode="elem", prob=0.5, seed=5)
    q = s2.draw(16, H, W, step=0)
    unmixed = q.partner == np.arange(16)
    assert 0 < unmixed.sum() < 16
    assert (q.blend[unmixed] == 1).all() and (q.wlab[unmixed] == 1).all() and (q.box[unmixed] == 0).all()


def test_switch_prob_picks_cutmix_or_mixup():
    assert all((MixSampler(0.8, 1.0, switch_prob=0.0, seed=2).draw(4, H, W, s).box == 0).all() for s in range(8))
    assert all((MixSampler(0.8, 1.0, switch_prob=1.0, seed=2).draw(4, H, W, s).blend == 1).all() for s in range(8))
    kinds = {bool((MixSampler(0.8, 1.0, seed=2).draw(4, H, W, s).blend == 1).all()) for s in range(16)}
    assert kinds == {True, False}


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_partner_is_a_valid_index_and_the_middle_row_pairs_with_itself(n):
    p = MixSampler(0.8, 0.0, seed=0).draw(n, H, W, 0)
    assert ((p.partner >= 0) & (p.partner < n)).all()
    assert np.array_equal(p.partner[p.partner], np.arange(n))  # an involution
    if n % 2:
        assert p.partner[n // 2] == n // 2


def test_sampler_refuses_nonsense():
    with pytest.raises(ValueError):
        MixSampler(0.0, 0.0)
    with pytest.raises(ValueError):
        MixSampler(0.2, 0.0, mode="pairs")
    with pytest.raises(ValueError):
        MixSampler(0.2, 0.0, prob=1.5)


def test_plan_to_device_round_trips():
    p = MixSampler(0.8, 1.0, mode="elem", seed=9).draw(7, H, W, 2)
    d = plan_to_device(p, "cpu")
    assert d.partner.dtype == torch.int32 and d.blend.dtype == torch.float32 and d.box.shape == (7, 4)
    assert all(t.is_contiguous() for t in d)
    assert _same(p, [t.numpy() for t in d])


# ----------------------------------------------------------------------------- oracle: sensitivity
def _image_case(layout):
    gen = torch.Generator().manual_seed(11)
    N = 5
    src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=gen)
    partner = torch.arange(N - 1, -1, -1, dtype=torch.int32)
    blend = torch.tensor([1.0, 0.25, 1.0, 0.75, 1.0])
    box = torch.tensor([[3, 5, 8, 11], [0, 0, 0, 0], [1, 1, 2, 2], [0, 0, 0, 0], [5, 7, 12, 20]], dtype=torch.int32)
    return src, (partner, blend, box)


@pytest.mark.parametrize("layout", ["plain", "s2d2", "s2d4"])
def test_image_oracle_catches_seeded_mistakes(layout):
    src, plan = _image_case(layout)
    S = M.LAYOUTS[layout][0]
    # preconditions: partner images differ, blends are not 1/2, a box edge is odd (it splits a block)
    assert not torch.equal(src, src[plan[0].long()])
    assert all(float(b) != 0.5 for b in plan[1])
    assert any(int(v) % 2 for v in plan[2].reshape(-1))
    good = M.mix_images(src, False, 1 / 255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), plan, layout)
    assert good.shape == (5, H // S, W // S, S * S * M.LAYOUTS[layout][1])
    bugs = ["shift", "swap"] + (["block"] if S > 1 else [])
    for bug in bugs:
        bad = M.mix_images(src, False, 1 / 255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), plan, layout, bug=bug)
        n_diff = int((bad != good).sum())
        assert n_diff > 0, bug
        # far above one bf16 rounding of a normalised pixel (|v| <= 2.7): the GPU tests would see it
        assert (bad - good).abs().max().item() > 0.01, bug


def test_image_oracle_by_hand():
    """Two 2x2 one-channel images: row 0 blended 1/4 : 3/4 with a one-pixel box, row 1 untouched."""
    src = torch.tensor([[[[8.0], [16.0]], [[24.0], [32.0]]], [[[80.0], [160.0]], [[240.0], [248.0]]]])
    plan = (torch.tensor([1, 1]), torch.tensor([0.25, 1.0]), torch.tensor([[1, 0, 2, 1], [0, 0, 0, 0]]))
    out = M.mix_images(src, False, 0.5, (1.0,), (2.0,), plan, "plain")
    na = (src.double() * 0.5 - 1.0) / 2.0
    want0 = 0.25 * na[0] + 0.75 * na[1]
    want0[1, 0] = na[1, 1, 0]
    assert torch.equal(out[0, ..., :1], want0) and torch.equal(out[1, ..., :1], na[1])
    assert (out[..., 1:] == 0).all() and out.shape == (2, 2, 2, 8)
    s2d = M.mix_images(src, False, 0.5, (1.0,), (2.0,), plan, "s2d2")
    assert s2d.shape == (2, 1, 1, 16)
    assert torch.equal(s2d[0, 0, 0, [0, 4, 8, 12]], want0.reshape(-1))


def _loss_case(C=7):
    gen = torch.Generator().manual_seed(13)
    B = 6
    x = torch.randn(B, C + 2, generator=gen)
    labels = torch.tensor([0, 3, 6, 2, 5, 1])
    partner = torch.arange(B - 1, -1, -1, dtype=torch.int32)
    wlab = torch.tensor([0.3, 0.9, 1.0, 0.0, 0.5, 0.7])
    return x, labels, partner, wlab, C


def test_loss_oracle_catches_the_weight_on_the_wrong_label():
    x, labels, partner, wlab, C = _loss_case()
    assert not torch.equal(labels, labels[partner.long()])  # precondition: the pair differs
    good = M.xent_mix_rows(x, labels, partner, wlab, C)["loss"]
    bad = M.xent_mix_rows(x, labels, partner, wlab, C, bug="wlab")["loss"]
    rows = wlab != 0.5
    assert ((good - bad).abs()[rows] > 1e-3).all()
    gg = M.xent_mix_grad(x, labels, partner, wlab, C, 1.0)
    gb = M.xent_mix_grad(x, labels, partner, wlab, C, 1.0, bug="wlab")
    assert ((gg - gb).abs().amax(1)[rows] > 1e-2).all()


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_loss_oracle_against_torch_soft_targets_fp64(smoothing):
    """The oracle against an independent formulation: torch's cross_entropy on explicit soft targets."""
    x, labels, partner, wlab, C = _loss_case()
    t = M.xent_mix_targets(labels, partner, wlab, C, smoothing)
    assert torch.allclose(t.sum(1), torch.ones(6, dtype=torch.float64), atol=1e-15)
    leaf = x[:, :C].double().requires_grad_(True)
    rows = F.cross_entropy(leaf, t, reduction="none")
    r = M.xent_mix_rows(x, labels, partner, wlab, C, smoothing)
    assert (rows.detach() - r["loss"]).abs().max().item() < 1e-13
    rows.sum().mul(0.37).backward()
    assert (leaf.grad - M.xent_mix_grad(x, labels, partner, wlab, C, 0.37, smoothing)).abs().max().item() < 1e-14
    assert torch.equal(r["rank"], (x[:, :C].double() > x[:, :C].double().gather(1, labels[:, None])).sum(1))


def test_loss_oracle_zeroes_rows_with_an_invalid_label():
    x, labels, partner, wlab, C = _loss_case()
    labels = labels.clone()
    labels[0], labels[4] = -1, C  # rows 0 and 4 by their own label, rows 5 and 1 by their partner's
    r = M.xent_mix_rows(x, labels, partner, wlab, C)
    assert r["valid"].tolist() == [False, False, True, True, False, False]
    assert (r["loss"][~r["valid"]] == 0).all() and (r["loss"][r["valid"]] > 0).all()
    g = M.xent_mix_grad(x, labels, partner, wlab, C, 1.0)
    assert (g[~r["valid"]] == 0).all()


# ----------------------------------------------------------------------------- ops/_ref.py against the oracle
@pytest.mark.parametrize("layout", ["plain", "s2d2", "s2d4"])
@pytest.mark.parametrize("nchw", [False, True])
def test_ref_input_math_matches_the_oracle(layout, nchw):
    src, plan = _image_case(layout)
    if nchw:
        src = src.permute(0, 3, 1, 2).contiguous()
    S, cq = M.LAYOUTS[layout]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    got = Fn.to_device_nhwc(src, mean, std, cpad=8, nchw=nchw, in_scale=1 / 255.0, s2d=S if S > 1 else False, mix=plan)
    want = M.mix_images(src, nchw, 1 / 255.0, mean, std, plan, layout)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert (got.double() - want).abs().max().item() < 1e-5  # fp32 math on |v| <= 2.7
    # the identity plan is the unmixed op, bit for bit
    ident = plan_to_device(identity_plan(5), "cpu")
    same = Fn.to_device_nhwc(src, mean, std, cpad=8, nchw=nchw, in_scale=1 / 255.0, s2d=S if S > 1 else False, mix=ident)
    plain = Fn.to_device_nhwc(src, mean, std, cpad=8, nchw=nchw, in_scale=1 / 255.0, s2d=S if S > 1 else False)
    assert torch.equal(same, plain)


def test_generic_channel_padding_refuses_a_plan():
    src, plan = _image_case("plain")
    with pytest.raises(ValueError, match="mix plan"):
        Fn.to_device_nhwc(src, None, None, cpad=3, nchw=False, mix=plan)
    with pytest.raises(ValueError, match="mix plan"):
        Fn.to_device_nhwc(src, None, None, cpad=16, nchw=False, mix=plan)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_ref_loss_math_matches_the_oracle_and_torch(smoothing):
    """fp32 reference math: within 1e-6 max(1, max|x|) of the fp64 oracle and of torch's fp32
    soft-target cross-entropy (a few fp32 roundings of magnitudes up to max|x| ~ 3)."""
    x, labels, partner, wlab, C = _loss_case()
    labels = labels.clone()
    labels[4] = C  # one invalid own label (row 4), one invalid partner label (row 1)
    sm = float(torch.tensor(smoothing, dtype=torch.float32))
    r = M.xent_mix_rows(x, labels, partner, wlab, C, sm)
    tol = 1e-6 * r["absmax"].clamp_min(1.0)
    for padded in (False, True):
        leaf = x.clone().requires_grad_(True)
        logits = leaf if padded else leaf[:, :C]
        loss, rank = Fn.cross_entropy(logits, labels, C, smoothing=smoothing, reduction="sum", return_rank=True,
                                      mix=(partner, wlab))
        rows, rank2 = Fn.K(leaf).xent_mix_fwd(logits.detach(), labels, partner, wlab, C, smoothing)
        assert ((rows.double() - r["loss"]).abs() <= tol).all()
        assert (rows[~r["valid"]] == 0).all()
        assert abs(loss.item() - r["loss"].sum().item()) <= tol.sum().item()
        assert torch.equal(rank.long()[r["own_valid"]], r["rank"][r["own_valid"]]) and torch.equal(rank, rank2)
        (loss * 0.37).backward()
        want = M.xent_mix_grad(x, labels, partner, wlab, C, float(torch.tensor(0.37)), sm)
        assert leaf.grad.shape == x.shape
        assert (leaf.grad[:, :C].double() - want).abs().max().item() <= 1e-6
        assert (leaf.grad[:, C:] == 0).all() and (leaf.grad[~r["valid"]] == 0).all()
    # torch, fp32, on the valid rows
    v = r["valid"]
    t = M.xent_mix_targets(labels, partner, wlab, C, sm)[v].float()
    leaf = x[v][:, :C].clone().requires_grad_(True)
    trows = F.cross_entropy(leaf, t, reduction="none")
    rows, _ = Fn.K(x).xent_mix_fwd(x[:, :C], labels, partner, wlab, C, smoothing)
    assert ((rows[v] - trows.detach()).abs().double() <= tol[v]).all()
    trows.sum().mul(0.37).backward()
    d = Fn.K(x).xent_mix_bwd(x[:, :C], labels, partner, wlab, C, torch.tensor([0.37]), 1.0, smoothing, False)
    assert (d[v] - leaf.grad).abs().max().item() <= 1e-6


def test_without_mix_the_one_label_function_runs(monkeypatch):
    from ddp_classification_pytorch_amd.ops import _ref

    def boom(*a, **k):
        raise AssertionError("the two-label op ran without a plan")

    monkeypatch.setattr(_ref, "xent_mix_fwd", boom)
    monkeypatch.setattr(_ref, "to_nhwc_mix", boom)
    monkeypatch.setattr(_ref, "to_nhwc_s2d_mix", boom)
    x, labels, *_ = _loss_case()
    Fn.cross_entropy(x, labels, 7)
    Fn.to_device_nhwc(_image_case("plain")[0], None, None, nchw=False)


# ----------------------------------------------------------------------------- end to end
SMALL = ["--device", "cpu", "--image-size", "64", "--batchsize", "4", "--synthetic-train-size", "16",
         "--synthetic-val-size", "8", "--workers", "0", "--log-interval", "1", "--max-steps-per-epoch", "4"]


def test_main_baseline_trains_with_mixup_and_cutmix_on_the_cpu(tmp_path):
    import main as entry

    entry.main(["--workload", "baseline", "--data", "synthetic", "--model", "resnet18", "--num-classes", "10",
                "--epochs", "1", "--mixup-alpha", "0.2", "--cutmix-alpha", "1.0", "--out-dir", str(tmp_path)] + SMALL)
    with open(tmp_path / "metrics.jsonl") as f:
        recs = [json.loads(line) for line in f]
    it = [r for r in recs if r["kind"] == "train_iter"]
    assert len(it) == 4
    assert all(np.isfinite(r["loss"]) and r["loss"] > 0 for r in it)
    assert all(np.isfinite(r["loss"]) for r in recs if r["kind"] in ("train_epoch", "val"))


@pytest.mark.parametrize("workload", ["arcface", "cdr", "nested", "plc"])
def test_one_label_workloads_refuse_the_mix_flags(tmp_path, workload):
    import main as entry

    with pytest.raises(ValueError, match="baseline only"):
        entry.main(["--workload", workload, "--data", "synthetic", "--model", "resnet18", "--num-classes", "10",
                    "--epochs", "1", "--mixup-alpha", "0.2", "--out-dir", str(tmp_path)] + SMALL)


def test_loaders_yield_the_plan_with_fixed_shapes():
    """SyntheticLoader with a sampler: (x, labels, partner, wlab), the identity plan on unmixed steps."""
    from ddp_classification_pytorch_amd.data import SyntheticLoader

    s = MixSampler(0.8, 1.0, prob=0.5, seed=4)
    ld = SyntheticLoader(6, 8, size=16, num_classes=10, device="cpu", mix=s, s2d=True)
    plain = SyntheticLoader(6, 8, size=16, num_classes=10, device="cpu", s2d=True)
    kinds = set()
    for step, (b, pb) in enumerate(zip(ld, plain)):
        assert len(b) == 4 and len(pb) == 2
        x, labels, partner, wlab = b
        assert x.shape == pb[0].shape == (6, 8, 8, 16) and partner.shape == wlab.shape == (6,)
        want = s.draw(6, 16, 16, step)
        assert np.array_equal(partner.numpy(), want.partner) and np.array_equal(wlab.numpy(), want.wlab)
        ident = _is_identity(want)
        kinds.add(ident)
        assert torch.equal(x, pb[0]) == ident
    assert kinds == {True, False}
