"""Per-segment gradient checks of the ResNet family against fp64 ("teacher forcing").

One training step of the project model runs with cloning hooks at every block boundary; the fp64
mirror of ONE segment (stem, a residual block, head; tests/model_mirror.py) is then run on the
tensors captured from that step, and every parameter gradient of the segment and the gradient at
its input are compared.  Unlike a whole-model gradient, whose distance from fp64 in bf16 is of
order 1 for ANY implementation (test_yardstick_usable measures it), a segment's error stays at a
few per cent in bf16 and at fp32 rounding on the CPU path, so the bounds here can fail: they pin
the autograd wiring of ops/functional.py and models/resnet.py -- GradJoin claim / deposit,
StridedGrad compact deposits, BNSource and the dgrad-epilogue BN backward, the BN prologues of
conv2 / conv3, shortcut-BN fusion, the one-op stem."""
import copy

import pytest
import torch

from ddp_classification_pytorch_amd.models import build_model, input_layout
from ddp_classification_pytorch_amd.models import resnet as R
from ddp_classification_pytorch_amd.ops import functional as Fn
from tests import model_mirror as M

FP32_BOUND = 1e-4  # the fp32-path-versus-fp64 bound of test_model_parity.py
KINK_TOL = 1e-5    # ~100 fp32 roundings of a normalised pre-activation (M.teacher_forced_errors)


def _flat(errs):
    return [(seg, q, e, y) for seg, qs in errs.items() for q, (e, y) in qs.items()]


def _cpu_errors(name, hw, frozen=False, batch=4, classes=10):
    torch.manual_seed(0)
    model = build_model(name, num_classes=classes)
    if frozen:
        M.frozen_copy(model)
    model64 = copy.deepcopy(model).double()
    imgs = torch.randn(batch, 3, *hw)
    labels = torch.randint(0, classes, (batch,))

    def step(m):
        Fn.cross_entropy(m(Fn.to_device_nhwc(imgs, cpad=8, nchw=True)), labels).backward()

    return M.teacher_forced_errors(model, model64, step, training=not frozen, labels=labels, kink_tol=KINK_TOL)


def _expected_quantities(name, errs, frozen):
    """Every segment is there with the quantities the check is about."""
    model = build_model(name, num_classes=10)
    blocks = M.named_blocks(model)
    assert set(errs) == {"stem", "head"} | {n for n, _ in blocks}
    keep = (lambda n: "bn" not in n and "downsample.1" not in n) if frozen else (lambda n: True)
    for n, blk in blocks:
        assert set(errs[n]) == {p for p, _ in blk.named_parameters() if keep(p)} | {"dx"}, n
    assert set(errs["stem"]) == {"conv1.weight"} | (set() if frozen else {"bn1.weight", "bn1.bias"})
    assert set(errs["head"]) == {"fc.weight", "fc.bias", "dy_last"}


# ----------------------------------------------------------------------------- a. harness exactness (CPU, fp32 path)
@pytest.mark.parametrize("name,hw", [("resnet50", (64, 64)), ("resnet18", (64, 64)), ("resnext50_32x4d", (64, 64)),
                                     ("cifar_resnet18", (32, 32))])
def test_cpu_segments_match_fp64(name, hw):
    """The fp32 reference-math path through the same functional.py wiring: every quantity of every
    segment within 1e-4 of fp64 (measured <= 2e-6).

    ResNeXt-50 layer1.1 (bn1.bias 1.4e-3, conv1.weight 1.0e-3, dx 7e-4 without the kink analysis)
    is neither a near-zero norm nor the grouped path: the fp64 mirror puts ONE of that block's
    131,072 bn1 outputs at -1.4e-7, the fp32 path (and stock fp32 PyTorch alike) at +1.2e-7, so
    that element's ReLU mask differs, and one mask element is worth ~1e-3 of these gradients.
    ``kink_tol`` removes exactly that direction (M.teacher_forced_errors); the block is then at
    1e-6 like every other."""
    errs = _cpu_errors(name, hw)
    _expected_quantities(name, errs, False)
    for seg, q, e, _ in _flat(errs):
        assert e <= FP32_BOUND, (seg, q, e)


@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_cpu_segments_match_fp64_frozen_bn(name):
    """Frozen BN (folded conv epilogues): the conv / fc gradients and dx against the eval-BN mirror."""
    errs = _cpu_errors(name, (64, 64), frozen=True)
    _expected_quantities(name, errs, True)
    for seg, q, e, _ in _flat(errs):
        assert e <= FP32_BOUND, (seg, q, e)


# ----------------------------------------------------------------------------- b. the yardstick
def _mirror_yardsticks(name, hw):
    torch.manual_seed(0)
    model64 = build_model(name, num_classes=10).double()
    image = torch.randn(8, 3, *hw, dtype=torch.float64)
    labels = torch.randint(0, 10, (8,))
    cap, g_rounded = M.mirror_capture_step(model64, image, labels, True, torch.bfloat16)
    ref = M.segment_grads(model64, cap, True, None)
    rnd = M.segment_grads(model64, cap, True, torch.bfloat16)
    yard = {(seg, q): M.rel_l2(rnd[seg][q], g) for seg, qs in ref.items() for q, g in qs.items()}
    return model64, image, labels, g_rounded, yard


@pytest.mark.parametrize("hw", [(64, 64), (96, 64)])
@pytest.mark.parametrize("name", ["resnet50", "resnext50_32x4d", "resnet18"])
def test_yardstick_usable(name, hw):
    """Purely in the fp64 mirror: a step of the bf16-storage mirror supplies the captures, and each
    segment's bf16-storage gradients are within 0.2 of its exact fp64 ones on the same tensors
    (measured: blocks <= 0.13, stem <= 0.10, head 3e-3) -- the cap is a condition for the per-segment
    bounds below to mean anything.  For ResNet-50 the same rounding model moves the WHOLE-model
    gradient by more than 3x the worst segment (printed; measured ~1.2 against 0.13): end-to-end
    bf16 gradient bounds in training mode are vacuous, a zero gradient has error 1.0."""
    model64, image, labels, g_rounded, yard = _mirror_yardsticks(name, hw)
    worst = max(yard, key=yard.get)
    print(f"{name} {hw}: worst yardstick {worst} {yard[worst]:.3e}")
    for key, y in yard.items():
        assert y <= 0.2, (key, y)
    if name == "resnet50":
        _, g_exact = M.mirror_capture_step(model64, image, labels, True, None)
        names = sorted(g_exact)
        whole = M.rel_l2(torch.cat([g_rounded[n].flatten() for n in names]),
                         torch.cat([g_exact[n].flatten() for n in names]))
        blocks = max(y for (seg, _), y in yard.items() if seg not in ("stem", "head"))
        print(f"{name} {hw}: whole-model bf16-storage gradient error {whole:.3f}, worst block yardstick {blocks:.3f}")
        assert whole >= 3 * blocks, (whole, blocks)


# ----------------------------------------------------------------------------- c. sensitivity (CPU, fp32 path)
def _split(errs):
    dx = {seg: e for seg, q, e, _ in _flat(errs) if q == "dx"}
    rest = [(seg, q, e) for seg, q, e, _ in _flat(errs) if q != "dx"]
    return dx, rest


def test_dropped_residual_deposit_is_seen(monkeypatch):
    """GradJoin.deposit losing its argument (the residual / downsample gradient never reaches the
    block input): the block input gradients are wrong by > 0.1, every parameter gradient -- each
    follows from the gradient the block actually received -- stays exact."""
    def deposit(self, g):
        self.arrived += 1
        return None

    monkeypatch.setattr(Fn.GradJoin, "deposit", deposit)
    dx, rest = _split(_cpu_errors("resnet50", (64, 64)))
    assert max(dx.values()) > 0.1, dx
    for seg, q, e in rest:
        assert e <= FP32_BOUND, (seg, q, e)


def test_shifted_strided_deposit_is_seen(monkeypatch):
    """StridedGrad.full scattering onto the odd pixels (96 x 64 input: stage 4 is 3 pixels high):
    the stride-2 projection blocks' input gradients are wrong by > 0.1, everything else stays exact.
    With the dgrad-epilogue BN backward on, conv1's epilogue adds the compact deposit itself and
    ``full`` is never called (asserted: the mutation is inert there), so the mutated step runs with
    ``set_bn_backward_fusion(False)``, where the claimed deposit is expanded by ``full``."""
    def full(self):
        N, _, _, C = self.compact.shape
        out = self.compact.new_zeros((N, self.H, self.W, C))
        out[:, 1::2, 1::2, :] = self.compact
        return out

    monkeypatch.setattr(Fn.StridedGrad, "full", full)
    assert max(e for _, _, e, _ in _flat(_cpu_errors("resnet50", (96, 64)))) <= FP32_BOUND
    prev = Fn._FUSE_BN_BWD[0]
    Fn.set_bn_backward_fusion(False)
    try:
        dx, rest = _split(_cpu_errors("resnet50", (96, 64)))
    finally:
        Fn.set_bn_backward_fusion(prev)
    strided = {"layer2.0", "layer3.0", "layer4.0"}
    assert min(dx[s] for s in strided) > 0.1, dx
    for seg, q, e in rest + [(s, "dx", e) for s, e in dx.items() if s not in strided]:
        assert e <= FP32_BOUND, (seg, q, e)


def test_unfused_shortcut_bn_is_the_same():
    """Control: the projection shortcut's BN as a pass of its own changes no result."""
    prev = Fn.shortcut_bn_fusion()
    Fn.set_shortcut_bn_fusion(False)
    try:
        errs = _cpu_errors("resnet50", (64, 64))
    finally:
        Fn.set_shortcut_bn_fusion(prev)
    for seg, q, e, _ in _flat(errs):
        assert e <= FP32_BOUND, (seg, q, e)


# ----------------------------------------------------------------------------- GPU
F_BF16 = 2.2     # see test_gpu_segments_within_bf16_yardstick
FLOOR = 1e-2     # the kernel tests' bf16 tolerance for a single conv
CAP = 0.25
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _build(name, classes):
    if name == "bottleneck1111":  # the smallest net with every projection-block path
        return R.ResNet(R.Bottleneck, [1, 1, 1, 1], num_classes=classes)
    return build_model(name, num_classes=classes)


def _gpu_errors(name, hw, frozen=False, check_input=None):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = _build(name, 100)
    if frozen:
        M.frozen_copy(model)
    model64 = copy.deepcopy(model).double()
    model = model.to(dev)
    imgs = torch.randint(0, 256, (8, 3, *hw), dtype=torch.uint8, device=dev)
    labels = torch.randint(0, 100, (8,), device=dev)
    x = Fn.to_device_nhwc(imgs, MEAN, STD, nchw=True, in_scale=1 / 255.0, **input_layout(model))
    if check_input is not None:
        check_input(x)

    def step(m):
        Fn.cross_entropy(m(x), labels).backward()

    return M.teacher_forced_errors(model, model64, step, training=not frozen, labels=labels)


def _violations(errs, report=None):
    bad = []
    for seg, q, e, y in _flat(errs):
        if report is not None:
            print(f"{report} {seg}.{q}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f}")
        if not (e <= max(F_BF16 * y, FLOOR) and e <= CAP):
            bad.append((seg, q, e, y))
    return bad


class _Config:
    """One switch setting of the wiring, restored on exit."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.saved = (Fn._FUSE_PLAIN[0], Fn._PLAIN_FUSE_MAX[0], Fn._FUSE_BN_BWD[0], Fn._STRIDED_DEPOSIT[0],
                      Fn.bn_prologue_enabled(), Fn.bn_prologue3x3_enabled(), R._FUSED_STEM[0])
        if self.name == "plain_bn_separate":  # the path the benchmark's b1024 / b4096 layers take
            Fn.set_plain_bn_backward_fusion(False, max_elems=0)
        elif self.name == "plain_bn_fused":
            Fn.set_plain_bn_backward_fusion(True)
        elif self.name == "bn_backward_unfused":
            Fn.set_bn_backward_fusion(False)
        elif self.name == "full_size_deposit":
            Fn.set_strided_deposit(False)
        elif self.name == "no_bn_prologue":
            Fn.set_bn_prologue(False)
            Fn.set_bn_prologue3x3(False)
        elif self.name == "bn_prologue_1x1":  # opt-in: bn2 + ReLU inside conv3's GEMMs
            Fn.set_bn_prologue(True)
        elif self.name == "unfused_stem":
            R._FUSED_STEM[0] = False
        else:
            assert self.name == "default"
        return self

    def __exit__(self, *exc):
        plain, pmax, bnbwd, strided, pro, pro3, stem = self.saved
        Fn.set_plain_bn_backward_fusion(plain, max_elems=pmax)
        Fn.set_bn_backward_fusion(bnbwd)
        Fn.set_strided_deposit(strided)
        Fn.set_bn_prologue(pro)
        Fn.set_bn_prologue3x3(pro3)
        R._FUSED_STEM[0] = stem
        return False


GPU_MODELS = ["resnet50", "resnext50_32x4d", "resnet18", "bottleneck1111"]
CONFIGS = ["default", "plain_bn_separate", "plain_bn_fused", "bn_backward_unfused", "full_size_deposit",
           "no_bn_prologue", "bn_prologue_1x1", "unfused_stem"]


@pytest.mark.gpu
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("hw", [(64, 64), (96, 64)])
@pytest.mark.parametrize("name", GPU_MODELS)
def test_gpu_segments_within_bf16_yardstick(name, hw, config):
    """One bf16 training step on the HIP kernels: per quantity of every segment,
    err_ours <= max(F * yardstick, 1e-2) and err_ours <= 0.25, both errors against the fp64 mirror
    of that segment on the captured tensors, the yardstick being the bf16-storage mirror's.
    F = 2.2: the default configuration measured on the MI355X is tabulated in
    profiles/r7/teacher_forced_block_grads.txt; the largest err_ours / yardstick there is 1.449
    (a BN weight gradient at 3.2e-2 against 2.2e-2; the kernels round at other points than the
    yardstick does), and F is 1.5 x that, rounded up to one decimal.  Nothing measured above 2."""
    def fused_stem_runs(x):
        if config == "default" and hw == (64, 64):
            assert Fn.stem_bn_pool_fusable(x)

    with _Config(config):
        errs = _gpu_errors(name, hw, check_input=fused_stem_runs)
    bad = _violations(errs, report=f"{name} {hw} {config}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(64, 64), (96, 64)])
@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_gpu_segments_within_bf16_yardstick_frozen_bn(name, hw):
    """Frozen BN folded into the conv epilogues, same bound; conv / fc gradients and dx."""
    errs = _gpu_errors(name, hw, frozen=True)
    assert all("bn" not in q and "downsample.1" not in q for _, q, _, _ in _flat(errs))
    bad = _violations(errs, report=f"{name} {hw} frozen")
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_bound_sees_dropped_residual_deposit(monkeypatch):
    """The bf16 bound still discriminates: with GradJoin.deposit losing its argument the bounded
    check fails, on block input gradients."""
    def deposit(self, g):
        self.arrived += 1
        return None

    monkeypatch.setattr(Fn.GradJoin, "deposit", deposit)
    bad = _violations(_gpu_errors("resnet50", (64, 64)))
    assert bad and all(q == "dx" for _, q, _, _ in bad), bad
    assert max(e for _, _, e, _ in bad) > CAP
