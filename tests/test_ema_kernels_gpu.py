"""mt_ema / mt_swap (csrc/optim.hip) through optim.WeightEMA on the GPU.

* Lattice (tests/ema_ref.py): torch.equal to the fp64 oracle after each of the 5 updates -- single
  tensors around the 16-byte path's and the chunk's edges, one tensor of 301 chunks, 70 tensors of
  1..70 elements in one launch.
* Views at float offsets 0..3 of the live tensor, of the average and of both give the bits of the
  aligned run (16-byte against 4-byte path).
* Random inputs: every element within the derived two-rounding bound
  2^-24 (omd |w - e| + |E|) (1 + 2^-22) of the fp64 value; the worst ratio is printed.
* e == w is a fixed point; a skipped optimizer step (ClipCtl.skip) leaves every average untouched.
* mt_swap copies bit patterns (NaN payloads, -0.0, denormals), twice is the identity.
* Nothing outside a view is written: every buffer is compared whole outside its view.
"""
import pytest
import torch

from tests import ema_ref as R

pytestmark = pytest.mark.gpu
CANARY = 12345.0


def _dev():
    return torch.device("cuda", 0)


def _hold(values, off):
    """A device buffer holding ``values`` as a view at float offset ``4 + off`` of a 16-byte aligned
    allocation, every other element a canary -> (buffer, view)."""
    n = values.numel()
    buf = torch.full((4 + off + n + 4,), CANARY, dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    view = buf[4 + off:4 + off + n]
    view.view(torch.int32).copy_(R.bits(values).to(_dev()))
    return buf, view


def _canaries_intact(buf, view):
    start = (view.data_ptr() - buf.data_ptr()) // 4
    out = torch.cat([buf[:start], buf[start + view.numel():]])
    return bool((out == CANARY).all())


def _ema(pairs, **kw):
    from ddp_classification_pytorch_amd.optim import WeightEMA

    return WeightEMA.from_pairs(pairs, **kw)


def _setup(ws, es, ow=0, oe=0, **kw):
    hw = [_hold(w, ow) for w in ws]
    he = [_hold(e, oe) for e in es]
    ema = _ema([(w[1], e[1]) for w, e in zip(hw, he)], **kw)
    return ema, hw, he


def _set(holds, values):
    for (_, view), v in zip(holds, values):
        view.copy_(v.to(_dev()))


CASES = {f"n{n}": (n,) for n in R.SINGLE_SIZES}
CASES["chunks301"] = (R.MANY_CHUNKS,)
CASES["small70"] = R.SMALL_MANY


# ----------------------------------------------------------------------------- 1. the lattice
@pytest.mark.parametrize("case", list(CASES))
def test_lattice_equals_the_fp64_oracle_after_every_step(case):
    sizes = CASES[case]
    for k in (1, 2, 3):
        ks = (k,) * R.T
        e0, ws = R.lattice(sizes, seed=10 * k + len(sizes))
        want = R.oracle(e0, ws, [2.0 ** -k] * R.T, lattice_ks=ks)
        ema, hw, he = _setup(ws[0], e0, decay=1 - 2.0 ** -k)
        for t in range(R.T):
            _set(hw, ws[t])
            ema.update()
            for i, ((_, view), w) in enumerate(zip(he, want[t])):
                assert torch.equal(view.cpu(), w), (k, t, i)
        assert ema.num_updates == R.T
        for (bw, vw), (be, ve), w in zip(hw, he, ws[-1]):
            assert _canaries_intact(bw, vw) and _canaries_intact(be, ve)
            assert torch.equal(vw.cpu(), w)  # the live tensor is only read


def test_lattice_follows_an_omd_that_changes_every_step():
    ks = (1, 2, 3, 2, 1)
    sizes = (5, 4096, 2 * 4096 + 5)
    e0, ws = R.lattice(sizes, steps=len(ks), seed=7)
    want = R.oracle(e0, ws, [2.0 ** -k for k in ks], lattice_ks=ks)
    ema, hw, he = _setup(ws[0], e0, decay=0.5)
    for t, k in enumerate(ks):
        _set(hw, ws[t])
        ema.decay = 1 - 2.0 ** -k
        ema.update()
        for (_, view), w in zip(he, want[t]):
            assert torch.equal(view.cpu(), w), t
    assert ema.pushes == len(ks)  # 1/2, 1/4, 1/8, 1/4, 1/2: every step wrote the device scalar


# ----------------------------------------------------------------------------- 2. alignment
def _random(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in sizes], [torch.randn(n, generator=g) for n in sizes]


OFFSETS = [(o, 0) for o in range(1, 4)] + [(0, o) for o in range(1, 4)] + [(o, o) for o in range(1, 4)] + [(1, 2)]


@pytest.fixture(scope="module")
def aligned_run():
    ws, es = _random(R.SINGLE_SIZES, seed=5)
    ema, hw, he = _setup(ws, es, decay=0.9)
    ema.update()
    ema.update()
    upd = [R.bits(v).cpu() for _, v in he]
    ema.swap()
    swp = ([R.bits(v).cpu() for _, v in hw], [R.bits(v).cpu() for _, v in he])
    return ws, es, upd, swp


@pytest.mark.parametrize("ow,oe", OFFSETS)
def test_views_at_odd_float_offsets_give_the_aligned_bits(aligned_run, ow, oe):
    ws, es, upd, swp = aligned_run
    ema, hw, he = _setup(ws, es, ow=ow, oe=oe, decay=0.9)
    ema.update()
    ema.update()
    for i, (_, v) in enumerate(he):
        assert torch.equal(R.bits(v).cpu(), upd[i]), i
    ema.swap()
    for i, ((bw, vw), (be, ve)) in enumerate(zip(hw, he)):
        assert torch.equal(R.bits(vw).cpu(), swp[0][i]) and torch.equal(R.bits(ve).cpu(), swp[1][i]), i
        assert _canaries_intact(bw, vw) and _canaries_intact(be, ve), i


# ----------------------------------------------------------------------------- 3. random inputs, the bound
MIXED = tuple([1, 2, 3, 5, 7, 63, 64, 65, 255, 1023, 1024, 1025, 4095, 4096, 4097, 5000, 8192, 9001, 12288, 20001]
              + list(range(10, 60)))


@pytest.mark.parametrize("decay", [0.9998, 0.9])
def test_random_inputs_within_the_two_rounding_bound(decay):
    assert len(MIXED) == 70
    ws, es = _random(MIXED, seed=11)
    omd = R.omd_of(decay, 0, False)
    if decay == 0.9:
        assert omd == float(torch.tensor(0.1, dtype=torch.float32))
    ema, hw, he = _setup(ws, es, decay=decay)
    ema.update()
    assert float(ema._omd) == omd
    worst = 0.0
    for (_, view), w, e in zip(he, ws, es):
        worst = max(worst, R.worst_ratio(view.cpu(), w, e, omd))
    print(f"decay {decay}: worst |error| / bound = {worst:.4f}")
    assert worst <= 1.0
    for (bw, vw), (be, ve) in zip(hw, he):
        assert _canaries_intact(bw, vw) and _canaries_intact(be, ve)


# ----------------------------------------------------------------------------- 4. fixed point, skip
def test_equal_average_is_a_fixed_point():
    ws = [R.nasty(n, seed=n) for n in (5, 4096, 4097 + 4096)]
    # every finite value, denormals included (inf - inf is NaN by definition; IEEE's (-0) - (-0) is +0)
    ws = [torch.where(torch.isfinite(w) & (R.bits(w) != -0x80000000), w, torch.ones_like(w)) for w in ws]
    ema, hw, he = _setup(ws, ws, decay=0.9998)
    for _ in range(3):
        ema.update()
    for (_, view), w in zip(he, ws):
        assert torch.equal(R.bits(view).cpu(), R.bits(w))


def test_skipped_optimizer_step_leaves_every_average_untouched():
    from ddp_classification_pytorch_amd.optim import FusedSGD

    sizes = (5, 4096, 4097 + 4096)
    ws, es = _random(sizes, seed=21)
    ps = [torch.nn.Parameter(w.to(_dev())) for w in ws]
    opt = FusedSGD(ps, lr=0.1, momentum=0.9, skip_nonfinite=True)
    he = [_hold(e, 0) for e in es]
    ema = _ema([(p.detach(), e[1]) for p, e in zip(ps, he)], decay=0.9, optimizer=opt)
    for p in ps:
        p.grad = torch.ones_like(p)
    p_bad = ps[2].grad
    p_bad[4096] = float("inf")     # the first element of a second chunk
    before_p = [p.detach().clone() for p in ps]
    opt.step()
    ema.update()
    assert int(opt.skipped_steps()) == 1 and ema.num_updates == 1
    for p, b, (buf, view), e in zip(ps, before_p, he, es):
        assert torch.equal(p.detach(), b)
        assert torch.equal(R.bits(view).cpu(), R.bits(e)) and _canaries_intact(buf, view)
    # a finite step: the optimizer steps and the average follows again
    p_bad[4096] = 1.0
    opt.step()
    ema.update()
    omd = R.omd_of(0.9, 1, False)
    assert int(opt.skipped_steps()) == 1 and ema.num_updates == 2
    for p, b, (buf, view), e in zip(ps, before_p, he, es):
        assert not torch.equal(p.detach(), b)
        assert not torch.equal(view.cpu(), e)
        assert R.worst_ratio(view.cpu(), p.detach().cpu(), e, omd) <= 1.0
        assert _canaries_intact(buf, view)


# ----------------------------------------------------------------------------- 5. the exchange
@pytest.mark.parametrize("case", list(CASES))
def test_swap_copies_bit_patterns_and_twice_is_the_identity(case):
    sizes = CASES[case]
    ws = [R.nasty(n, seed=2 * i) for i, n in enumerate(sizes)]
    es = [R.nasty(n, seed=2 * i + 1) for i, n in enumerate(sizes)]
    ema, hw, he = _setup(ws, es)
    ema.swap()
    for (bw, vw), (be, ve), w, e in zip(hw, he, ws, es):
        assert torch.equal(R.bits(vw).cpu(), R.bits(e)) and torch.equal(R.bits(ve).cpu(), R.bits(w))
        assert _canaries_intact(bw, vw) and _canaries_intact(be, ve)
    ema.swap()
    for (bw, vw), (be, ve), w, e in zip(hw, he, ws, es):
        assert torch.equal(R.bits(vw).cpu(), R.bits(w)) and torch.equal(R.bits(ve).cpu(), R.bits(e))
        assert _canaries_intact(bw, vw) and _canaries_intact(be, ve)


def test_applied_restores_on_an_exception_and_refuses_an_update_inside():
    ws, es = [R.nasty(4099, seed=1)], [R.nasty(4099, seed=2)]
    ema, hw, he = _setup(ws, es, ow=1, oe=3)
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            assert torch.equal(R.bits(hw[0][1]).cpu(), R.bits(es[0]))
            1 / 0
    assert torch.equal(R.bits(hw[0][1]).cpu(), R.bits(ws[0])) and torch.equal(R.bits(he[0][1]).cpu(), R.bits(es[0]))
    with pytest.raises(RuntimeError, match="inside applied"):
        with ema.applied():
            ema.update()
    assert torch.equal(R.bits(he[0][1]).cpu(), R.bits(es[0]))


def test_ops_check_their_tables():
    from ddp_classification_pytorch_amd import _ext

    ops = _ext.hip_ops()
    omd = torch.full((1,), 0.5, device=_dev())
    bad = torch.zeros(2, 5, dtype=torch.int64, device=_dev())
    chunks = torch.zeros(0, 2, dtype=torch.int32, device=_dev())
    with pytest.raises(RuntimeError, match="table int64"):
        ops.mt_ema(bad, chunks, omd, None)
    with pytest.raises(RuntimeError, match="table int64"):
        ops.mt_swap(bad, chunks)
