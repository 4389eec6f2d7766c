"""The weight EMA on the CPU path (optim/ema.py over ops/_ref.py), its decay schedule, exchange,
persistence, the CLI refusal, and main.py --model-ema end to end (log, checkpoint, resume).

The lattice (tests/ema_ref.py) is exact: torch.equal to the fp64 oracle after each of the 5 updates.
Sensitivity of the checks is shown, not assumed: the alternative form (1 - omd) e + omd w exceeds the
two-rounding bound on standard-normal data (measured: 2.36 of the bound; the defined form: 0.998), and
an update that drops a tensor's last element or uses the previous step's omd leaves the lattice oracle.
"""
import json
import os

import pytest
import torch

from tests import ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ema(pairs, **kw):
    from ddp_classification_pytorch_amd.optim import WeightEMA

    return WeightEMA.from_pairs(pairs, **kw)


def _run_lattice(sizes, ks, seed):
    e0, ws = R.lattice(sizes, steps=len(ks), seed=seed)
    want = R.oracle(e0, ws, [2.0 ** -k for k in ks], lattice_ks=ks)
    live = [w.clone() for w in ws[0]]
    avg = [e.clone() for e in e0]
    ema = _ema(list(zip(live, avg)), decay=1 - 2.0 ** -ks[0])
    got = []
    for t, k in enumerate(ks):
        for dst, src in zip(live, ws[t]):
            dst.copy_(src)
        ema.decay = 1 - 2.0 ** -k
        ema.update()
        got.append([a.clone() for a in avg])
    return got, want, ws, e0


@pytest.mark.parametrize("ks", [(1,) * 5, (2,) * 5, (3,) * 5, (1, 2, 3, 2, 1)], ids=str)
def test_lattice_is_exact_on_the_cpu_path(ks):
    got, want, _, _ = _run_lattice((1, 3, 4, 5, 4097, 2 * 4096 + 5), ks, seed=sum(ks))
    for t, (g_t, w_t) in enumerate(zip(got, want)):
        for i, (g, w) in enumerate(zip(g_t, w_t)):
            assert torch.equal(g, w), (t, i)


def test_lattice_catches_a_dropped_last_element_and_a_stale_omd():
    ks = (1, 2, 3, 2, 1)
    sizes = (5, 4097)
    e0, ws = R.lattice(sizes, steps=len(ks), seed=3)
    want = R.oracle(e0, ws, [2.0 ** -k for k in ks], lattice_ks=ks)
    # (a) the last element of every tensor never updated
    cur = [e.clone() for e in e0]
    for t, k in enumerate(ks):
        for e, w in zip(cur, ws[t]):
            e[:-1] += 2.0 ** -k * (w[:-1] - e[:-1])
    assert all(not torch.equal(c, w) for c, w in zip(cur, want[-1]))
    assert all(torch.equal(c[:-1], w[:-1]) for c, w in zip(cur, want[-1]))
    # (b) every step uses the omd of the step before it
    cur = [e.clone() for e in e0]
    for t in range(len(ks)):
        k = ks[max(t - 1, 0)]
        for e, w in zip(cur, ws[t]):
            e += 2.0 ** -k * (w - e)
    assert all(not torch.equal(c, w) for c, w in zip(cur, want[-1]))


@pytest.mark.parametrize("fault", ["drops_last_element", "stale_omd"])
def test_lattice_comparison_catches_a_broken_cpu_path(monkeypatch, fault):
    """The same comparison as test_lattice_is_exact_on_the_cpu_path, run against the package with its
    CPU kernel broken on purpose: it must not pass."""
    from ddp_classification_pytorch_amd.ops import _ref

    real, seen = _ref.mt_ema, []

    def broken(pairs, omd, skip=False):
        if fault == "drops_last_element":
            return real([(w[:-1], e[:-1]) for w, e in pairs], omd, skip)
        seen.append(omd.clone())
        return real(pairs, seen[max(len(seen) - 2, 0)], skip)  # the omd of the step before

    monkeypatch.setattr(_ref, "mt_ema", broken)
    ks = (1, 2, 3, 2, 1)
    got, want, _, _ = _run_lattice((5, 4097), ks, seed=3)
    assert all(not torch.equal(g, w) for g, w in zip(got[-1], want[-1]))
    monkeypatch.setattr(_ref, "mt_ema", real)
    got, want, _, _ = _run_lattice((5, 4097), ks, seed=3)
    assert all(torch.equal(g, w) for g, w in zip(got[-1], want[-1]))


def test_random_inputs_within_the_two_rounding_bound_and_the_other_form_is_not():
    g = torch.Generator().manual_seed(0)
    n = 100_000
    w, e = torch.randn(n, generator=g), torch.randn(n, generator=g)
    omd = R.omd_of(0.9998, 0, False)
    avg = e.clone()
    ema = _ema([(w, avg)], decay=0.9998)
    ema.update()
    defined = R.worst_ratio(avg, w, e, omd)
    o32 = torch.tensor(omd, dtype=torch.float32)
    other = (1 - o32) * e + o32 * w          # fp32 throughout: three roundings and a rounded 1 - omd
    alt = R.worst_ratio(other, w, e, omd)
    print(f"worst error / bound: defined form {defined:.3f}, (1 - omd) e + omd w {alt:.3f}")
    assert defined <= 1.0
    assert alt > 1.0


@pytest.mark.parametrize("warmup", [False, True])
def test_decay_schedule_and_pushes(warmup):
    w = torch.zeros(4)
    ema = _ema([(w, torch.zeros(4))], decay=0.99, warmup=warmup)
    seen, pushes = [], []
    for n in range(41):
        assert ema.num_updates == n
        ema.push_decay()
        ema.push_decay()                       # nothing changed: no second write
        seen.append(float(ema._omd))
        pushes.append(ema.pushes)
        ema.update()
    want = [R.omd_of(0.99, n, warmup) for n in range(41)]
    assert seen == want
    if warmup:
        d = [min(0.99, (1 + n) / (10 + n)) for n in range(41)]
        assert d[0] == 0.1 and d[40] == 41 / 50 and all(x < 0.99 for x in d)
    changes = 1 + sum(1 for a, b in zip(want, want[1:]) if a != b)
    assert pushes[-1] == changes and pushes[0] == 1
    assert changes == (41 if warmup else 1)


def test_equal_average_is_a_fixed_point():
    w = R.nasty(4099, seed=1)
    # every finite value, denormals included; inf - inf is NaN by definition, and IEEE's (-0) - (-0) = +0
    # turns an average of -0.0 into +0.0 (equal as numbers)
    w = torch.where(torch.isfinite(w) & (R.bits(w) != -0x80000000), w, torch.ones_like(w))
    avg = w.clone()
    ema = _ema([(w, avg)], decay=0.9998)
    ema.update()
    assert torch.equal(R.bits(avg), R.bits(w))


def test_applied_exchanges_and_restores_every_bit():
    w, e = R.nasty(4100, seed=2), R.nasty(4100, seed=3)
    w0, e0 = R.bits(w).clone(), R.bits(e).clone()
    ema = _ema([(w, e)], names=["x"])
    with ema.applied():
        assert torch.equal(R.bits(w), e0) and torch.equal(R.bits(e), w0)
        assert torch.equal(R.bits(ema.average_of("x")), e0)  # the average is wherever its bits are
    assert torch.equal(R.bits(w), w0) and torch.equal(R.bits(e), e0)
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            1 / 0
    assert torch.equal(R.bits(w), w0) and torch.equal(R.bits(e), e0)


def test_applied_bumps_the_weight_generation():
    from ddp_classification_pytorch_amd.ops import functional as Fn

    ema = _ema([(torch.zeros(3), torch.ones(3))])
    g0 = Fn._GEN[0]
    with ema.applied():
        assert Fn._GEN[0] == g0 + 1
    assert Fn._GEN[0] == g0 + 2


def test_capture_rules(monkeypatch):
    """While the current stream is capturing: no exchange, no creation of the device scalar; an update
    whose scalar exists launches without pushing."""
    from ddp_classification_pytorch_amd.optim import ema as E

    ema = _ema([(torch.ones(3), torch.zeros(3))], decay=0.5)
    monkeypatch.setattr(E, "_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        ema.swap()
    with pytest.raises(RuntimeError, match="captured"):
        with ema.applied():
            pass
    with pytest.raises(RuntimeError, match="before capture"):
        ema.update()
    with pytest.raises(RuntimeError, match="before capture"):
        ema.push_decay()
    assert ema.num_updates == 0
    monkeypatch.setattr(E, "_capturing", lambda: False)
    ema.update()                                   # eager: creates the scalar, omd = 0.5
    ema.decay = 0.75                               # the next push would write omd = 0.25
    monkeypatch.setattr(E, "_capturing", lambda: True)
    ema.update()                                   # "captured": reads the scalar as it is (0.75, not 0.625)
    assert ema.pushes == 1 and ema.num_updates == 2
    assert torch.equal(ema.average_of("0"), torch.full((3,), 0.75))
    ema.on_graph_replay()
    assert ema.num_updates == 3


def _tiny_model():
    from ddp_classification_pytorch_amd.models import build_model

    torch.manual_seed(0)
    return build_model("cifar_resnet18", num_classes=10)


def test_tracks_fp32_state_and_carries_integer_buffers_live():
    from ddp_classification_pytorch_amd.optim import WeightEMA

    m = _tiny_model()
    ema = WeightEMA(m, decay=0.5)
    sd = m.state_dict()
    fp = [k for k, v in sd.items() if v.dtype == torch.float32]
    assert ema.keys() == ["model." + k for k in fp] and len(fp) < len(sd)
    for k in fp:
        assert torch.equal(ema.average_of("model." + k), sd[k])
        assert ema.average_of("model." + k).data_ptr() != sd[k].data_ptr()
    bn = next(x for x in m.modules() if hasattr(x, "_nbt_pending"))
    bn._nbt_pending += 3
    out = ema.state_dict()
    assert list(out["averages"]) == ["model." + k for k in sd]
    name = next(k for k, v in m.named_modules() if v is bn)
    assert int(out["averages"][f"model.{name}.num_batches_tracked"]) == 3
    fresh = _tiny_model()
    fresh.load_state_dict(ema.model_state_dict("model"))  # strict: every key is there
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        WeightEMA.from_pairs([(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        WeightEMA.from_pairs([(torch.zeros(4, 4).t(), torch.zeros(4, 4))])


def test_state_dict_round_trip_into_a_fresh_object():
    from ddp_classification_pytorch_amd.optim import WeightEMA

    m = _tiny_model()
    ema = WeightEMA({"net": m}, decay=0.75, warmup=True)
    for _ in range(3):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p))
        ema.update()
    state = ema.state_dict()
    other = WeightEMA({"net": _tiny_model()}, decay=0.5)
    ptrs = [other.average_of(k).data_ptr() for k in other.keys()]
    other.load_state_dict(state)
    assert other.num_updates == 3 and other.decay == 0.75 and other.warmup is True
    assert ptrs == [other.average_of(k).data_ptr() for k in other.keys()]  # copied into, never rebound
    for k in ema.keys():
        assert torch.equal(other.average_of(k), ema.average_of(k)), k
    other.push_decay()
    assert float(other._omd) == R.omd_of(0.75, 3, True)
    bad = dict(state, averages={k: v for k, v in list(state["averages"].items())[1:]})
    with pytest.raises(KeyError):
        other.load_state_dict(bad)


def test_cpu_update_honours_the_optimizers_skip():
    from ddp_classification_pytorch_amd.optim import FusedSGD, WeightEMA

    p = torch.nn.Parameter(torch.ones(8))
    opt = FusedSGD([p], lr=0.5, skip_nonfinite=True)
    ema = WeightEMA.from_pairs([(p.detach(), p.detach().clone())], decay=0.5, optimizer=opt)
    p.grad = torch.full((8,), float("inf"))
    opt.step()
    with torch.no_grad():
        p.add_(1.0)            # the live tensor moved (as BN statistics do in a skipped step)
    ema.update()
    assert torch.equal(ema.average_of("0"), torch.ones(8)) and ema.num_updates == 1
    p.grad = torch.ones(8)
    opt.step()
    ema.update()
    assert torch.equal(ema.average_of("0"), torch.full((8,), 1.25)) and ema.num_updates == 2


@pytest.mark.parametrize("workload", ["nested", "plc"])
@pytest.mark.parametrize("flags,named", [(["--model-ema"], "--model-ema"),
                                         (["--model-ema-decay", "0.9"], "--model-ema-decay"),
                                         (["--model-ema-warmup"], "--model-ema-warmup")])
def test_refuse_ema_names_the_flag(workload, flags, named):
    from ddp_classification_pytorch_amd.config import build_parser, refuse_ema

    args = build_parser().parse_args(["--workload", workload] + flags)
    with pytest.raises(ValueError, match=named) as ei:
        refuse_ema(args, workload)
    assert workload in str(ei.value)
    refuse_ema(build_parser().parse_args(["--workload", workload]), workload)  # no flag: nothing raised


def test_flag_defaults():
    from ddp_classification_pytorch_amd.config import build_parser
    from ddp_classification_pytorch_amd.optim import build_ema

    a = build_parser().parse_args([])
    assert a.model_ema is False and a.model_ema_decay == 0.9998 and a.model_ema_warmup is False
    assert build_ema(a, {"model": torch.nn.Linear(2, 2)}) is None


# ----------------------------------------------------------------------------- main.py end to end
def _main(out, extra):
    import main as entry

    torch.manual_seed(0)
    entry.main(["--workload", "baseline", "--data", "synthetic", "--model", "resnet18", "--dataset", "CIFAR10",
                "--device", "cpu", "--batchsize", "8", "--max-steps-per-epoch", "3", "--synthetic-train-size", "32",
                "--synthetic-val-size", "16", "--workers", "0", "--log-interval", "1", "--out-dir", str(out)] + extra)
    with open(os.path.join(out, "metrics.jsonl")) as f:
        recs = [json.loads(line) for line in f]
    return recs, torch.load(os.path.join(out, "last.pth"), map_location="cpu", weights_only=True)


@pytest.fixture(scope="module")
def main_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ema_main")
    ema = ["--model-ema", "--model-ema-decay", "0.9"]
    full = _main(d / "full", ["--epochs", "2"] + ema)
    _main(d / "split", ["--epochs", "1"] + ema)
    resumed = _main(d / "split", ["--epochs", "2", "--auto-resume"] + ema)
    plain = _main(d / "plain", ["--epochs", "2"])
    return {"full": full, "resumed": resumed, "plain": plain}


def test_main_logs_val_ema_and_checkpoints_the_average(main_runs):
    recs, ck = main_runs["full"]
    ve = [r for r in recs if r["kind"] == "val_ema"]
    assert [r["epoch"] for r in ve] == [0, 1] and [r["updates"] for r in ve] == [3, 6]
    assert [r["epoch"] for r in recs if r["kind"] == "val"] == [0, 1]
    assert all(r["loss"] == r["loss"] and r["count"] == 16 for r in ve)
    e = ck["ema"]
    assert e["n"] == 6 and e["decay"] == 0.9 and e["warmup"] is False
    live = ck["models"]["model"]
    assert list(e["averages"]) == ["model." + k for k in live]
    moved = sum(1 for k, v in live.items() if v.dtype == torch.float32 and not torch.equal(v, e["averages"]["model." + k]))
    assert moved > 20                                        # an average, not a copy of the live weights
    assert "ema" not in main_runs["plain"][1]


def test_main_resume_continues_the_average(main_runs):
    a, b = main_runs["full"][1]["ema"], main_runs["resumed"][1]["ema"]
    assert a["n"] == b["n"] == 6
    assert list(a["averages"]) == list(b["averages"])
    for k, v in a["averages"].items():
        assert torch.equal(v, b["averages"][k]), k
    assert [r["updates"] for r in main_runs["resumed"][0] if r["kind"] == "val_ema"] == [3, 6]


def test_main_live_model_is_untouched_by_the_average(main_runs):
    a, b = main_runs["full"][1]["models"]["model"], main_runs["plain"][1]["models"]["model"]
    assert list(a) == list(b) and len(a) > 20
    for k, v in a.items():
        assert torch.equal(v, b[k]), k
