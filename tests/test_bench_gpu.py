"""bench.py's command line on one GPU, at a toy size:

* a plain ``--gpus 1`` run times exactly ``--steps`` steps, prints one JSON line with
  ``ms_per_step``, and ``--dump-outputs`` writes the last step's loss, gradients, parameters and
  BN running statistics as float32 ``.npy`` files of at most 64 MB in all, the same from run to
  run whatever ``--steps`` and ``--warmup`` are;
* the diagnostic phases of a data-parallel run (SyncBN phases, bucket telemetry, collective probe)
  run only with ``--full`` (``tests/test_ddp_gpu.py`` covers them there)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = ["--batch", "8", "--image-size", "64", "--model", "resnet18", "--num-classes", "10", "--no-autotune"]


def _bench(args, env):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """One plain run with --dump-outputs: (JSON record, dump directory), shared and left unchanged."""
    d = tmp_path_factory.mktemp("bench") / "dump"
    rec = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)] + TOY, dict(os.environ))
    return rec, d


def test_bench_plain_run_dumps_outputs(dumped):
    rec, d = dumped
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["ms_per_step"] > 0
    # value and ms_per_step describe the same 3 timed steps of 8 images
    assert rec["value"] == pytest.approx(8 / (rec["ms_per_step"] * 1e-3), rel=1e-3)
    files = sorted(os.listdir(d))
    assert files == ["bn_running_stats.npy", "grads.npy", "loss.npy", "params.npy"]
    arrs = {f[:-4]: np.load(d / f) for f in files}
    assert all(a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
    assert arrs["loss"].shape == (1,) and float(arrs["loss"][0]) == pytest.approx(rec["config"]["final_loss"], abs=1e-4)
    # ResNet-18 with 10 classes: 11,181,642 parameters, more than bench.DUMP_MAX_ELEMS, so the fixed
    # sample of that size; every BN running mean / variance (4,800 channels), unsampled
    assert arrs["params"].size == 4 * 2**20 and arrs["bn_running_stats"].size == 2 * 4800
    assert arrs["grads"].size == 4 * 2**20
    assert np.abs(arrs["params"]).max() > 0 and np.abs(arrs["grads"]).max() > 0


def _assert_same_dump(d1, d2):
    """Bound: with the same kernels only the summation order of weight-gradient atomics could differ
    between two processes.  An fp32 sum of K terms in another order moves by at most K * 2^-24
    relative to the sum of magnitudes, ~sqrt(K) * 2^-24 typically; K <= 8 * 32 * 32 here (images x
    output pixels), so 1e-4 relative L2 leaves a factor of ten over 2^-24 * 128.  The forward has no
    atomics: the loss and the BN statistics get the same bound without needing it.  The parameters
    move by lr = 0.1 times the gradient's difference."""
    for name in ("loss", "grads", "params", "bn_running_stats"):
        a, b = np.load(d1 / (name + ".npy")).astype(np.float64), np.load(d2 / (name + ".npy")).astype(np.float64)
        rel = np.linalg.norm(a - b) / np.linalg.norm(a)
        print(name, "relative L2 between two runs:", rel, "max |a - b|:", np.abs(a - b).max())
        assert rel <= 1e-4, (name, rel)


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_bench_dump_is_reproducible(dumped, tmp_path, mode):
    """Another process with other --steps and --warmup dumps the same arrays, because the dumped
    step starts from the seeded state again.  The shared run makes 3 steps before the dumped one
    (HIP graph: 1 warm-up step, the capture runs nothing, 2 replays); these make 6 (graph) and 5
    (eager, where the restore must also mark the cached bf16 weights stale), so a restore that
    left weights, momentum or BN statistics behind would show as a different trajectory."""
    _, d1 = dumped
    d2 = tmp_path / "dump"
    args = {"graph": ["--steps", "4", "--warmup", "3", "--graph"], "eager": ["--steps", "4", "--warmup", "2", "--eager"]}
    rec = _bench(["--gpus", "1", "--dump-outputs", str(d2)] + args[mode] + TOY, dict(os.environ))
    assert rec["config"]["hip_graph"] == (mode == "graph")
    assert rec["config"]["dump_tuning"] == {"replayed": 0, "timed": 0}  # --no-autotune
    _assert_same_dump(d1, d2)


def test_bench_dump_with_replayed_autotuning(tmp_path):
    """The autotuner on: a first process times the toy shapes and records its decisions
    (DCP_TUNE_CACHE), a second replays them, times nothing, and dumps the same arrays -- the
    mechanism by which the committed table makes headline dumps repeatable."""
    env = dict(os.environ, DCP_TUNE_CACHE=str(tmp_path / "tune.txt"))
    env.pop("DCP_AUTOTUNE", None)
    toy = [x for x in TOY if x != "--no-autotune"]
    d1, d2 = tmp_path / "a", tmp_path / "b"
    r1 = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d1)] + toy, dict(env))
    t1 = r1["config"]["dump_tuning"]
    assert r1["config"]["autotune"] is True and t1["replayed"] == 0 and t1["timed"] > 0
    r2 = _bench(["--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d2)] + toy, dict(env))
    assert r2["config"]["dump_tuning"] == {"replayed": t1["timed"], "timed": 0}
    _assert_same_dump(d1, d2)


def test_bench_plain_ddp_run_skips_diagnostics():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    rec = _bench(["--force-ddp", "--steps", "2", "--warmup", "1"] + TOY, env)
    assert rec["dist_backend"] == "nccl" and rec["world_size"] == 1 and rec["value"] > 0
    assert rec["syncbn_value"] is None and rec["syncbn_peer_value"] is None
    assert rec["comm"] is None and rec["comm_probe"] is None and "diagnostic_errors" not in rec
