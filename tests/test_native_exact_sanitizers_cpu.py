"""The exact entry point of the native shard loader (csrc/host/loader.cpp:dcpl_submit_exact, the
`pil` resampling mode) under AddressSanitizer + UBSan and under ThreadSanitizer:
tests/native/loader_exact_sanitize.cpp is a stand-alone program that includes loader.cpp, keeps
every batch in flight on an 8-thread pool and frees its geometry buffers.  It runs as a child
process with the caller's environment plus the sanitizers' own option variables; no Python code
runs under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ddp_classification_pytorch_amd.data.shards import write_shard

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "native", "loader_exact_sanitize.cpp")
CXX = shutil.which("g++") or shutil.which("clang++")
# what a sanitizer runtime prints when it cannot start in this process environment at all
REFUSED = ("runtime does not come first in initial library list", "unexpected memory mapping",
           "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "failed to allocate")


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    rng = np.random.default_rng(3)
    imgs = [(rng.integers(0, 256, (int(rng.integers(8, 60)), int(rng.integers(8, 60)), 3), dtype=np.uint8), i)
            for i in range(53)]
    p = str(tmp_path_factory.mktemp("san_exact") / "s.dcps")
    write_shard(p, imgs)
    return p


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_exact_loader_under_sanitizer(tmp_path, shard, san):
    exe = str(tmp_path / f"loader_exact_{san.split(',')[0]}")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={san}", "-fno-omit-frame-pointer",
           "-ffp-contract=off", DRIVER, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr or "").lower():
        pytest.skip(f"{san} sanitizer runtime unavailable: {r.stderr[-300:]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, shard], capture_output=True, text=True, env=env, timeout=300)
    out = run.stdout + run.stderr
    if run.returncode != 0 and "loader_exact_sanitize" not in out and any(m in out for m in REFUSED):
        pytest.skip(f"{san} runtime refused to start: {out[-300:]}")
    assert run.returncode == 0, out[-3000:]
    assert "loader_exact_sanitize ok=1" in out
    assert "ERROR: AddressSanitizer" not in out and "WARNING: ThreadSanitizer" not in out
    assert "runtime error" not in out
