"""The autotuner decisions that ``bench.py --dump-outputs`` replays for the headline shapes
(``ddp_classification_pytorch_amd/bench_dump_tuning.txt``) belong to the candidate tables in the
sources: its entries are indices into them, so the file carries their fingerprint."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_tuning_table_matches_candidate_tables():
    bench = _bench()
    with open(bench.DUMP_TUNE_CACHE) as f:
        lines = f.read().splitlines()
    assert lines[0] == "# candidate tables " + bench.candidate_tables_fingerprint()
    body = lines[1:]
    assert body and body == sorted(body) and len(set(body)) == len(body)
    with open(os.path.join(ROOT, "ddp_classification_pytorch_amd", "csrc", "bindings.cpp")) as f:
        text = f.read()
    i = text.index("kWgCfgs[] = {")
    n_wg = text[i:text.index("};", i)].count("{") - 1
    for ln in body:
        kind, key, choice = ln.split("\t")
        assert kind in ("tg", "wg") and key and re.fullmatch(r"\d+", choice), ln
        if kind == "wg":
            assert int(choice) < n_wg, ln


def test_fingerprint_ignores_comments_and_spacing(tmp_path, monkeypatch):
    bench = _bench()
    want = bench.candidate_tables_fingerprint()
    csrc = tmp_path / "ddp_classification_pytorch_amd" / "csrc"
    csrc.mkdir(parents=True)
    src = os.path.join(ROOT, "ddp_classification_pytorch_amd", "csrc")
    for name in ("conv_igemm.hip", "bindings.cpp"):
        with open(os.path.join(src, name)) as f:
            text = f.read()
        (csrc / name).write_text(text.replace("kTgCfgs[] = {", "kTgCfgs[] = {  // a remark\n"))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.candidate_tables_fingerprint() == want
    text = (csrc / "bindings.cpp").read_text()
    (csrc / "bindings.cpp").write_text(text.replace("kWgCfgs[] = {{0, 0, 0, 0, 0},", "kWgCfgs[] = {{0, 0, 0, 0, 0}, {3, 0, 0, 0, 0},"))
    assert bench.candidate_tables_fingerprint() != want
