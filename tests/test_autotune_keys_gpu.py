"""The autotuner's problem keys, its cache text and its tuned launches, pinned from outside.

Recorded tuning caches (``DCP_TUNE_CACHE`` files, ``bench_dump_tuning.txt``) name a conv problem by the
key the library builds for it, so the keys are an interface: a key that changes silently turns every
recorded decision into a miss.  Every expected key below is written out by hand from the format strings
of ``launch_tap_gemm`` (conv_igemm.hip) and ``conv_wgrad`` (bindings.cpp), never read back from the
build under test:

* tap GEMM: ``N Hs Ws Cs Co T Hd Wd Hy Wy ss ds oy ox ntaps|<stats><bias><relu><addsrc><bnb><aff>|`` then
  ``dy,dx,widx;`` per tap, then ``|s2:<Cs2>,<bias2>`` with a second source.  ``bnb`` is 1 for a fused
  BN backward that recomputes the mask, 2 with mask bits, 3 with mask bits and no BN input.
* weight gradient: ``N Ho Wo Co H W C KH KW stride pad``.

Shapes: N = 2 on 8 x 8 pixels (one 128-row tile), channels multiples of 64 (only those are tuned).

The tuned call against the heuristic: every tap-GEMM candidate accumulates an output in the same k order,
so the bf16 conv outputs are compared with ``torch.equal``.  The two exceptions the sources name do not
arise here: split-K of the 128-row kernels needs >= 16 64-deep k-units (tg_split_slices) and the deepest
problem here, 9 taps of 64 channels, has 9; the BN statistics of a 64-channel tile are not compared.
The weight gradients have at most 128 GEMM rows, one split under every plan (a split is >= 256 rows), and
the 32- and 64-row k-tiles both feed the MFMAs 32 rows at a time in row order: the fp32 results are
compared with ``torch.equal`` as well.
"""
import os

import pytest
import torch

from ddp_classification_pytorch_amd import _ext, tuning

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "ddp_classification_pytorch_amd", "bench_dump_tuning.txt")

FWD_TAPS_3X3 = "-1,-1,0;-1,0,1;-1,1,2;0,-1,3;0,0,4;0,1,5;1,-1,6;1,0,7;1,1,8;"


def _bf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF16).to(DEV)


def _cases(K):
    """name -> (callable returning the bf16 / fp32 GEMM output, kind, expected keys)"""
    g = torch.Generator().manual_seed(11)
    x64 = _bf(g, 2, 8, 8, 64)
    x64b = _bf(g, 2, 8, 8, 64)
    dy128 = _bf(g, 2, 8, 8, 128)
    dy128s = _bf(g, 2, 4, 4, 128)
    w1 = _bf(g, 128, 1, 1, 64, scale=0.125)
    w3 = _bf(g, 64, 3, 3, 64, scale=0.04)
    w3g = _bf(g, 128, 3, 3, 64, scale=0.04)
    wt1 = _bf(g, 64, 1, 1, 128, scale=0.09)
    wt3 = _bf(g, 64, 3, 3, 128, scale=0.03)
    wcat = _bf(g, 128, 128, scale=0.09)
    wlin = _bf(g, 128, 64, scale=0.125)
    xlin = _bf(g, 2, 64)
    res128 = _bf(g, 2, 8, 8, 128)
    add64 = _bf(g, 2, 8, 8, 64)
    y64 = _bf(g, 2, 8, 8, 64)
    mask = torch.randint(0, 256, (2, 8, 8, 8), generator=g, dtype=torch.uint8).to(DEV)
    vec = lambda n: torch.randn(n, generator=g).to(DEV)
    sc128, sh128, b128, blin = vec(128), vec(128), vec(128), vec(128)
    sc, sh, mean = vec(64), vec(64), vec(64)
    invstd = (torch.randn(64, generator=g).abs() + 0.5).to(DEV)
    bn = lambda y, m: K.conv_dgrad_bn(dy128, wt1, 0, None, y, None, sc, sh, mean, invstd, 1, m, 0.0)[0]
    return {
        "conv_fwd_1x1": (lambda: K.conv_fwd(x64, w1, 1, 0, True)[0], "tg",
                         ["2 8 8 64 128 1 8 8 8 8 1 1 0 0 1|100000|0,0,0;"]),
        "conv_fwd_3x3_s2": (lambda: K.conv_fwd(x64, w3, 2, 1, True)[0], "tg",
                            ["2 8 8 64 64 9 4 4 4 4 2 1 0 0 9|100000|" + FWD_TAPS_3X3]),
        "conv_fwd_affine": (lambda: K.conv_fwd_affine(x64, w1, 1, 0, sc128, sh128, 1, 0.0, res128), "tg",
                            ["2 8 8 64 128 1 8 8 8 8 1 1 0 0 1|000101|0,0,0;"]),
        "conv_fwd_geo": (lambda: K.conv_fwd_geo(x64, w3g, 1, 1, 8, 8, False)[0], "tg",
                         ["2 8 8 64 128 9 8 8 8 8 1 1 0 0 9|000000|" + FWD_TAPS_3X3]),
        "conv_dgrad_s1_add": (lambda: K.conv_dgrad(dy128, wt1, 8, 8, 1, 0, add64), "tg",
                              ["2 8 8 128 64 1 8 8 8 8 1 1 0 0 1|000100|0,0,0;"]),
        "conv_dgrad_s2": (lambda: K.conv_dgrad(dy128s, wt3, 8, 8, 2, 1, None), "tg",
                          ["2 4 4 128 64 9 8 8 4 4 1 2 0 0 1|000000|0,0,4;",
                           "2 4 4 128 64 9 8 8 4 4 1 2 0 1 2|000000|0,1,3;0,0,5;",
                           "2 4 4 128 64 9 8 8 4 4 1 2 1 0 2|000000|1,0,1;0,0,7;",
                           "2 4 4 128 64 9 8 8 4 4 1 2 1 1 4|000000|1,1,0;1,0,2;0,1,6;0,0,8;"]),
        "conv_dgrad_bn_recompute": (lambda: bn(y64, None), "tg",
                                    ["2 8 8 128 64 1 8 8 8 8 1 1 0 0 1|000010|0,0,0;"]),
        "conv_dgrad_bn_mask": (lambda: bn(y64, mask), "tg", ["2 8 8 128 64 1 8 8 8 8 1 1 0 0 1|000020|0,0,0;"]),
        "conv_dgrad_bn_mask_no_y": (lambda: bn(None, mask), "tg",
                                    ["2 8 8 128 64 1 8 8 8 8 1 1 0 0 1|000030|0,0,0;"]),
        "conv1x1_cat": (lambda: K.conv1x1_cat(x64, x64b, wcat, b128), "tg",
                        ["2 8 8 64 128 1 8 8 8 8 1 1 0 0 1|000000|0,0,0;|s2:64,1"]),
        "linear_fwd": (lambda: K.linear_fwd(xlin, wlin, blin, 1), "tg",
                       ["2 1 1 64 128 1 1 1 1 1 1 1 0 0 1|011000|0,0,0;"]),
        "conv_wgrad_1x1": (lambda: K.conv_wgrad(dy128, x64, 1, 1, 1, 0), "wg", ["2 8 8 128 8 8 64 1 1 1 0"]),
        "conv_wgrad_3x3_s2": (lambda: K.conv_wgrad(dy128s, x64, 3, 3, 2, 1), "wg", ["2 4 4 128 8 8 64 3 3 2 1"]),
    }


@pytest.fixture(scope="module")
def tuned():
    """Every op once with the autotuner on, once with it off; the export text after the tuned calls."""
    K = _ext.hip_ops()
    cases = _cases(K)
    tuning.apply(K, "autotune=1", reset=True)
    try:
        out_tuned = {name: fn().clone() for name, (fn, _, _) in cases.items()}
        torch.cuda.synchronize()
        export = K.autotune_export()
        entries = K.autotune_entries()
    finally:
        tuning.apply(K, "", reset=True)
    out_heur = {name: fn().clone() for name, (fn, _, _) in cases.items()}
    torch.cuda.synchronize()
    return K, cases, out_tuned, out_heur, export, entries


NAMES = ["conv_fwd_1x1", "conv_fwd_3x3_s2", "conv_fwd_affine", "conv_fwd_geo", "conv_dgrad_s1_add", "conv_dgrad_s2",
         "conv_dgrad_bn_recompute", "conv_dgrad_bn_mask", "conv_dgrad_bn_mask_no_y", "conv1x1_cat", "linear_fwd",
         "conv_wgrad_1x1", "conv_wgrad_3x3_s2"]


def test_case_list_is_complete(tuned):
    assert sorted(NAMES) == sorted(tuned[1])


@pytest.mark.parametrize("name", NAMES)
def test_key_is_exported_verbatim(tuned, name):
    _, cases, _, _, export, entries = tuned
    _, kind, keys = cases[name]
    lines = export.split("\n")
    for key in keys:
        hits = [ln for ln in lines if ln.startswith(f"{kind}\t{key}\t")]
        assert len(hits) == 1, (name, key, [ln for ln in lines if ln.startswith(kind + "\t2 ")])
        choice = hits[0].rsplit("\t", 1)[1]
        assert choice.isdigit(), hits[0]
    assert entries == len([ln for ln in lines if ln])


@pytest.mark.parametrize("name", NAMES)
def test_tuned_call_equals_heuristic(tuned, name):
    _, _, out_tuned, out_heur, _, _ = tuned
    a, b = out_tuned[name], out_heur[name]
    assert a.dtype == b.dtype and a.shape == b.shape
    assert bool(b.float().abs().sum() > 0), "the reference output is all zeros"
    assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())


def test_recorded_cache_replays(tuned):
    """All 88 recorded decisions are accepted and come back out line for line."""
    K = tuned[0]
    with open(DUMP) as f:
        text = f.read()
    lines = [ln for ln in text.split("\n") if ln and not ln.startswith("#")]
    assert len(lines) == 88
    assert K.autotune_import(text) == 88
    out = set(K.autotune_export().split("\n"))
    missing = [ln for ln in lines if ln not in out]
    assert not missing, missing


def test_import_skips_bad_lines(tuned):
    K = tuned[0]
    before = K.autotune_entries()
    text = ("tg\t7777 1 1 64 64 1 1 1 1 1 1 1 0 0 1|000000|0,0,0;\t999\n"  # past the tap-GEMM table
            "tg\t7777 1 1 64 64 1 1 1 1 1 1 1 0 0 1|000001|0,0,0;\t-1\n"
            "wg\t7777 1 1 64 1 1 64 1 1 1 0\t999\n"  # past the weight-gradient table
            "wg\t7777 1 1 64 1 1 64 1 1 1 1\t-1\n"
            "7777 1 1 64 64 1 1 1 1 1 1 1 0 0 1|000000|0,0,0; 1\n"  # no tab at all
            "tg\t7777 1 1 64 64 1 1 1 1 1 1 1 0 0 1|000010|0,0,0;\n"  # a key without a choice
            "wg\t7777 1 1 64 1 1 64 1 1 1 2\n"
            "tg\t7777 1 1 64 64 1 1 1 1 1 1 1 0 0 1|000100|0,0,0;\t1\n"  # the two good ones
            "wg\t7777 1 1 64 1 1 64 1 1 1 3\t2")
    assert K.autotune_import(text) == 2
    assert K.autotune_entries() == before + 2
    out = K.autotune_export().split("\n")
    assert "tg\t7777 1 1 64 64 1 1 1 1 1 1 1 0 0 1|000100|0,0,0;\t1" in out
    assert "wg\t7777 1 1 64 1 1 64 1 1 1 3\t2" in out
    assert len([ln for ln in out if ln.startswith(("tg\t7777 ", "wg\t7777 "))]) == 2
