"""Reference of the weight EMA (csrc/optim.hip: mt_ema / mt_swap; optim/ema.py), shared by
test_ema_cpu.py, test_ema_kernels_gpu.py and test_ema_graph_gpu.py.

    t  = fl32(w - e)
    e' = fl32(e + omd t)          (one fused multiply-add)

against the real-number value E = e + omd (w - e).  Two roundings: |t_fl - t| <= u |t| enters E scaled
by omd, the fused multiply-add rounds its own result once,

    |e' - E| <= u (omd |w - e| + |E|) (1 + 2^-22),      u = 2^-24

(the last factor covers the second-order terms, and the CPU path's fp64 intermediate).

The lattice: omd = 2^-k and every entry of e_0 and of every w_t an integer in [-64, 64] times one
common power of two.  After T updates an average is an integer multiple of 2^-(kT) of that unit and at
most 64 of it in magnitude (7 + kT bits); a difference w - e is at most 128 of it (8 + kT bits).  With
sum of k over the steps + 8 <= 24 every t and every e' is an fp32 number: the fp32 chain IS the fp64
oracle, bit for bit, whatever the order of evaluation.  The oracle asserts that precondition and that
each of its values survives a round trip through fp32.
"""
import numpy as np
import torch

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -22
CHUNK = 4096
T = 5

# single tensors around the 16-byte path's and the chunk's edges, and more than two chunks
SINGLE_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 5)
MANY_CHUNKS = 300 * 4096 + 77     # 301 chunks
SMALL_MANY = tuple(range(1, 71))  # 70 tensors of 1..70 elements in one launch


def omd_of(decay, n, warmup):
    """fl32(1 - d_n), d_n = min(decay, (1 + n) / (10 + n)) under warm-up: fp64, rounded once."""
    d = min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay
    return float(np.float32(1.0 - d))


def lattice(sizes, steps=T, seed=0, unit_pow=-3):
    """(e_0, [w_1 .. w_T]): lists of fp32 tensors, integers in [-64, 64] times 2^unit_pow."""
    g = torch.Generator().manual_seed(seed)
    unit = 2.0 ** unit_pow

    def draw():
        return [(torch.randint(-64, 65, (n,), generator=g).to(torch.float32) * unit) for n in sizes]

    return draw(), [draw() for _ in range(steps)]


def check_lattice(e0, ws, ks, unit_pow=-3):
    assert sum(ks) + 8 <= 24, "lattice precondition: sum of k over the steps + 8 <= 24"
    assert len(ks) == len(ws)
    unit = 2.0 ** unit_pow
    for ts in [e0] + list(ws):
        for t in ts:
            q = t.to(torch.float64) / unit
            assert bool((q == q.round()).all()) and bool((q.abs() <= 64).all()), "not on the lattice"


def oracle(e0, ws, omds, lattice_ks=None, unit_pow=-3):
    """The fp64 chain E_t = E_{t-1} + omd_t (w_t - E_{t-1}): a list over the steps of lists of fp64
    tensors.  With ``lattice_ks`` (omd_t = 2^-k_t) the lattice precondition is asserted and every value
    must be an fp32 number; the returned tensors are then fp32."""
    if lattice_ks is not None:
        check_lattice(e0, ws, lattice_ks, unit_pow)
        assert [float(o) for o in omds] == [2.0 ** -k for k in lattice_ks]
    cur = [e.to(torch.float64) for e in e0]
    out = []
    for w_t, omd in zip(ws, omds):
        cur = [e + float(omd) * (w.to(torch.float64) - e) for e, w in zip(cur, w_t)]
        if lattice_ks is not None:
            for e in cur:
                assert torch.equal(e.to(torch.float32).to(torch.float64), e), "oracle value is not an fp32 number"
            out.append([e.to(torch.float32) for e in cur])
        else:
            out.append([e.clone() for e in cur])
    return out


def one_step64(w, e, omd):
    """E = e + omd (w - e) in fp64 from fp32 inputs."""
    e64 = e.to(torch.float64)
    return e64 + float(omd) * (w.to(torch.float64) - e64)


def bound(w, e, omd):
    """The two-rounding bound per element (fp64)."""
    e64, w64 = e.to(torch.float64), w.to(torch.float64)
    return U * (float(omd) * (w64 - e64).abs() + one_step64(w, e, omd).abs()) * SLACK


def worst_ratio(got, w, e, omd):
    """max over the elements of |got - E| / bound (0 / 0 counts as 0)."""
    err = (got.to(torch.float64) - one_step64(w, e, omd)).abs()
    b = bound(w, e, omd)
    off = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    r = torch.where(b > 0, err / b.clamp_min(1e-300), off)
    return float(r.max()) if r.numel() else 0.0


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def nasty(n, seed=0):
    """fp32 bit patterns that arithmetic would change: NaN payloads, -0.0, denormals, infinities,
    mixed into random normals."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    # quiet / signalling / negative NaN payloads, -0.0, the smallest and largest denormal, a negative
    # denormal, +inf, -inf -- written through an integer view: copies of bits, never float moves
    special = torch.tensor([0x7FC00001, 0x7F800123, -0x00400000, -0x80000000, 0x00000001, 0x007FFFFF,
                            -0x7FFFFFFF, 0x7F800000, -0x00800000], dtype=torch.int64).to(torch.int32)
    idx = torch.randperm(n, generator=g)[:min(n, special.numel())]
    x.view(torch.int32)[idx] = special[:idx.numel()]
    return x
