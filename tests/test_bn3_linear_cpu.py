"""The algebra behind the linear bn3 backward (csrc/bn_lin.hip), in fp64 on the CPU against autograd.

For x3 = a2 W3^T (a 1x1 conv as a matrix product over n rows) followed by a training-mode BN, with g
the gradient at the BN's output, S1 = sum g, S2 = sum g xhat, a = gamma istd, b = -gamma istd^2 S2 / n
(in units of x3 - mean) and e = a S1 / n:

    d_a2 = g (diag(a) W3) + a2 Q + bias,   Q = W3^T diag(b) W3,   bias = -colmean(a2) Q - e W3
    dW3  = diag(a) (g^T a2) + diag(b) W3 (a2^T a2 - n colmean^T colmean) - e (x) colsum(a2)
    dgamma = S2, dbeta = S1

Bounds.  Every entry is a sum of at most L = n + C + m products, so its fp64 round-off is at most
L u (u = 2^-53) times the sum of the magnitudes of its terms; BN backward subtracts means, which
inflates that against the norm of the result by the cancellation it performs.  The bound on the
relative L2 error is 100 L u (margin 100 for that cancellation, about 5e-12 here): eleven orders
below any wiring mistake (a wrong sign or a dropped term is an error of order 1), and it does not
come from the formulas under test (they measure ~1e-15).
"""
import pytest
import torch

N_ROWS, M_IN, C_OUT = 392, 16, 64
U = 2.0 ** -53
BOUND = 100 * (N_ROWS + C_OUT + M_IN) * U
EPS = 1e-5


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _problem(mean_over_sigma=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    a2 = torch.relu(rnd(N_ROWS, M_IN)) + mean_over_sigma * rnd(1, M_IN).abs()
    W3 = rnd(C_OUT, M_IN) / M_IN ** 0.5
    gamma, beta = rnd(C_OUT).abs() + 0.5, rnd(C_OUT)
    gout = rnd(N_ROWS, C_OUT)
    return a2, W3, gamma, beta, gout


def _autograd(a2, W3, gamma, beta, gout):
    a2, W3, gamma, beta = (t.clone().requires_grad_(True) for t in (a2, W3, gamma, beta))
    x3 = a2 @ W3.t()
    y = torch.nn.functional.batch_norm(x3, None, None, gamma, beta, training=True, eps=EPS)
    y.backward(gout)
    return a2.grad, W3.grad, gamma.grad, beta.grad


def _coefficients(a2, W3, gamma, gout):
    n = a2.shape[0]
    x3 = a2 @ W3.t()
    mean, var = x3.mean(0), x3.var(0, unbiased=False)
    istd = (var + EPS).rsqrt()
    S1, S2 = gout.sum(0), (gout * (x3 - mean) * istd).sum(0)
    a = gamma * istd
    return n, a, -gamma * istd * istd * S2 / n, a * S1 / n, S1, S2


def test_linear_bn_backward_matches_autograd():
    a2, W3, gamma, beta, gout = _problem()
    d_a2, dW3, dgamma, dbeta = _autograd(a2, W3, gamma, beta, gout)
    n, a, b, e, S1, S2 = _coefficients(a2, W3, gamma, gout)
    cs = a2.sum(0)
    Q = W3.t() @ (b[:, None] * W3)
    bias = -(cs / n) @ Q - e @ W3
    got_dx = gout @ (a[:, None] * W3) + a2 @ Q + bias
    cov = a2.t() @ a2 - torch.outer(cs, cs) / n
    got_dw = a[:, None] * (gout.t() @ a2) + b[:, None] * (W3 @ cov) - torch.outer(e, cs)
    errs = {"d_a2": _rel(got_dx, d_a2), "dW3": _rel(got_dw, dW3), "dgamma": _rel(S2, dgamma), "dbeta": _rel(S1, dbeta)}
    print(errs, "bound", BOUND)
    for k, v in errs.items():
        assert v <= BOUND, (k, v)


@pytest.mark.parametrize("mean_over_sigma", [3.0, 30.0])
def test_centred_bias_with_rounded_q(mean_over_sigma):
    """The GEMM multiplies a2 with Qr = bf16(Q).  With the bias taken from the SAME rounded matrix,
    d_a2 = g aW3 + (a2 - colmean) Qr - e W3 exactly, so the rounding of Q meets only the centred
    a2: err_c = |(a2 - colmean) dQ| <= |a2 - colmean|_F |dQ|_F.  A bias from the unrounded Q leaves
    a2 dQ whole; the two parts are orthogonal (the centred one has zero column means), so
    err_u^2 = err_c^2 + n |colmean dQ|^2 -- asserted as an identity, to round-off."""
    a2, W3, gamma, beta, gout = _problem(mean_over_sigma, seed=1)
    d_a2, _, _, _ = _autograd(a2, W3, gamma, beta, gout)
    n, a, b, e, _, _ = _coefficients(a2, W3, gamma, gout)
    cm = a2.mean(0)
    Q = W3.t() @ (b[:, None] * W3)
    Qr = Q.to(torch.bfloat16).double()
    lin = gout @ (a[:, None] * W3) - e @ W3
    centred = lin + a2 @ Qr - cm @ Qr
    uncentred = lin + a2 @ Qr - cm @ Q
    same = lin + (a2 - cm) @ Qr
    assert _rel(centred, same) <= BOUND
    dQ = Qr - Q
    err_c, err_u = (centred - d_a2).norm().item(), (uncentred - d_a2).norm().item()
    slack = BOUND * d_a2.norm().item()
    assert err_c <= (a2 - cm).norm().item() * dQ.norm().item() + slack
    want_u = (err_c ** 2 + n * (cm @ dQ).norm().item() ** 2) ** 0.5
    print(f"mean/sigma {mean_over_sigma}: centred {err_c:.3e} uncentred {err_u:.3e} (predicted {want_u:.3e})")
    assert abs(err_u - want_u) <= 1e-6 * want_u + slack
    assert err_c <= err_u + slack
