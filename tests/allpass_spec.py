"""The specification of all-pass warping (csrc/allpass.hip, nn.AllPassWarp, AllPassWarpLayer) written out in numpy,
float64 unless another dtype is asked for -- the same lines in float32 are the GPU tests' yardstick for what float32
can hold -- plus a differentiable torch twin whose gradients come from autograd, and the reference's closed-form
coefficient table restated from the formula in the docstring of its gen_w_matrix_3d.

For one frame with warping factor a, W(a) is N x N:
    W[0][0] = 1,  W[0][c] = 0 (c >= 1),  W[r][0] = a W[r-1][0],  W[r][c] = W[r-1][c-1] + a (W[r-1][c] - W[r][c-1])
    dW[r][0] = a dW[r-1][0] + W[r-1][0]
    dW[r][c] = dW[r-1][c-1] + (W[r-1][c] - W[r][c-1]) + a (dW[r-1][c] - dW[r][c-1])
A row of D = nb * N features is nb blocks; block b gives y_b = x_b' W with x_b' = x_b, its first coefficient halved
for b < 3 and y_b[0] doubled afterwards; with normalisation x is first taken as x * std_dev + mean and y written as
(y - mean) / std_dev."""
import math
from fractions import Fraction

import numpy as np
import torch


def warp_matrices(a, N, dtype=np.float64):
    """(W [M, N, N], dW/da [M, N, N]) for the factors a [M], every operation in `dtype`"""
    a = np.asarray(a, dtype=dtype)
    M = a.shape[0]
    W = np.zeros((M, N, N), dtype=dtype)
    dW = np.zeros((M, N, N), dtype=dtype)
    W[:, 0, 0] = 1
    for r in range(1, N):
        W[:, r, 0] = a * W[:, r - 1, 0]
        dW[:, r, 0] = a * dW[:, r - 1, 0] + W[:, r - 1, 0]
        for c in range(1, N):
            t = W[:, r - 1, c] - W[:, r, c - 1]
            W[:, r, c] = W[:, r - 1, c - 1] + a * t
            dW[:, r, c] = dW[:, r - 1, c - 1] + t + a * (dW[:, r - 1, c] - dW[:, r, c - 1])
    return W, dW


def closed_form_table(N):
    """[N, N, 2N] float64: table[r, c, p] = coefficient of a^p in W[r][c], from the reference's formula
        A(m, k) = 1 / (k-1)! * sum_{n = max(0, k-m)}^{k} (k choose n) (m+n-1)! / (m+n-k)! (-1)^(n+k+m) a^(2n+m-k)
    for k >= 1 (factorials of non-positive numbers taken as 1), A(0, 0) = 1 and A(m, 0) = 0 otherwise, with
    W[r][c] = A(m = c, k = r): the reference stores A[m, k], transposes it and multiplies the feature row from the
    left.  Exact rational arithmetic until the final conversion; powers from 2N on are cut as the reference cuts
    them (there are none: the degree is at most r + c <= 2N - 2)."""
    def fact(i):
        return math.factorial(i) if i > 0 else 1

    table = np.zeros((N, N, 2 * N), dtype=np.float64)
    table[0, 0, 0] = 1.0
    for m in range(N):
        for k in range(1, N):
            for n in range(max(0, k - m), k + 1):
                coeff = Fraction(math.comb(k, n) * (-1) ** (n + m + k) * fact(m + n - 1), fact(m + n - k) * fact(k - 1))
                degree = 2 * n + m - k
                if degree < 2 * N:
                    table[k, m, degree] = float(coeff)
    return table


def closed_form_matrices(a, N, dtype=np.float64):
    """W [M, N, N] from the table, evaluated in `dtype` as the reference does: table and powers of a cast, one sum"""
    a = np.asarray(a, dtype=dtype)
    powers = np.cumprod(np.concatenate([np.ones((a.shape[0], 1), dtype=dtype),
                                        np.repeat(a[:, None], 2 * N - 1, axis=1)], axis=1), axis=1)
    return np.einsum("ijk,lk->lij", closed_form_table(N).astype(dtype), powers)


def _edge(D, N, value, dtype):
    """[D] ones with `value` at the first coefficient of blocks 0..2"""
    e = np.ones(D, dtype=dtype)
    e[0:3 * N:N] = value
    return e


def forward(x, a, N, mean=None, std_dev=None, dtype=np.float64):
    """y [M, D] of x [M, D] warped by a [M]"""
    x = np.asarray(x, dtype=dtype)
    M, D = x.shape
    assert D % N == 0
    W, _ = warp_matrices(a, N, dtype)
    if std_dev is not None:
        x = x * np.asarray(std_dev, dtype=dtype)
    if mean is not None:
        x = x + np.asarray(mean, dtype=dtype)
    xp = (x * _edge(D, N, 0.5, dtype)).reshape(M, D // N, N)
    y = np.einsum("mbr,mrc->mbc", xp, W).astype(dtype).reshape(M, D) * _edge(D, N, 2.0, dtype)
    if mean is not None:
        y = y - np.asarray(mean, dtype=dtype)
    if std_dev is not None:
        y = y / np.asarray(std_dev, dtype=dtype)
    return y


def backward(dy, x, a, N, mean=None, std_dev=None, dtype=np.float64):
    """(dx [M, D], da [M, nb]: each block's share of dL/da, their sum over the blocks is the gradient) for
    dy = dL/dy.  Blocks do not mix in y and dx, so a call on the first k blocks is the first k blocks of this."""
    x = np.asarray(x, dtype=dtype)
    g = np.asarray(dy, dtype=dtype)
    M, D = x.shape
    W, dW = warp_matrices(a, N, dtype)
    if std_dev is not None:
        x = x * np.asarray(std_dev, dtype=dtype)
        g = g / np.asarray(std_dev, dtype=dtype)
    if mean is not None:
        x = x + np.asarray(mean, dtype=dtype)
    xp = (x * _edge(D, N, 0.5, dtype)).reshape(M, D // N, N)
    gp = (g * _edge(D, N, 2.0, dtype)).reshape(M, D // N, N)
    dxp = np.einsum("mbc,mrc->mbr", gp, W).astype(dtype).reshape(M, D)
    da = np.einsum("mbr,mbc,mrc->mb", xp, gp, dW).astype(dtype)
    dx = dxp * _edge(D, N, 0.5, dtype)
    if std_dev is not None:
        dx = dx * np.asarray(std_dev, dtype=dtype)
    return dx, da


# ---------------------------------------------------------------------------------------- torch twin
def torch_warp_matrix(a, N):
    """W [M, N, N] in a's dtype, differentiable in a [M]"""
    zero = 0 * a          # (tied to a, so that a gradient exists at N = 1 too: zeros)
    one = zero + 1
    rows = [[one] + [zero] * (N - 1)]
    for r in range(1, N):
        row = [a * rows[r - 1][0]]
        for c in range(1, N):
            row.append(rows[r - 1][c - 1] + a * (rows[r - 1][c] - row[c - 1]))
        rows.append(row)
    return torch.stack([torch.stack(row, dim=-1) for row in rows], dim=-2)


def torch_forward(x, a, N, mean=None, std_dev=None):
    """y with x's leading shape [.., D] and a [.., 1] or [..]; differentiable in x and a, in x's dtype"""
    shape = x.shape
    D = shape[-1]
    x2 = x.reshape(-1, D)
    W = torch_warp_matrix(a.reshape(-1).to(x.dtype), N)
    if std_dev is not None:
        x2 = x2 * std_dev.to(x.dtype)
    if mean is not None:
        x2 = x2 + mean.to(x.dtype)
    half = torch.from_numpy(_edge(D, N, 0.5, np.float64)).to(x.dtype)
    two = torch.from_numpy(_edge(D, N, 2.0, np.float64)).to(x.dtype)
    xp = (x2 * half).reshape(-1, D // N, N)
    y = torch.einsum("mbr,mrc->mbc", xp, W).reshape(-1, D) * two
    if mean is not None:
        y = y - mean.to(x.dtype)
    if std_dev is not None:
        y = y / std_dev.to(x.dtype)
    return y.reshape(shape)


def combine(alphas):
    """the reference's combination of successive warps: reduce((a1 + a2) / (1 + a1 a2))"""
    out = alphas[0]
    for alpha in alphas[1:]:
        out = (out + alpha) / (1 + out * alpha)
    return out


# ---------------------------------------------------------------------------------------- the tests' tolerance rule
def within_yardstick(name, got, truth, yard, where):
    """asserts max|got - truth| <= 8 max(max|yard - truth|, 2^-24 max|truth|) and prints the figures: `yard` is the
    same computation in float32 on the CPU, `truth` in float64 (the reasoning: tests/test_gpu_allpass.py)"""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    scale = np.abs(truth).max()
    err, yerr = np.abs(got - truth).max(), np.abs(np.asarray(yard, dtype=np.float64) - truth).max()
    allowed = 8 * max(yerr, 2.0 ** -24 * scale)
    print("{} {}: kernel {:.3g} yardstick {:.3g} (relative to max {:.3g}: {:.3g} / {:.3g})"
          .format(where, name, err, yerr, scale, err / max(scale, 1e-300), yerr / max(scale, 1e-300)))
    assert np.isfinite(got).all(), "{} {}: not finite".format(where, name)
    assert err <= allowed, "{} {}: error {:.3g} above 8 x yardstick {:.3g}".format(where, name, err, allowed)
