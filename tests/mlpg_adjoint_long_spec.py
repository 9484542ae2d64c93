"""The MLPG adjoint for utterances too long for the dense restatement (helper, no tests): the same mathematics as
tests/mlpg_adjoint_spec.py -- z = P^-1 g, dL/dmu_w = tau_w o (W_w z) -- with P kept as the [3, T] upper band that
`mlpg_adjoint_spec.upper_band` lays out (built here diagonal by diagonal from the windows and precisions, never as a
dense matrix: the dense P of a 2 000-frame utterance is 32 MB per dimension and its solve cubic), solved by
scipy.linalg.solveh_banded plus one step of iterative refinement with the residual in np.longdouble.
tests/test_mlpg_adjoint_long_spec.py holds the band to upper_band(precision(..)) and the result to
mlpg_adjoint_spec.adjoint; the case tables of tests/test_gpu_mlpg_adjoint_stream.py are below."""
import functools

import numpy as np

import mlpg_adjoint_spec as spec

# window coefficients on rows t-1, t, t+1 (mlpg_adjoint_spec.windows)
_COEFFS = ((0.0, 1.0, 0.0), (-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))

# ---- the case tables of tests/test_gpu_mlpg_adjoint_stream.py -------------------------------------------------------
# The stream form's geometry: 16-frame chunks (208, 224, 256), the one-frame remainder that borrows a frame (209, 225,
# 241, 257, 273, 513, 529, 1041), 2 and 4 chunks per workgroup, 16 scan segments (241 .. 273), blocks of 8 aggregates
# (1041, 2050), and utterances of one chunk or less among them.
LENGTHS = (194, 0, 207, 208, 209, 1, 210, 224, 225, 2, 241, 256, 257, 273, 3, 513, 529, 17, 1041, 2050)
DIMS = (1, 2, 63, 64, 65, 130)
PLACED_LENGTHS = (209, 257, 1, 529)


def band(T, var, dim):
    """[dim, 3, T]: the upper band of P = sum_w W_w^T diag(tau_w) W_w of every dimension, ab[d, 2 - k, j] = P_d[j - k, j]"""
    ab = np.zeros((dim, 3, T))
    t = np.arange(T)
    for coeff, tau in zip(_COEFFS, spec.taus(T, var, dim)):
        for m1 in (-1, 0, 1):
            for m2 in range(m1, 2):
                c = coeff[m1 + 1] * coeff[m2 + 1]
                if c == 0.0:
                    continue
                rows = t[(t + m1 >= 0) & (t + m2 < T)]          # window rows that have both columns
                ab[:, 2 - (m2 - m1), rows + m2] += c * tau[rows].T
    return ab


def band_matvec(ab, x):
    """P x for P given by its upper band ab [3, T] (symmetric) and x [T] or [T, n], in the dtype of the operands"""
    ab = ab.reshape(ab.shape + (1,) * (x.ndim - 1))
    y = ab[2] * x
    for k in (1, 2):
        if x.shape[0] > k:
            y[:-k] += ab[2 - k, k:] * x[k:]
            y[k:] += ab[2 - k, k:] * x[:-k]
    return y


def solve_banded(ab, b):
    """ab [3, T], b [T] or [T, n] -> P^-1 b: Cholesky on the band, then one refinement step with the residual in
    extended precision"""
    from scipy.linalg import solveh_banded
    T = b.shape[0]
    cut = ab[max(0, 3 - T):]                     # (a band no wider than the matrix)
    x = solveh_banded(cut, b)
    r = b.astype(np.longdouble) - band_matvec(ab.astype(np.longdouble), x.astype(np.longdouble))
    return (x.astype(np.longdouble) + solveh_banded(cut, r.astype(np.float64))).astype(np.float64)


def adjoint(g, var, dim):
    """dL/dc [T, dim] -> dL/dmu [T, 3 * dim], as mlpg_adjoint_spec.adjoint"""
    g = np.asarray(g, dtype=np.float64)
    T = g.shape[0]
    if T == 0:
        return np.zeros((0, 3 * dim))
    ab = band(T, var, dim)
    if (ab == ab[:1]).all():                     # one matrix for every dimension: one factorisation
        z = solve_banded(ab[0], g)
    else:
        z = np.stack([solve_banded(ab[d], g[:, d]) for d in range(dim)], axis=1)
    zp = np.zeros((T + 2, dim))                  # z outside the utterance counts as 0
    zp[1:-1] = z
    tau0, tau1, tau2 = spec.taus(T, var, dim)
    return np.concatenate([tau0 * z, tau1 * (0.5 * (zp[2:] - zp[:-2])), tau2 * (zp[:-2] - 2.0 * z + zp[2:])], axis=1)


@functools.lru_cache(maxsize=None)
def stream_case(dim, kind, lengths=LENGTHS):
    """(offsets, var, gout, ref): gout [Ttot, dim] float64 holding values that float32 represents exactly, so that its
    float32 copy is the same gradient and both input types share ref, the float64 adjoint of exactly those values.
    Computed once per case; treat as read-only."""
    offsets = spec.offsets_of(lengths)
    var = spec.variances(kind, dim)
    rng = np.random.RandomState(31 * dim + (1 if kind == "typical" else 2) + len(lengths))
    gout = rng.standard_normal((offsets[-1], dim)).astype(np.float32).astype(np.float64)
    ref = spec.per_utterance(adjoint, gout, var, dim, offsets)
    for a in (gout, ref, var):
        a.setflags(write=False)
    return offsets, var, gout, ref


def composed_gradient(grad, streams, offsets, width):
    """The gradient MlpgFunction's backward returns, composed from the forward solve and torch window ops (DESIGN.md
    section 25 (c)) -- nothing of the adjoint's kernels: ops.mlpg_generation on rows (g var_0, 0, 0), whose right-hand
    side is g itself, gives z = P^-1 g; then the three windows with the edge precisions.  grad [N, sum of dims] on the
    GPU, streams [(col0, dim, variances [3 * dim] float64 on the GPU)]; returns [N, width] float64."""
    import torch
    from idiaptts_amd import ops
    N, dev = grad.shape[0], grad.device
    grad = grad.double()
    first = torch.zeros(N, 1, dtype=torch.float64, device=dev)
    last = torch.zeros(N, 1, dtype=torch.float64, device=dev)
    starts = [a for a, b in zip(offsets[:-1], offsets[1:]) if b > a]
    ends = [b - 1 for a, b in zip(offsets[:-1], offsets[1:]) if b > a]
    first[starts] = 1.0
    last[ends] = 1.0
    edge = torch.clamp(first + last, max=1.0)
    out = torch.zeros(N, width, dtype=torch.float64, device=dev)
    zero_row = torch.zeros(1, 1, dtype=torch.float64, device=dev)
    o0 = 0
    for col0, dim, var in streams:
        rows = torch.zeros(N, 3 * dim, dtype=torch.float64, device=dev)
        rows[:, :dim] = grad[:, o0:o0 + dim] * var[:dim]
        z = ops.mlpg_generation(rows, var, dim, offsets)
        zp = torch.cat((zero_row.expand(1, dim), z[:-1]), dim=0) * (1.0 - first)
        zn = torch.cat((z[1:], zero_row.expand(1, dim)), dim=0) * (1.0 - last)
        tau0, tau1, tau2 = (1.0 / var[w * dim:(w + 1) * dim] for w in range(3))
        tau1 = (1.0 - edge) * tau1 + edge / spec.BIG_VAR
        tau2 = (1.0 - edge) * tau2 + edge / spec.BIG_VAR
        out[:, col0:col0 + dim] = tau0 * z
        out[:, col0 + dim:col0 + 2 * dim] = tau1 * (0.5 * (zn - zp))
        out[:, col0 + 2 * dim:col0 + 3 * dim] = tau2 * (zp - 2.0 * z + zn)
        o0 += dim
    return out
