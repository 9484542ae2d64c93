"""The float64 restatement of MLPG and of its adjoint that the tests of the differentiable MLPG compare against
(helper, no tests): dense windows W_w, the precisions tau_w with the edge rule, the precision matrix P, the trajectory
c = P^-1 sum_w W_w^T (tau_w o mu_w) and the adjoint

    z = P^-1 g,   dL/dmu_w = tau_w o (W_w z)

per utterance, plus the case tables of the GPU sweep.  The solves are numpy's dense LU followed by two steps of
iterative refinement with the residual in extended precision, so that the reference's own error stays near one
rounding of the solution whatever the conditioning of P (the log-uniform variances reach 1e6)."""
import functools

import numpy as np

BIG_VAR = 1e11                      # the delta variances of the first and last frame (misc/mlpg.py:114-117)

# ---- the case tables of tests/test_gpu_mlpg_adjoint.py -------------------------------------------------------------
# One batch with every length: the last-two-frames rule (0 .. 4), the prefetch block of 8 (7, 8, 9, 16, 17), wave edges
# (63, 64, 65), the forward's change of form (193, 194) and an utterance past the point where the factor repeats (300).
LENGTHS = (65, 0, 1, 300, 2, 3, 4, 7, 194, 8, 9, 16, 17, 63, 64, 193)
DIMS = (1, 2, 15, 16, 17, 60, 64, 65)
VARIANCE_SETS = ("typical", "loguniform")
F64_RMSE, F64_MAX = 1e-10, 1e-9             # the forward's bounds (tests/test_gpu_mlpg.py), times max(1, max|ref|)
F32_REL, F32_ELEM = 2e-6, 2e-5              # the dense layers' bounds (tests/lnorm_cases.py)


def variances(kind, dim, seed=0):
    """[3 * dim]: static | delta | delta-delta"""
    if kind == "typical":
        return np.repeat([1.3, 0.05, 0.02], dim)
    assert kind == "loguniform"
    rng = np.random.RandomState(1000 + 7 * dim + seed)
    return 10.0 ** rng.uniform(-3.0, 2.0, size=3 * dim)


def offsets_of(lengths):
    return [0] + [int(o) for o in np.cumsum(lengths)]


# ---- the mathematics -----------------------------------------------------------------------------------------------
def windows(T):
    """dense W_0, W_1 = [-.5 0 .5], W_2 = [1 -2 1], [T, T] each; neighbours outside the utterance are absent"""
    eye = np.eye(T)
    up, down = np.eye(T, k=1), np.eye(T, k=-1)
    return eye, 0.5 * (up - down), up + down - 2.0 * eye


def taus(T, var, dim):
    """tau_w [T, dim] for w = 0, 1, 2: 1 / var_w, with 1 / BIG_VAR in the first and last frame for w = 1, 2"""
    var = np.asarray(var, dtype=np.float64)
    out = []
    for w in range(3):
        tau = np.tile(1.0 / var[w * dim:(w + 1) * dim], (T, 1))
        if w > 0 and T > 0:
            tau[0] = tau[T - 1] = 1.0 / BIG_VAR
        out.append(tau)
    return out


def precision(T, var, dim):
    """P [dim, T, T] = sum_w W_w^T diag(tau_w) W_w"""
    return sum((W.T[None] * tau.T[:, None, :]) @ W for W, tau in zip(windows(T), taus(T, var, dim)))


def solve(P, b):
    """P [D, T, T], b [D, T] -> x [D, T]; see the module docstring"""
    x = np.linalg.solve(P, b[..., None])[..., 0]
    Pl = P.astype(np.longdouble)
    for _ in range(2):
        r = b.astype(np.longdouble) - np.einsum("dij,dj->di", Pl, x.astype(np.longdouble))
        x = (x.astype(np.longdouble) + np.linalg.solve(P, r.astype(np.float64)[..., None])[..., 0]).astype(np.float64)
    return x


def rhs(rows, var, dim):
    """b [T, dim] = sum_w W_w^T (tau_w o mu_w) of one utterance's rows [T, 3 * dim]"""
    T = rows.shape[0]
    return sum(W.T @ (tau * rows[:, w * dim:(w + 1) * dim])
               for w, (W, tau) in enumerate(zip(windows(T), taus(T, var, dim))))


def trajectory(rows, var, dim):
    """[T, 3 * dim] -> [T, dim]"""
    rows = np.asarray(rows, dtype=np.float64)
    T = rows.shape[0]
    if T == 0:
        return np.zeros((0, dim))
    return solve(precision(T, var, dim), rhs(rows, var, dim).T).T


def adjoint(g, var, dim):
    """dL/dc [T, dim] -> dL/dmu [T, 3 * dim]"""
    g = np.asarray(g, dtype=np.float64)
    T = g.shape[0]
    if T == 0:
        return np.zeros((0, 3 * dim))
    z = solve(precision(T, var, dim), g.T).T
    return np.concatenate([tau * (W @ z) for W, tau in zip(windows(T), taus(T, var, dim))], axis=1)


def per_utterance(fn, x, var, dim, offsets):
    """fn (trajectory or adjoint) on every utterance of the stacked rows x"""
    return np.concatenate([fn(x[a:b], var, dim) for a, b in zip(offsets[:-1], offsets[1:])], axis=0)


def upper_band(P):
    """[T, T] -> the [3, T] upper band scipy.linalg.solveh_banded takes"""
    T = P.shape[0]
    ab = np.zeros((3, T))
    for k in range(3):
        ab[2 - k, k:] = np.diagonal(P, k)
    return ab


# ---- shared references ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_case(dim, kind, f32):
    """(offsets, var, gout, ref) of the shape sweep: gout [Ttot, dim] in the case's dtype, ref the float64 adjoint of
    exactly those values.  Computed once per case; treat as read-only."""
    offsets = offsets_of(LENGTHS)
    var = variances(kind, dim)
    rng = np.random.RandomState(17 * dim + (1 if kind == "typical" else 2))
    gout = rng.standard_normal((offsets[-1], dim))
    if f32:
        gout = gout.astype(np.float32)
    ref = per_utterance(adjoint, gout.astype(np.float64), var, dim, offsets)
    for a in (gout, ref, var):
        a.setflags(write=False)
    return offsets, var, gout, ref


def check_f64(got, ref, what=""):
    scale = max(1.0, np.abs(ref).max()) if ref.size else 1.0
    diff = got - ref
    rmse = np.sqrt(np.mean(diff ** 2)) if diff.size else 0.0
    err = np.abs(diff).max() if diff.size else 0.0
    print("f64 {}: rmse {:.3e} (bound {:.1e}), max {:.3e} (bound {:.1e}), scale {:.3e}".format(
        what, rmse, F64_RMSE * scale, err, F64_MAX * scale, scale))
    assert rmse <= F64_RMSE * scale and err <= F64_MAX * scale, (what, rmse, err, scale)


def check_f32(got, ref, what=""):
    scale = max(1.0, np.abs(ref).max()) if ref.size else 1.0
    diff = got.astype(np.float64) - ref
    rel = np.linalg.norm(diff) / max(np.linalg.norm(ref), 1e-300) if diff.size else 0.0
    err = np.abs(diff).max() if diff.size else 0.0
    print("f32 {}: rel 2-norm {:.3e} (bound {:.1e}), max {:.3e} (bound {:.1e})".format(
        what, rel, F32_REL, err, F32_ELEM * scale))
    assert rel <= F32_REL and err <= F32_ELEM * scale, (what, rel, err, scale)
