"""Layer 0's weight gradient from column lists of its sparse input (csrc/sparse_wgrad.hip): dw = dz^T x and db against
fp64 and against the dense entry over edge shapes and inputs, a plan from another matrix, NaN, bit-identical re-runs,
the dense fallback, and the flat model with the path on.  The bound on dw / db is that of
tests/test_gpu_nn.py::test_linear_bwd_weight: the sparse path is one more summation order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 256                                   # rows of a tile of the column build
BOUND = 3e-6


def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-30)


def _pad4(n):
    return (n + 3) // 4 * 4


def _skewed(M, K, rng):
    """40 columns at 0.9 (as many as K has), 100 always-zero columns, the rest at 0.07, one all-dense row"""
    dens = np.full(K, 0.07)
    perm = rng.permutation(K)
    dens[perm[:min(40, K)]] = 0.9
    dens[perm[40:140]] = 0.0
    x = np.where(rng.random((M, K)) < dens[None, :], 1.0 - rng.random((M, K)), 0.0)
    x[M // 2, :] = 0.5 + rng.random(K)
    return x.astype(np.float32)


def _input(kind, M, K, seed):
    """float32 [M, pitch]: the first K columns hold the matrix, the pad columns behind them 7.0 (a list or a strip
    that named one would show)"""
    rng = np.random.default_rng(seed)
    pitch = _pad4(K) + 4
    x = np.full((M, pitch), 7.0, dtype=np.float32)
    if kind == "skewed":
        x[:, :K] = _skewed(M, K, rng)
    else:
        vals = (1.0 - rng.random((M, K))).astype(np.float32)
        x[:, :K] = np.where(rng.random((M, K)) < kind, vals, np.float32(0.0))
    return x


def _dz(M, N, seed, gpu):
    """[M, N] view of a [M, pad4(N)] buffer whose pad columns hold 3.0.  The values are uniform in (-0.25, 0.75): both
    signs, but a mean away from zero.  The shapes go down to a single output (N = K = 1), whose relative error is
    that of one sum: an fp32 chain of n terms is off by about sqrt(n) * 6e-8 * sum|t|, so against |sum t| the bound
    of 3e-6 can only be asked where sum|t| / |sum t| stays near 1 (here 1.25); with a zero-mean dz that ratio is
    sqrt(n) and larger for one output, whatever the order of the sum."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((M, _pad4(N)), 3.0)
    buf[:, :N] = torch.rand(M, N, generator=g) - 0.25
    return buf.to(gpu)[:, :N]


def _sparse_dw(ops, dz, xg, K, plan=None, **kw):
    plan = ops.sparse_cols_plan(xg, K=K) if plan is None else plan
    cols = ops.sparse_cols_build(xg, plan, K=K)
    return ops.linear_bwd_weight_sparse(dz, xg, cols, plan, K=K, **kw)


SHAPES = [(M, N, K) for M in (1, 5, T - 1, T, T + 1, 2 * T + 1, 1030) for N in (1, 63, 64, 65, 187)
          for K in (1, 3, 425, 512)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_sparse_wgrad_shapes_and_inputs(gpu, M, N, K):
    from idiaptts_amd import ops
    dz = _dz(M, N, M * 13 + N, gpu)
    dz64 = dz.cpu().double()
    for kind in (0.0, 0.07, 1.0, "skewed"):
        x = _input(kind, M, K, seed=M + 3 * N + 7 * K)
        xg = torch.from_numpy(x).to(gpu)
        x64 = torch.from_numpy(x[:, :K]).double()
        ref_w, ref_b = dz64.t() @ x64, dz64.sum(dim=0)
        lddw = _pad4(K)
        before = ops.sparse_wgrad_counts()
        dw = torch.full((N, lddw), 5.0, device=gpu)
        dw, db = _sparse_dw(ops, dz, xg, K, dw=dw)
        after = ops.sparse_wgrad_counts()
        assert after.col_builds == before.col_builds + 1 and after.dw_sparse == before.dw_sparse + 1
        assert after.dw_dense == before.dw_dense
        dense_w, dense_b = ops.linear_bwd_weight(dz, xg[:, :K])
        figs = (_rel(dw[:, :K].cpu().double(), ref_w), _rel(db.cpu().double(), ref_b),
                _rel(dw[:, :K].cpu(), dense_w.cpu()), _rel(db.cpu(), dense_b.cpu()))
        print("M %d N %d K %d %s: dw %.2e db %.2e against fp64, dw %.2e db %.2e against dense" % ((M, N, K, kind) + figs))
        assert max(figs) < BOUND, (kind, figs)
        assert float(dw[:, K:].abs().sum()) == 0.0                              # pad columns of dw
        # accumulate: onto the result itself gives exactly twice
        dw2, db2 = _sparse_dw(ops, dz, xg, K, dw=dw.clone(), db=db.clone(), accumulate=True)
        assert torch.equal(dw2, 2 * dw) and torch.equal(db2, 2 * db)
        dw3, none = _sparse_dw(ops, dz, xg, K, want_bias=False)
        assert none is None and torch.equal(dw3, dw[:, :K])


def _two_block_matrices(M, K, seed):
    """A has its dense columns at 0..39, B at 100..139; elsewhere 5 %"""
    rng = np.random.default_rng(seed)
    out = []
    for first in (0, 100):
        dens = np.full(K, 0.05)
        dens[first:first + 40] = 0.95
        out.append(np.where(rng.random((M, K)) < dens[None, :], 1.0 - rng.random((M, K)), 0.0).astype(np.float32))
    return out


def test_plan_from_another_matrix(gpu):
    """the plan is a hint: made from A, used on B whose dense columns are different ones"""
    from idiaptts_amd import ops
    M, N, K = 2 * T + 1, 65, 425
    a, b = _two_block_matrices(M, K, 5)
    ag, bg = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    plan = ops.sparse_cols_plan(ag)
    assert len(plan.heavy) == 31 and set(plan.heavy) <= set(range(40))
    dz = _dz(M, N, 3, gpu)
    dw, db = _sparse_dw(ops, dz, bg, K, plan=plan)
    ref_w, ref_b = dz.cpu().double().t() @ torch.from_numpy(b).double(), dz.cpu().double().sum(dim=0)
    dense_w, dense_b = ops.linear_bwd_weight(dz, bg)
    figs = (_rel(dw.cpu().double(), ref_w), _rel(db.cpu().double(), ref_b), _rel(dw.cpu(), dense_w.cpu()),
            _rel(db.cpu(), dense_b.cpu()))
    print("stale plan: %.2e %.2e %.2e %.2e" % figs)
    assert max(figs) < BOUND, figs


@pytest.mark.parametrize("which", ["light", "heavy"])
def test_nan_marks_its_column_alone(gpu, which):
    from idiaptts_amd import ops
    M, N, K = T + 1, 65, 425
    x = _input("skewed", M, K, seed=21)[:, :K].copy()
    xg = torch.from_numpy(x).to(gpu)
    plan = ops.sparse_cols_plan(xg)
    col = plan.heavy[3] if which == "heavy" else [o for o in plan.owners if len(o) > 1][-1][1]
    xg[T - 2, col] = float("nan")
    dw, db = _sparse_dw(ops, _dz(M, N, 4, gpu), xg, K, plan=plan)
    nan_cols = torch.isnan(dw).any(dim=0).cpu()
    assert bool(torch.isnan(dw[:, col]).all())
    assert nan_cols.sum().item() == 1 and not bool(torch.isnan(db).any())


def test_reruns_and_deferred_reductions_are_bit_identical(gpu):
    from idiaptts_amd import ops
    M, N, K = 1030, 187, 425
    xg = torch.from_numpy(_input("skewed", M, K, seed=8)).to(gpu)
    dz = _dz(M, N, 6, gpu)
    plan = ops.sparse_cols_plan(xg, K=K)
    dw, db = _sparse_dw(ops, dz, xg, K, plan=plan)
    dw_again, db_again = _sparse_dw(ops, dz, xg, K, plan=plan)
    assert torch.equal(dw, dw_again) and torch.equal(db, db_again)
    with ops.deferred_reductions():
        dw_def, db_def = _sparse_dw(ops, dz, xg, K, plan=plan)
    assert torch.equal(dw, dw_def) and torch.equal(db, db_def)


def test_wide_input_runs_the_dense_entry(gpu):
    """K > 512 has no plan: the entry point runs the dense product, decided on the host, and says so"""
    from idiaptts_amd import ops
    M, N, K = 70, 33, 516
    xg = torch.from_numpy(_input(0.07, M, K, seed=1)[:, :K].copy()).to(gpu)
    dz = _dz(M, N, 2, gpu)
    with pytest.raises(ValueError):
        ops.sparse_cols_plan(xg)
    before = ops.sparse_wgrad_counts()
    dw, db = ops.linear_bwd_weight_sparse(dz, xg, None, None)
    after = ops.sparse_wgrad_counts()
    assert after.dw_dense == before.dw_dense + 1 and after.dw_sparse == before.dw_sparse
    assert after.col_builds == before.col_builds
    dense_w, dense_b = ops.linear_bwd_weight(dz, xg)
    assert torch.equal(dw, dense_w) and torch.equal(db, dense_b)


def _three_steps(gpu, batches, **kw):
    from idiaptts_amd.native_ff import FlatFFModel
    model = FlatFFModel((425, 512, 512, 187), ("tanh", "tanh", None), device=gpu, seed=4, **kw)
    losses = []
    for x, y, n in batches:
        valid = torch.ones(x.shape[0], dtype=torch.uint8, device=gpu)
        losses.append(model.train_step(x, y, valid, n).item())
    return model, losses


def test_model_sparse_wgrad_matches_dense(gpu):
    """the numbers of _assert_same_training in tests/test_gpu_sparse_rows.py: loss 1e-5 relative, parameters 2e-6"""
    from idiaptts_amd import ops
    from idiaptts_amd.bench_support import make_ff_batch
    batches = []
    for step in range(3):
        x, y, lengths = make_ff_batch(3, seed=100 + step)
        batches.append((x.to(gpu), y.to(gpu), float(lengths.sum())))
    c0 = ops.sparse_wgrad_counts()
    dense, dense_losses = _three_steps(gpu, batches, sparse_input=False)
    assert ops.sparse_wgrad_counts() == c0                      # forced off: follows sparse_input
    model, losses = _three_steps(gpu, batches, sparse_input=True)
    c1 = ops.sparse_wgrad_counts()
    assert c1.col_builds == c0.col_builds + 3 and c1.dw_sparse == c0.dw_sparse + 3 and c1.dw_dense == c0.dw_dense
    for a, b in zip(losses, dense_losses):
        assert abs(a - b) < 1e-5 * abs(b)
    for i in range(len(model.layout)):
        assert (model.weight(i) - dense.weight(i)).abs().max().item() < 2e-6
        assert (model.bias(i) - dense.bias(i)).abs().max().item() < 2e-6
    only_w, losses_w = _three_steps(gpu, batches, sparse_input=False, sparse_wgrad=True)
    c2 = ops.sparse_wgrad_counts()
    assert c2.dw_sparse == c1.dw_sparse + 3
    for i in range(len(model.layout)):
        assert (only_w.weight(i) - dense.weight(i)).abs().max().item() < 2e-6
