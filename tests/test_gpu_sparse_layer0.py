"""The fixed costs of layer 0's sparse kernels: the forward's slab fill by 16-byte loads against
the dword fill and fp64, and the weight gradient's merge of the heavy shares over tile counts, pitches, whole and
partial slabs.  Neither changes a summation order, so wherever two ways lead to the same sums the check is bit
equality; the fp64 bounds are those of tests/test_gpu_sparse_rows.py and tests/test_gpu_sparse_wgrad.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 256                                   # rows of a tile


def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-30)


def _pad4(n):
    return (n + 3) // 4 * 4


def _matrix(M, K, seed, density=0.1, heavy_cols=0):
    """float32 [M, K + 3] (so ldx > K), pad columns 7.0; `density` of uniform (0, 1] values, the first `heavy_cols`
    columns (as many as K has) at 0.9; where M allows it an all-zero row, a dense row and a row of -0.0 / NaN / a
    denormal in turn"""
    rng = np.random.default_rng(seed)
    x = np.full((M, K + 3), 7.0, dtype=np.float32)
    dens = np.full(K, density)
    dens[:heavy_cols] = 0.9
    vals = (1.0 - rng.random((M, K))).astype(np.float32)
    x[:, :K] = np.where(rng.random((M, K)) < dens[None, :], vals, np.float32(0.0))
    special = x[M - 1]
    special[0:K:3] = np.float32(-0.0)
    special[1:K:3] = np.float32("nan")
    special[2:K:3] = np.float32(1e-40)
    if M >= 3:
        x[0, :K] = 0.0
        x[1, :K] = 0.5 + np.arange(K, dtype=np.float32)
    return x


# ---------------------------------------------------------------------------------------------- forward: slab fill
@pytest.mark.parametrize("K", [1, 425, 428, 512])
@pytest.mark.parametrize("N", [1, 65, 512])
def test_forward_slab_fill(gpu, N, K):
    """K % 4 == 0 with 16-byte rows of w takes the 16-byte fill, anything else the dword fill; the same w one float
    further on is misaligned and must give the same bits"""
    from idiaptts_amd import ops
    M = 130
    g = torch.Generator().manual_seed(N * 31 + K)
    x = torch.from_numpy(_matrix(M, K, seed=N + K, density=0.07)[:, :K].copy())
    # the bounds are on every output and were set for inputs in (0, 1] (tests/test_gpu_sparse_rows.py): no NaN row,
    # and the dense row drawn from that range
    x[M - 1] = 0.0
    x[1] = 1.0 - torch.rand(K, generator=g)
    w = (torch.rand(N, K, generator=g) - 0.5) * (2.0 / K ** 0.5)
    b = torch.rand(N, generator=g) - 0.5
    ref = torch.tanh(torch.nn.functional.linear(x.double(), w.double(), b.double())).float()
    xg, bg = x.to(gpu), b.to(gpu)
    store = torch.empty(N * K + 4, device=gpu)
    w_al = store[:N * K].view(N, K)
    w_mis = store[1:N * K + 1].view(N, K)
    assert w_al.data_ptr() % 16 == 0 and w_mis.data_ptr() % 16 == 4
    lists = ops.sparse_rows_build(xg, want_record=False)
    w_al.copy_(w)
    y_al = ops.linear_fwd_sparse(lists, xg, w_al, bg, 1).clone()
    w_mis.copy_(w)
    y_mis = ops.linear_fwd_sparse(lists, xg, w_mis, bg, 1)
    assert torch.equal(y_al, y_mis)
    print("N %d K %d: rel %.2e max %.2e" % (N, K, _rel(y_al.cpu(), ref), (y_al.cpu() - ref).abs().max().item()))
    assert _rel(y_al.cpu(), ref) < 2e-6
    assert (y_al.cpu() - ref).abs().max().item() < 2e-5


# ------------------------------------------------------------------- weight gradient: tile buffers and share merge
BOUND = 3e-6


def _dz(M, N, lddz, seed, gpu):
    """[M, N] view of a [M, lddz] buffer whose pad columns hold 3.0; uniform in (-0.25, 0.75), see
    tests/test_gpu_sparse_wgrad.py::_dz"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((M, lddz), 3.0)
    buf[:, :N] = torch.rand(M, N, generator=g) - 0.25
    return buf.to(gpu)[:, :N]


def _wgrad_input(M, K, seed):
    x = _matrix(M, K, seed=seed, density=0.07, heavy_cols=20)[:, :K].copy()
    x[M - 1] = 0.0                                        # no NaN
    return x


def _dw(ops, dz, xg, plan, K):
    cols = ops.sparse_cols_build(xg, plan, K=K)
    before = ops.sparse_wgrad_counts()
    dw, db = ops.linear_bwd_weight_sparse(dz, xg, cols, plan, K=K)
    after = ops.sparse_wgrad_counts()
    assert after.dw_sparse == before.dw_sparse + 1 and after.dw_dense == before.dw_dense
    return dw, db


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_wgrad_tiles_and_pitches(gpu, M, N, pad):
    from idiaptts_amd import ops
    K = 425
    x = _wgrad_input(M, K, seed=M + N)
    xg = torch.from_numpy(x).to(gpu)
    plan = ops.sparse_cols_plan(xg, K=K)
    dz = _dz(M, N, N + pad, M * 13 + N, gpu)
    dw, db = _dw(ops, dz, xg, plan, K)
    dz64 = dz.cpu().double()
    ref_w, ref_b = dz64.t() @ torch.from_numpy(x).double(), dz64.sum(dim=0)
    figs = (_rel(dw.cpu().double(), ref_w), _rel(db.cpu().double(), ref_b))
    print("M %d N %d lddz %d: dw %.2e db %.2e" % (M, N, N + pad, figs[0], figs[1]))
    assert max(figs) < BOUND, figs
    dw_again, db_again = _dw(ops, dz, xg, plan, K)
    assert torch.equal(dw, dw_again) and torch.equal(db, db_again)
    with ops.deferred_reductions():
        dw_def, db_def = _dw(ops, dz, xg, plan, K)
    assert torch.equal(dw, dw_def) and torch.equal(db, db_def)
    # the other pitch holds the same dz: the same bits
    other = _dz(M, N, N + 4 - pad, M * 13 + N, gpu)
    assert torch.equal(other, dz)
    dw_o, db_o = _dw(ops, other, xg, plan, K)
    assert torch.equal(dw, dw_o) and torch.equal(db, db_o)


def test_wgrad_three_tiles_per_workgroup(gpu):
    """one slab and 2 x 256 x CUs + 1 rows: every workgroup walks three tiles, so both tile buffers are used again"""
    from idiaptts_amd import ops
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    M, N, K = 2 * T * cus + 1, 64, 65
    rng = np.random.default_rng(17)
    dens = np.full(K, 0.07)
    dens[:3] = 0.9
    x = np.where(rng.random((M, K)) < dens[None, :], 1.0 - rng.random((M, K)), 0.0).astype(np.float32)
    xg = torch.from_numpy(x).to(gpu)
    plan = ops.sparse_cols_plan(xg, K=K)
    assert len(plan.heavy) == 3
    dz = _dz(M, N, N, 23, gpu)
    dw, db = _dw(ops, dz, xg, plan, K)
    dz64 = dz.cpu().double()
    ref_w, ref_b = dz64.t() @ torch.from_numpy(x).double(), dz64.sum(dim=0)
    figs = (_rel(dw.cpu().double(), ref_w), _rel(db.cpu().double(), ref_b))
    print("M %d: dw %.2e db %.2e" % (M, figs[0], figs[1]))
    assert max(figs) < BOUND, figs
    dw_again, db_again = _dw(ops, dz, xg, plan, K)
    assert torch.equal(dw, dw_again) and torch.equal(db, db_again)


@pytest.mark.parametrize("M", [257, 3 * T + 5])
def test_wgrad_partial_slab_equals_the_zero_padded_one(gpu, M):
    """N = 65: the second slab holds one column and its loads stop at N; the same dz zero-padded to 128 columns has
    two whole slabs.  The same sums in the same order: the first 65 rows of dw are bit-equal."""
    from idiaptts_amd import ops
    N, K = 65, 425
    x = _wgrad_input(M, K, seed=M)
    xg = torch.from_numpy(x).to(gpu)
    plan = ops.sparse_cols_plan(xg, K=K)
    dz = _dz(M, N, 68, 31, gpu)
    wide = torch.zeros((M, 128), device=gpu)
    wide[:, :N] = dz
    dw, db = _dw(ops, dz, xg, plan, K)
    dw_w, db_w = _dw(ops, wide, xg, plan, K)
    assert torch.equal(dw, dw_w[:N]) and torch.equal(db, db_w[:N])
    assert float(dw_w[N:].abs().sum()) == 0.0 and float(db_w[N:].abs().sum()) == 0.0
    dz64 = dz.cpu().double()
    ref_w, ref_b = dz64.t() @ torch.from_numpy(x).double(), dz64.sum(dim=0)
    figs = (_rel(dw.cpu().double(), ref_w), _rel(db.cpu().double(), ref_b))
    assert max(figs) < BOUND, figs


@pytest.mark.parametrize("which", ["light", "heavy"])
def test_wgrad_nan_stays_in_its_column(gpu, which):
    from idiaptts_amd import ops
    M, N, K = 2 * T + 1, 128, 425
    xg = torch.from_numpy(_wgrad_input(M, K, seed=21)).to(gpu)
    plan = ops.sparse_cols_plan(xg, K=K)
    col = plan.heavy[3] if which == "heavy" else [o for o in plan.owners if len(o) > 1][-1][1]
    xg[T + 2, col] = float("nan")
    dw, db = _dw(ops, _dz(M, N, N, 4, gpu), xg, plan, K)
    assert bool(torch.isnan(dw[:, col]).all())
    assert torch.isnan(dw).any(dim=0).sum().item() == 1 and not bool(torch.isnan(db).any())


# ------------------------------------------------------------------------------------------------------- the model
def _three_steps(gpu, batches):
    from idiaptts_amd.native_ff import FlatFFModel
    model = FlatFFModel((425, 512, 512, 187), ("tanh", "tanh", None), device=gpu, seed=4, sparse_input=True,
                        sparse_wgrad=True)
    losses = []
    for x, y, n in batches:
        valid = torch.ones(x.shape[0], dtype=torch.uint8, device=gpu)
        losses.append(model.train_step(x, y, valid, n))
    return model, torch.stack(losses)




def test_model_steps_count_and_repeat(gpu):
    """three steps with both sparse paths: every counter moves by three, and a second model fed the same batches
    ends with the same bits (no order in the step depends on timing)"""
    from idiaptts_amd import ops
    from idiaptts_amd.bench_support import make_ff_batch
    batches = []
    for step in range(3):
        x, y, lengths = make_ff_batch(3, seed=100 + step)
        batches.append((x.to(gpu), y.to(gpu), float(lengths.sum())))

    def moved():
        r, c = ops.sparse_path_counts(), ops.sparse_wgrad_counts()
        return (r.builds, r.fwd_sparse, c.col_builds, c.dw_sparse)

    before = moved()
    model, losses = _three_steps(gpu, batches)
    assert tuple(b - a for a, b in zip(before, moved())) == (3, 3, 3, 3)
    again, losses_again = _three_steps(gpu, batches)
    assert torch.equal(losses, losses_again)
    assert torch.equal(model.params, again.params)
    assert torch.equal(model.exp_avg, again.exp_avg) and torch.equal(model.exp_avg_sq, again.exp_avg_sq)
