"""Layer 0 on a sparse input (csrc/sparse_rows.hip): the row lists against numpy, the forward product that walks
them against fp64 and against the dense product, and the flat model with the path forced on, forced off and chosen
from the first batch.  Tolerances are those of tests/test_gpu_nn.py: the sparse path is one more summation order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-30)


def _sparse_matrix(M, K, density, seed, pitch=None, pad_value=7.0):
    """float32 [M, pitch] whose first K columns are zero except a `density` share of uniform (0, 1] values; the pad
    columns hold `pad_value` (a list that named one would show)."""
    rng = np.random.default_rng(seed)
    pitch = K if pitch is None else pitch
    x = np.full((M, pitch), pad_value, dtype=np.float32)
    vals = (1.0 - rng.random((M, K))).astype(np.float32)
    x[:, :K] = np.where(rng.random((M, K)) < density, vals, np.float32(0.0))
    return x


def _numpy_lists(x, K):
    """counts [M], and (row, position in the row's list, k) of every non-zero: np.nonzero walks row-major, i.e.
    ascending k inside a row.  -0.0 != 0 is False, NaN != 0 and a denormal != 0 are True."""
    nz = x[:, :K] != 0
    counts = nz.sum(axis=1).astype(np.int64)
    rows, cols = np.nonzero(nz)
    starts = np.concatenate([[0], np.cumsum(counts)])[:-1]
    pos = np.arange(rows.size) - starts[rows]
    return counts, rows, pos, cols


# the build gives one wave a row and a workgroup four; its grid stops at 8192 workgroups, so 32768 rows is where a
# wave's share goes from one row to two
@pytest.mark.parametrize("K", [1, 3, 425])
@pytest.mark.parametrize("M", [1, 3, 5, 32767, 32769])
def test_row_lists_equal_numpy(gpu, M, K):
    from idiaptts_amd import ops
    pitch = (K + 3) // 4 * 4 if K == 425 else K + 3
    x = _sparse_matrix(M, K, 0.1, seed=M * 7 + K, pitch=pitch)
    special = x[M - 1]                      # a row of -0.0, NaN and a denormal in turn
    special[0:K:3] = np.float32(-0.0)
    special[1:K:3] = np.float32("nan")
    special[2:K:3] = np.float32(1e-40)
    if M >= 3:
        x[0, :K] = 0.0                      # an all-zero row
        x[1, :K] = 0.5 + np.arange(K, dtype=np.float32)   # an all-non-zero row: K entries, nothing capped
    before = ops.sparse_path_counts()
    lists = ops.sparse_rows_build(torch.from_numpy(x).to(gpu), K=K)
    assert ops.sparse_path_counts().builds == before.builds + 1
    counts, rows, pos, cols = _numpy_lists(x, K)
    got_counts = lists.counts().cpu().numpy()
    assert np.array_equal(got_counts, counts)
    ent = lists.entries().cpu().numpy()
    assert lists.pitch >= K
    assert np.array_equal(ent[rows, pos, 0], cols)
    assert np.array_equal(ent[rows, pos, 1], x[:, :K].view(np.int32)[rows, cols])
    assert lists.record() == (int(counts.sum()), int(counts.max()))
    if M >= 3:
        assert counts[0] == 0 and counts[1] == K
    # -0.0 dropped, NaN and the denormal kept
    assert counts[M - 1] == len(range(1, K, 3)) + len(range(2, K, 3))


FWD_SHAPES = [(1, 1, 1), (5, 7, 3), (130, 187, 425), (257, 512, 425), (333, 67, 409)]


@pytest.fixture(scope="module")
def fwd_cases():
    """inputs and the fp64 pre-activation of every (shape, density), computed once"""
    cases = {}
    for (M, N, K) in FWD_SHAPES:
        for density in (0.0, 0.07, 1.0):
            g = torch.Generator().manual_seed(M * 31 + N)
            x = torch.from_numpy(_sparse_matrix(M, K, density, seed=M + N + int(100 * density)))
            w = (torch.rand(N, K, generator=g) - 0.5) * (2.0 / K ** 0.5)
            b = torch.rand(N, generator=g) - 0.5
            z = torch.nn.functional.linear(x.double(), w.double(), b.double())
            cases[(M, N, K, density)] = (x, w, b, z)
    return cases


@pytest.mark.parametrize("density", [0.0, 0.07, 1.0])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
def test_linear_fwd_sparse(gpu, fwd_cases, M, N, K, act, density):
    from idiaptts_amd import ops
    x, w, b, z = fwd_cases[(M, N, K, density)]
    ref = [z, torch.tanh(z), torch.relu(z)][act].float()
    xg, wg, bg = x.to(gpu), w.to(gpu), b.to(gpu)
    before = ops.sparse_path_counts()
    lists = ops.sparse_rows_build(xg, want_record=False)
    # the output is a column slice of a wider buffer: the pad columns inside the 16-byte pitch become zeros (the dense
    # epilogue's contract), what lies behind them stays
    pad = (N + 3) // 4 * 4
    buf = torch.full((M, pad + 4), 3.0, device=gpu)
    y = ops.linear_fwd_sparse(lists, xg, wg, bg, act, out=buf[:, :N])
    after = ops.sparse_path_counts()
    assert after.fwd_sparse == before.fwd_sparse + 1 and after.fwd_dense == before.fwd_dense
    dense = ops.linear_fwd(xg, wg, bg, act)
    same_bits = torch.equal(y, dense)
    msg = "bits %s the dense product's" % ("equal" if same_bits else "differ from")
    assert _rel(y.cpu(), ref) < 2e-6, msg
    assert (y.cpu() - ref).abs().max().item() < 2e-5, msg
    assert _rel(y.cpu(), dense.cpu()) < 2e-6, msg
    assert float(buf[:, N:pad].abs().sum()) == 0.0 and bool((buf[:, pad:] == 3.0).all())


def test_linear_fwd_sparse_wide_input_runs_the_dense_product(gpu):
    """K > 512 does not fit the LDS slab: the entry point runs the dense product, decided from the shape, and says so"""
    from idiaptts_amd import ops
    M, N, K = 70, 33, 516
    x = torch.from_numpy(_sparse_matrix(M, K, 0.07, seed=1)).to(gpu)
    g = torch.Generator().manual_seed(2)
    w = ((torch.rand(N, K, generator=g) - 0.5) * (2.0 / K ** 0.5)).to(gpu)
    b = (torch.rand(N, generator=g) - 0.5).to(gpu)
    lists = ops.sparse_rows_build(x, want_record=False)
    before = ops.sparse_path_counts()
    y = ops.linear_fwd_sparse(lists, x, w, b, 1)
    after = ops.sparse_path_counts()
    assert after.fwd_dense == before.fwd_dense + 1 and after.fwd_sparse == before.fwd_sparse
    assert torch.equal(y, ops.linear_fwd(x, w, b, 1))


def _three_steps(gpu, sparse_input, batches):
    from idiaptts_amd.native_ff import FlatFFModel
    model = FlatFFModel((425, 512, 512, 187), ("tanh", "tanh", None), device=gpu, seed=4, sparse_input=sparse_input)
    losses = []
    for x, y, n in batches:
        valid = torch.ones(x.shape[0], dtype=torch.uint8, device=gpu)
        losses.append(model.train_step(x, y, valid, n).item())
    return model, losses


def _assert_same_training(model, losses, ref_model, ref_losses):
    """the numbers of test_ff_train_steps_match_reference_stack"""
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) < 1e-5 * abs(b)
    for i in range(len(model.layout)):
        assert (model.weight(i) - ref_model.weight(i)).abs().max().item() < 2e-6
        assert (model.bias(i) - ref_model.bias(i)).abs().max().item() < 2e-6


@pytest.fixture(scope="module")
def question_batches(gpu):
    from idiaptts_amd.bench_support import make_ff_batch
    out = []
    for step in range(3):
        x, y, lengths = make_ff_batch(3, seed=100 + step)
        out.append((x.to(gpu), y.to(gpu), float(lengths.sum())))
    return out


def test_model_sparse_input_matches_dense(gpu, question_batches):
    from idiaptts_amd import ops
    c0 = ops.sparse_path_counts()
    dense, dense_losses = _three_steps(gpu, False, question_batches)
    c1 = ops.sparse_path_counts()
    assert c1 == c0                                                  # forced off: no list, no sparse product
    sparse, sparse_losses = _three_steps(gpu, True, question_batches)
    c2 = ops.sparse_path_counts()
    assert c2.builds == c1.builds + 3 and c2.fwd_sparse == c1.fwd_sparse + 3
    _assert_same_training(sparse, sparse_losses, dense, dense_losses)


def test_model_chooses_from_the_first_batch(gpu, question_batches):
    from idiaptts_amd import ops
    dense, dense_losses = _three_steps(gpu, False, question_batches)
    c0 = ops.sparse_path_counts()
    auto, auto_losses = _three_steps(gpu, None, question_batches)
    c1 = ops.sparse_path_counts()
    assert auto.sparse_input is True
    assert c1.builds == c0.builds + 4 and c1.fwd_sparse == c0.fwd_sparse + 3     # one build more: the decision
    _assert_same_training(auto, auto_losses, dense, dense_losses)

    g = torch.Generator().manual_seed(9)
    M = question_batches[0][0].shape[0]
    uniform = [(torch.rand(M, 425, generator=g).to(gpu), question_batches[0][1], question_batches[0][2])]
    auto_u, _ = _three_steps(gpu, None, uniform)
    c2 = ops.sparse_path_counts()
    assert auto_u.sparse_input is False
    assert c2.builds == c1.builds + 1 and c2.fwd_sparse == c1.fwd_sparse         # the decision's build alone


def test_model_that_chose_sparse_takes_a_dense_batch(gpu, question_batches):
    """the decision holds: a later dense batch runs the sparse path (slower) and still meets the tolerance"""
    from idiaptts_amd import ops
    g = torch.Generator().manual_seed(11)
    M = question_batches[1][0].shape[0]
    batches = [question_batches[0],
               (torch.rand(M, 425, generator=g).to(gpu), question_batches[1][1], question_batches[1][2]),
               question_batches[2]]
    dense, dense_losses = _three_steps(gpu, False, batches)
    c0 = ops.sparse_path_counts()
    auto, auto_losses = _three_steps(gpu, None, batches)
    assert auto.sparse_input is True
    assert ops.sparse_path_counts().fwd_sparse == c0.fwd_sparse + 3
    _assert_same_training(auto, auto_losses, dense, dense_losses)
