"""The column block of layer 0's sparse weight gradient built from the row lists of x
(itts_sparse_cols_build_from_rows) against the block built from x itself (itts_sparse_cols_build): every defined byte
-- the counts of all 512 (owner, slot) pairs of every tile, every list up to its padded count, the whole strip -- then
the weight gradient on both blocks and the flat model with either build.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 256                                   # rows of a tile
BLOCK = 16                                # entries of a list block
DENORMAL = np.float32(1e-41)


def _layout(M, K):
    from idiaptts_amd import lib
    out = (ctypes.c_int64 * 3)()
    lib.check(lib.load().itts_sparse_cols_layout(M, K, out), "itts_sparse_cols_layout")
    return [int(v) for v in out]


def _decode(cols):
    """(counts uint16 [tiles * 512], entries int32 [tiles * 512, 256, 2], strip uint32 [tiles * 256, 32]) of a block"""
    from idiaptts_amd import ops
    lists = ops.SPARSE_COLS_OWNERS * ops.SPARSE_COLS_SLOTS
    strip_off, streams_off, nbytes = _layout(cols.M, cols.K)
    tiles = (cols.M + T - 1) // T
    raw = cols.block[:nbytes].cpu().numpy()
    strip = raw[strip_off:streams_off].view(np.uint32).reshape(tiles * T, ops.SPARSE_COLS_HEAVY + 1)
    at = streams_off
    counts = raw[at:at + tiles * lists * 2].view(np.uint16)
    at += tiles * lists * 2
    first = raw[at:at + tiles * lists * BLOCK * 8].view(np.int32).reshape(tiles * lists, BLOCK, 2)
    at += tiles * lists * BLOCK * 8
    over = raw[at:at + tiles * lists * (T - BLOCK) * 8].view(np.int32).reshape(tiles * lists, T - BLOCK, 2)
    assert at + over.nbytes == nbytes
    return counts, np.concatenate([first, over], axis=1), strip


def _assert_same_block(a, b, what):
    """every defined byte of two decoded blocks; returns the counts"""
    (ca, ea, sa), (cb, eb, sb) = a, b
    assert np.array_equal(ca, cb), what
    padded = (ca.astype(np.int64) + BLOCK - 1) // BLOCK * BLOCK
    defined = np.arange(T)[None, :] < padded[:, None]
    assert np.array_equal(ea[defined], eb[defined]), what
    assert np.array_equal(sa, sb), what
    return ca


def _matrix(M, K, density, seed, wide=3):
    """float32 [M, pad4(K + wide) + 4]: columns 0..K-1 at `density` with a row of K entries (row M / 2), a column
    `full` that is non-zero in all rows of tile 0, an all-zero row outside tile 0 (row 0 where M < 256, so that
    tile 0's 256 entries of `full` stay; none at M = 256), a -0.0, a NaN and a denormal (rows 1..3); `wide` more
    columns of non-zeros behind K (lists built over K + wide columns name them, a plan over K must not); zeros behind
    those"""
    rng = np.random.default_rng(seed)
    x = np.zeros((M, (K + wide + 3) // 4 * 4 + 4), dtype=np.float32)
    vals = (1.0 - rng.random((M, K))).astype(np.float32)
    x[:, :K] = np.where(rng.random((M, K)) < density, vals, np.float32(0.0))
    full = K // 2
    x[:, full] = vals[:, full]
    x[M // 2, :K] = vals[M // 2]
    if M != T:
        x[0 if M < T else T, :K] = 0.0
    x[:, K:K + wide] = 0.5
    specials = {}
    if M >= 4 and K >= 4:
        cols = [k for k in rng.permutation(K) if k != full][:3]
        for row, col, v in zip((1, 2, 3), cols, (np.float32(-0.0), np.float32("nan"), DENORMAL)):
            x[row, col] = v
            specials[(row, col)] = v
    return x, full, specials


def _minus_zero_columns(specials):
    return {col for (row, col), v in specials.items() if v == 0}


def _plan(ops, x, K, heavy, never_heavy, seed, gpu):
    """a plan over K columns with exactly min(heavy, K - 1) heavy columns, none of them in `never_heavy`"""
    M = x.shape[0]
    counts = [int(c) for c in (x[:, :K] != 0).sum(axis=0)]
    rng = np.random.default_rng(seed)
    pick = [k for k in rng.permutation(K) if k not in never_heavy][:heavy]
    for k in pick:
        counts[k] = 10 * M + 10
    plan = ops.SparseColsPlan(counts, M, gpu, heavy_density=5.0)
    assert sorted(plan.heavy) == sorted(pick)
    return plan


def _list_of(ops, plan, col):
    """owner * 8 + slot of a light column"""
    return [o * ops.SPARSE_COLS_SLOTS + s for o, cs in enumerate(plan.owners) for s, k in enumerate(cs) if k == col][0]


def _both_blocks(ops, xg, plan, K, K_lists):
    """(block from x, block from the row lists over K_lists columns), decoded; both into blocks of 0xFF bytes"""
    M = xg.shape[0]
    rows = ops.sparse_rows_build(xg, K=K_lists)
    out = []
    for lists in (None, rows):
        cols = ops.SparseCols(M, K, xg.device)
        cols.block.fill_(0xFF)
        before = ops.sparse_wgrad_counts()
        built = ops.sparse_cols_build(xg, plan, K=K, cols=cols, lists=lists)
        assert built.block.data_ptr() == cols.block.data_ptr()
        assert ops.sparse_wgrad_counts().col_builds == before.col_builds + 1
        out.append(built)
    return out


@pytest.mark.parametrize("K", [1, 63, 64, 65, 425, 512])
@pytest.mark.parametrize("M", [1, 16, 255, 256, 257, 600])
def test_block_equals_the_build_from_x(gpu, M, K):
    from idiaptts_amd import ops
    case = 0
    for density in (0.0, 0.02, 0.10, 0.50):
        for heavy in (0, 9, 31):
            case += 1
            x, full, specials = _matrix(M, K, density, seed=M * 1000 + K + case)
            # the -0.0 stays in a light column: a strip cell keeps its sign only in the build from x (the test below)
            never = _minus_zero_columns(specials) | ({full} if heavy != 31 else set())
            plan = _plan(ops, x, K, heavy, never, seed=case, gpu=gpu)
            xg = torch.from_numpy(x).to(gpu)
            K_lists = K + 3 if case % 2 else K
            from_x, from_rows = (_decode(c) for c in _both_blocks(ops, xg, plan, K, K_lists))
            what = "M %d K %d density %g heavy %d lists over %d" % (M, K, density, len(plan.heavy), K_lists)
            counts = _assert_same_block(from_rows, from_x, what)
            # what the blocks hold, not only that they agree: the counts are the light columns' non-zeros
            light = [k for k in range(K) if k not in plan.heavy]
            nonzero = (x[:, :K].view(np.uint32) & 0x7FFFFFFF) != 0
            assert int(counts.sum()) == int(nonzero[:, light].sum()), what
            if full in light and M >= T:
                code = _list_of(ops, plan, full)
                assert counts[code] == T, what                      # 256 entries: all 16 blocks of the list
                rows_of = from_rows[1][code, :, 0]
                assert np.array_equal(rows_of, np.arange(T) * 256), what


def test_special_values_and_columns_behind_the_plan(gpu):
    """-0.0 is dropped, NaN and a denormal are kept, listed columns 425..427 appear nowhere"""
    from idiaptts_amd import ops
    M, K = 257, 425
    x, full, specials = _matrix(M, K, 0.10, seed=77)
    plan = _plan(ops, x, K, 9, {col for row, col in specials} | {full}, seed=3, gpu=gpu)
    xg = torch.from_numpy(x).to(gpu)
    from_x, from_rows = (_decode(c) for c in _both_blocks(ops, xg, plan, K, 428))
    _assert_same_block(from_rows, from_x, "specials")
    counts, entries, strip = from_rows
    for (row, col), v in specials.items():
        code = _list_of(ops, plan, col)
        listed = entries[code, :counts[code]]                       # tile 0
        hit = listed[listed[:, 0] == row * 256]
        if v == 0:
            assert len(hit) == 0
        else:
            assert len(hit) == 1 and hit[0, 1] == int(np.array([v]).view(np.int32)[0])
    light = [k for k in range(K) if k not in plan.heavy]
    nonzero = (x[:, :K].view(np.uint32) & 0x7FFFFFFF) != 0
    assert int(counts.sum()) == int(nonzero[:, light].sum())        # nothing of columns 425..427 (257 x 3 entries)


def test_minus_zero_in_a_heavy_column(gpu):
    """The one place where the two builds may differ: the strip copies x's bits in the build from x, and the row
    lists do not hold a -0.0.  The cell is +0.0 from the lists, every other byte is equal, and no sum depends on the
    sign of a zero factor: dw and db are bit-equal."""
    from idiaptts_amd import ops
    M, N, K = 257, 64, 64
    x, full, specials = _matrix(M, K, 0.5, seed=5)
    plan = _plan(ops, x, K, 9, _minus_zero_columns(specials) | {full}, seed=9, gpu=gpu)
    col = plan.heavy[4]
    x[7, col] = -0.0
    xg = torch.from_numpy(x).to(gpu)
    a, b = _both_blocks(ops, xg, plan, K, K)
    from_x, from_rows = _decode(a), _decode(b)
    h = plan.heavy.index(col)
    assert from_x[2][7, h] == 0x80000000 and from_rows[2][7, h] == 0
    from_x[2][7, h] = 0
    _assert_same_block(from_rows, from_x, "minus zero")
    dz = _dz(M, N, 1, gpu)
    dw_x, db_x = ops.linear_bwd_weight_sparse(dz, xg, a, plan, K=K)
    dw_r, db_r = ops.linear_bwd_weight_sparse(dz, xg, b, plan, K=K)
    assert torch.equal(dw_x.view(torch.int32), dw_r.view(torch.int32))
    assert torch.equal(db_x.view(torch.int32), db_r.view(torch.int32))


@pytest.mark.parametrize("M,N,K,lddw", [(600, 70, 425, 428), (257, 64, 64, 64)])
def test_weight_gradient_is_bit_equal(gpu, M, N, K, lddw):
    from idiaptts_amd import ops
    x, full, specials = _matrix(M, K, 0.07, seed=M + N)
    for key in specials:
        x[key] = 0.25                                               # no NaN in the sums
    plan = _plan(ops, x, K, 9, set(), seed=2, gpu=gpu)
    xg = torch.from_numpy(x).to(gpu)
    a, b = _both_blocks(ops, xg, plan, K, K + 3)
    dz = _dz(M, N, M, gpu)
    before = ops.sparse_wgrad_counts()
    dw_x, db_x = ops.linear_bwd_weight_sparse(dz, xg, a, plan, dw=torch.full((N, lddw), 5.0, device=gpu), K=K)
    dw_r, db_r = ops.linear_bwd_weight_sparse(dz, xg, b, plan, dw=torch.full((N, lddw), 5.0, device=gpu), K=K)
    after = ops.sparse_wgrad_counts()
    assert after.dw_sparse == before.dw_sparse + 2 and after.dw_dense == before.dw_dense
    assert torch.equal(dw_x.view(torch.int32), dw_r.view(torch.int32))
    assert torch.equal(db_x.view(torch.int32), db_r.view(torch.int32))
    assert float(dw_r[:, :K].abs().sum()) > 0.0


def _dz(M, N, seed, gpu):
    """[M, N] view of a [M, pad4(N)] buffer (16-byte rows, as the model's), values in (-0.25, 0.75)"""
    buf = torch.full((M, (N + 3) // 4 * 4), 3.0)
    buf[:, :N] = torch.rand(M, N, generator=torch.Generator().manual_seed(seed)) - 0.25
    return buf.to(gpu)[:, :N]


def _batch(M, seed, gpu):
    """the recipe of bench_support.make_ff_batch at a chosen number of rows"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(M, 425, generator=g) < 0.05).float()
    x[:, 416:] = torch.rand(M, 9, generator=g)
    return x.to(gpu), torch.randn(M, 187, generator=g).to(gpu)


def test_model_steps_are_byte_equal(gpu):
    from idiaptts_amd import ops
    from idiaptts_amd.native_ff import FlatFFModel
    batches = [_batch(500, 11, gpu), _batch(530, 12, gpu)]
    results = []
    for from_lists in (True, False):
        model = FlatFFModel((425, 512, 512, 187), ("tanh", "tanh", None), device=gpu, seed=4, sparse_input=True,
                            sparse_wgrad=True)
        assert model.cols_from_lists is True
        model.cols_from_lists = from_lists
        before = ops.sparse_wgrad_counts()
        losses = []
        for step in range(3):
            x, y = batches[step % 2]
            valid = torch.ones(x.shape[0], dtype=torch.uint8, device=gpu)
            losses.append(model.train_step(x, y, valid, float(x.shape[0])).clone())
        after = ops.sparse_wgrad_counts()
        assert after.col_builds == before.col_builds + 3 and after.dw_sparse == before.dw_sparse + 3
        assert after.dw_dense == before.dw_dense
        results.append((model.params.clone(), torch.stack([l.reshape(()) for l in losses])))
    (params_a, loss_a), (params_b, loss_b) = results
    assert torch.equal(params_a.view(torch.int32), params_b.view(torch.int32))
    assert torch.equal(loss_a.view(torch.int32), loss_b.view(torch.int32))
    assert bool(torch.isfinite(loss_a).all())


def test_repeated_build_gives_the_same_block(gpu):
    from idiaptts_amd import ops
    M, K = 600, 425
    x, full, _ = _matrix(M, K, 0.10, seed=31)
    plan = _plan(ops, x, K, 9, set(), seed=4, gpu=gpu)
    xg = torch.from_numpy(x).to(gpu)
    rows = ops.sparse_rows_build(xg, K=428)
    blocks = []
    for fill in (0xFF, 0x00):
        cols = ops.SparseCols(M, K, gpu)
        cols.block.fill_(fill)
        blocks.append(_decode(ops.sparse_cols_build(xg, plan, K=K, cols=cols, lists=rows)))
    _assert_same_block(blocks[0], blocks[1], "repeat")


def test_lists_of_another_shape_are_refused(gpu):
    from idiaptts_amd import ops
    x, _, _ = _matrix(40, 64, 0.1, seed=1)
    xg = torch.from_numpy(x).to(gpu)
    plan = ops.sparse_cols_plan(xg, K=64)
    with pytest.raises(ValueError):
        ops.sparse_cols_build(xg, plan, K=64, lists=ops.sparse_rows_build(xg[:39], K=64))
    with pytest.raises(ValueError):
        ops.sparse_cols_build(xg, plan, K=64, lists=ops.sparse_rows_build(xg, K=63))
