"""The load schedule of the sparse layer-0 forward ("Load schedule and slot"): a wave requests
the counts and the first 48 entries (kAhead) of the next four rows before it walks the current four, rows longer than
that fetch the rest inside the walk, and the wait before the next group leaves the 16-byte store of y in flight.

Row lengths stand on every boundary of that schedule (the trips of 8, the fetches of 16, kAhead, dense rows), in
groups of four that mix them.  With exact inputs (values from {1, 0.5, 2, -1}, weights and bias multiples of 2^-6 in
[-2, 2]: every partial sum is a multiple of 2^-7 below 2^11, so any summation order gives the same float) the output
must equal the float64 product bit for bit: a dropped, doubled or misplaced entry shows.

A wave walks more than one group only where a row range has more than 64 rows, which the launch allows only once the
column slabs outnumber the compute units' share: the `deep` shapes (N = 16 384: one range, up to five groups a wave)
are there for the hand-off from one group to the next."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_AHEAD = 48                                   # kAhead of csrc/sparse_rows.hip
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, K_AHEAD - 1, K_AHEAD, K_AHEAD + 1, 63, 64, 65, -1)   # -1: K
MS = (1, 3, 4, 5, 130, 259)
VALUES = np.array([1.0, 0.5, 2.0, -1.0], dtype=np.float32)
SENTINEL = 77.0


def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-30)


def _pad4(n):
    return (n + 3) // 4 * 4


def _row_lengths(M, K):
    """non-zeros per row: every length of LENGTHS (clipped to K) in turn, seven places on per row so that the four
    rows of a group differ widely; then the fixed groups: long rows (0-3), four zero rows right behind them (4-7)
    and in the same wave's next group of a range of more than 64 rows (64-67), a long row beside three short ones
    (8-11), and the matrix' last row dense (alone in its group where M % 4 == 1)"""
    full = [K if v < 0 else min(v, K) for v in LENGTHS]
    lens = [full[(7 * m + 3) % len(full)] for m in range(M)]

    def put(m0, vals):
        for i, v in enumerate(vals):
            if m0 + i < M:
                lens[m0 + i] = min(v, K)

    put(0, (K, 65, 64, 63))
    put(4, (0, 0, 0, 0))
    put(8, (1, K, 0, 7))
    put(64, (0, 0, 0, 0))
    put(128, (49, 48, K, 47))
    for m in range(max(M - 4, 0), M - 1):       # the last row's neighbours, if it has any, are short
        if m >= 12:
            lens[m] = min((0, 1, 9)[m % 3], K)
    lens[M - 1] = K
    return lens


@functools.lru_cache(maxsize=None)
def _exact_x(M, K, ldx):
    """float32 [M, ldx]: row m has _row_lengths(M, K)[m] non-zeros from VALUES at random columns below K; columns
    from K on hold the sentinel"""
    rng = np.random.default_rng(1000 * M + K)
    x = np.zeros((M, ldx), dtype=np.float32)
    x[:, K:] = SENTINEL
    lens = _row_lengths(M, K)
    for m, n in enumerate(lens):
        cols = rng.choice(K, size=n, replace=False)
        x[m, cols] = VALUES[rng.integers(0, 4, size=n)]
    return torch.from_numpy(x), lens


def _exact_w(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-128, 129, (N, K), generator=g).float() / 64.0
    b = torch.randint(-128, 129, (N,), generator=g).float() / 64.0
    return w, b


def _out(M, N, wide, gpu):
    """[M, N] view of a sentinel-filled buffer.  wide: 16-byte aligned rows with one float4 of columns behind the
    padded width, which no store may touch; else a pitch that is no multiple of four floats"""
    if wide:
        pitch = _pad4(N) + 4
    else:
        pitch = N + 1 if (N + 1) % 4 else N + 2
    buf = torch.full((M, pitch), SENTINEL, device=gpu)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:, :N]


def _check_frame(buf, N, wide):
    """the pad columns inside the 16-byte pitch are zeros (as the dense epilogue writes them), everything behind is
    untouched"""
    first = _pad4(N) if wide else N
    if wide:
        assert torch.all(buf[:, N:first] == 0.0)
    assert torch.all(buf[:, first:] == SENTINEL)


def _w_both(w, gpu):
    """the same w at a 16-byte aligned address and one float further on"""
    N, K = w.shape
    store = torch.empty(2 * N * K + 8, device=gpu)
    w_al = store[:N * K].view(N, K)
    off = (N * K + 3) // 4 * 4 + 1
    w_mis = store[off:off + N * K].view(N, K)
    assert w_al.data_ptr() % 16 == 0 and w_mis.data_ptr() % 16 == 4
    w_al.copy_(w)
    w_mis.copy_(w)
    return w_al, w_mis


def _lists(x, K):
    from idiaptts_amd import ops
    xv = x[:, :K]
    return xv, ops.sparse_rows_build(xv, want_record=False)


# ------------------------------------------------------------------------------------------------- exact inputs
def test_row_lengths_cover_the_schedule():
    """(no device) the lengths that the exact tests run: every boundary is there, groups mix them"""
    lens = _row_lengths(259, 512)
    assert set(lens) >= {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 512}
    assert lens[0:4] == [512, 65, 64, 63] and lens[4:8] == [0, 0, 0, 0] and lens[64:68] == [0, 0, 0, 0]
    assert lens[8:12] == [1, 512, 0, 7]
    assert lens[258] == 512 and max(lens[256:258]) <= 9
    assert _row_lengths(5, 512)[4] == 512 and _row_lengths(1, 7) == [7]
    groups = [lens[i:i + 4] for i in range(12, 256, 4) if i not in (64, 128)]
    assert sum(max(g) - min(g) >= 30 for g in groups) > len(groups) // 2


@pytest.mark.parametrize("K,ldx", [(7, 7), (64, 64), (425, 428), (512, 512)])
@pytest.mark.parametrize("N", [1, 64, 65, 187])
def test_exact_rows_across_the_schedule(gpu, N, K, ldx):
    from idiaptts_amd import ops
    w, b = _exact_w(N, K, seed=N * 1000 + K)
    w_al, w_mis = _w_both(w, gpu)
    bg = b.to(gpu)
    before = ops.sparse_path_counts().fwd_sparse
    launches = 0
    for M in MS:
        x, lens = _exact_x(M, K, ldx)
        xg = x.to(gpu)
        xv, lists = _lists(xg, K)
        assert lists.counts().tolist() == lens
        ref = (xv.double() @ w_al.double().t() + bg.double()).float()
        for wide in (True, False):
            for wg in (w_al, w_mis):
                buf, out = _out(M, N, wide, gpu)
                ops.linear_fwd_sparse(lists, xv, wg, bg, ops.ACT_NONE, out=out)
                launches += 1
                assert torch.equal(out, ref), "M %d wide %s: %d cells differ" % (M, wide, (out != ref).sum().item())
                _check_frame(buf, N, wide)
    assert ops.sparse_path_counts().fwd_sparse == before + launches


@pytest.mark.parametrize("K,ldx", [(64, 64), (425, 428)])
@pytest.mark.parametrize("M", [259, 1030])
def test_exact_rows_deep(gpu, M, K, ldx):
    """N = 16 384 is 256 column slabs: one row range, so a wave walks up to five (M = 259) or seventeen (1030)
    groups one after the other, and the zero rows 64-67 are the group its wave 0 meets behind the long rows 0-3"""
    from idiaptts_amd import ops
    N = 16384
    w, b = _exact_w(N, K, seed=M + K)
    wg, bg = w.to(gpu), b.to(gpu)
    x, lens = _exact_x(M, K, ldx)
    xv, lists = _lists(x.to(gpu), K)
    assert lists.counts().tolist() == lens
    ref = (xv.double() @ wg.double().t() + bg.double()).float()
    for wide in (True, False):
        buf, out = _out(M, N, wide, gpu)
        ops.linear_fwd_sparse(lists, xv, wg, bg, ops.ACT_NONE, out=out)
        assert torch.equal(out, ref), "wide %s: %d cells differ" % (wide, (out != ref).sum().item())
        _check_frame(buf, N, wide)


# ------------------------------------------------------------------------------------------------ random inputs
def _random_case(M, N, K, ldx, gpu, seed):
    """values uniform in (0, 1] at the places of the exact matrix, w and b as tests/test_gpu_nn.py draws them"""
    g = torch.Generator().manual_seed(seed)
    x, _ = _exact_x(M, K, ldx)
    x = x.clone()
    vals = 1.0 - torch.rand(M, K, generator=g)
    x[:, :K] = torch.where(x[:, :K] != 0, vals, torch.zeros(()))
    w = (torch.rand(N, K, generator=g) - 0.5) * (2.0 / K ** 0.5)
    b = torch.rand(N, generator=g) - 0.5
    return x.to(gpu), w.to(gpu), b.to(gpu)


@pytest.mark.parametrize("M,N,K,ldx", [(130, 187, 425, 428), (259, 65, 512, 512), (259, 64, 64, 64), (5, 187, 7, 7),
                                       (259, 16384, 64, 64)])
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_random_rows_against_fp64(gpu, M, N, K, ldx, act):
    """the tolerances of the dense forward in tests/test_gpu_nn.py (2e-6 relative L2, 2e-5 on every output); sigmoid
    runs the other activation family's instantiation"""
    from idiaptts_amd import ops
    xg, wg, bg = _random_case(M, N, K, ldx, gpu, seed=M * 31 + N)
    xv, lists = _lists(xg, K)
    z = xv.double() @ wg.double().t() + bg.double()
    ref = (torch.tanh(z) if act == "tanh" else torch.sigmoid(z)).float()
    for wide in (True, False):
        buf, out = _out(M, N, wide, gpu)
        ops.linear_fwd_sparse(lists, xv, wg, bg, ops.ACT_BY_NAME[act], out=out)
        print("wide %s: rel %.2e max %.2e" % (wide, _rel(out, ref), (out - ref).abs().max().item()))
        assert _rel(out, ref) < 2e-6
        assert (out - ref).abs().max().item() < 2e-5
        _check_frame(buf, N, wide)


# ----------------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("wide", [True, False])
def test_special_values_land_where_the_dense_product_puts_them(gpu, wide):
    """NaN, +-inf and a denormal as list values, in the first fetch, behind kAhead and in a dense row; row 3 of w is
    all zeros, so an infinity gives NaN there in both products"""
    from idiaptts_amd import ops
    M, N, K, ldx = 130, 187, 425, 428
    xg, wg, bg = _random_case(M, N, K, ldx, gpu, seed=9)
    wg[3] = 0.0
    xv = xg[:, :K]
    nan, inf, den = float("nan"), float("inf"), 1e-40
    lens = _row_lengths(M, K)
    places = {0: (nan, 400), 1: (inf, 2), 2: (-inf, 424), 3: (den, 60), 9: (inf, 300), 12: (nan, 0), 13: (den, 5),
              M - 1: (-inf, 200)}
    for m, (v, k) in places.items():
        xv[m, k] = v
    xv[9, 17], xv[9, 410] = inf, -inf                 # both signs in one row: NaN wherever both weights are non-zero
    empty = lens.index(0)
    xv[empty, 7] = den                                # a list of one denormal
    xv, lists = _lists(xg, K)
    dense = ops.linear_fwd(xv, wg, bg, ops.ACT_NONE)
    buf, out = _out(M, N, wide, gpu)
    ops.linear_fwd_sparse(lists, xv, wg, bg, ops.ACT_NONE, out=out)
    assert torch.isnan(dense).any() and torch.isinf(dense).any()
    assert torch.equal(torch.isnan(out), torch.isnan(dense))
    assert torch.equal(torch.isposinf(out), torch.isposinf(dense))
    assert torch.equal(torch.isneginf(out), torch.isneginf(dense))
    fin = torch.isfinite(dense)
    assert (out[fin] - dense[fin]).abs().max().item() < 2e-5
    ref = (xv[empty].double() @ wg.double().t() + bg.double()).float()
    assert (out[empty] - ref).abs().max().item() < 2e-5
    _check_frame(buf, N, wide)


# ----------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("M,N,K,ldx", [(259, 187, 425, 428), (259, 16384, 64, 64)])
def test_dropout_entry_point_against_the_dense_dropout_forward(gpu, M, N, K, ldx):
    """same seed, salt and row offset: the same cells are dropped and the kept ones carry the same scale"""
    from idiaptts_amd import ops
    xg, wg, bg = _random_case(M, N, K, ldx, gpu, seed=5)
    xv, lists = _lists(xg, K)
    drop = dict(p=0.3, seed=1234567, salt=3, row_offset=1000)
    dense = ops.linear_fwd_dropout(xv, wg, bg, ops.ACT_TANH, **drop)
    for wide in (True, False):
        buf, out = _out(M, N, wide, gpu)
        ops.linear_fwd_sparse_dropout(lists, xv, wg, bg, ops.ACT_TANH, out=out, **drop)
        assert torch.equal(out == 0, dense == 0)
        assert 0.2 < (out == 0).float().mean().item() < 0.4
        assert _rel(out, dense) < 2e-6
        assert (out - dense).abs().max().item() < 2e-5
        _check_frame(buf, N, wide)
