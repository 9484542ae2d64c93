"""The ring GEMM's epilogues whose operands are fetched during the K loop (csrc/gemm_ring.h: EPI_DACT --
the input gradient times the previous activation's derivative -- and EPI_MSE -- the output layer fused
with the masked MSE) against the register-staged kernel, which has the same K order and no early loads.

Every case runs twice: on buffers the ring kernel takes (16-byte pitches and bases) and on copies it
refuses (a pitch that is no multiple of 4 floats), which the register-staged kernel computes.  The two
must agree BIT FOR BIT, and both are held to a torch float64 product within the bounds that
tests/test_gpu_nn.py uses for the same entry points.

The fused output layer (itts_linear_fwd_mse) requires 16-byte rows of x, w and dz, so the C ABI never
routes it to the staged kernel: its staged yardstick is itts_linear_fwd on a refused copy of x followed by
itts_masked_mse.  The gradient is the same float arithmetic per element and is compared bit for bit; the
loss is a sum of doubles taken in another (fixed) order there, so it is held to the 1e-6 relative bound of
test_output_layer_fused_with_the_masked_mse_equals_the_two_kernels, to float64 within 1e-5, and to
bit equality between two runs.  Against float64 the gradient is held element by element to the rounding
bound of its fp32 arithmetic (worked out in the test).

Sizes: the pair launch always has 512 persistent workgroups and the single launch up to 512, so a
workgroup meets a second tile -- the case in which the early operands live across a tile boundary --
only above 512 tiles; M = 16385 (1032 tiles of 128 x 64 at 512 columns, the last row tile one row high)
and M = 22017 (519 tiles at 187 columns) are there for that."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = {"tanh": 1, "relu": 2}


def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-30)


def _pad4(n):
    return (n + 3) // 4 * 4


def _sliced(t, pitch, offset=0, fill=0.0):
    """A copy of the [M, W] tensor t as the column slice [:, offset:offset + W] of an [M, pitch] buffer."""
    big = torch.full((t.shape[0], pitch), fill, dtype=t.dtype, device=t.device)
    view = big[:, offset:offset + t.shape[1]]
    view.copy_(t)
    return big, view


class _ran_on:
    """with _ran_on("ring", 2): the block must add exactly one product of epilogue kind 2 (0 store, 1 bias +
    activation, 2 activation derivative, 3 masked MSE) on the ring kernel and none of that kind on the other
    kernel (ops.gemm_path_counts) -- so that "ring against staged" can never be a kernel against itself."""

    def __init__(self, kernel, kind):
        self.kernel, self.kind = kernel, kind

    def __enter__(self):
        from idiaptts_amd import ops
        self.before = ops.gemm_path_counts()

    def __exit__(self, exc_type, exc, tb):
        from idiaptts_amd import ops
        if exc_type is not None:
            return False
        after = ops.gemm_path_counts()
        ring = after.ring[self.kind] - self.before.ring[self.kind]
        staged = after.staged[self.kind] - self.before.staged[self.kind]
        assert (ring, staged) == ((1, 0) if self.kernel == "ring" else (0, 1)), (self.kernel, self.kind, ring, staged)
        return False


def _bwd_inputs(M, N, K, act, gpu):
    g = torch.Generator().manual_seed(1000 * N + 7 * K + M)
    Kp, Np = _pad4(K), _pad4(N)
    x = torch.zeros(M, Kp)
    pre = torch.randn(M, K, generator=g)
    x[:, :K] = torch.tanh(pre) if act == "tanh" else torch.relu(pre)
    w = torch.zeros(N, Kp)
    w[:, :K] = torch.randn(N, K, generator=g) / N ** 0.5
    dz = torch.randn(M, N, generator=g)
    dzg = torch.zeros(M, Np, device=gpu)[:, :N]
    dzg.copy_(dz)
    return x, w, dz, x.to(gpu), w.to(gpu), dzg, Kp, Np


def _run_bwd(dzg, xg, wg, yprev, dx, act, N, Kp, Np, gpu, kernel="ring"):
    """itts_linear_bwd; `kernel`: the one the input-gradient product (EPI_DACT) must run on"""
    from idiaptts_amd import ops
    flat = torch.zeros(N * Kp + Np, device=gpu)
    dw, db = flat[:N * Kp].view(N, Kp), flat[N * Kp:N * Kp + N]
    with _ran_on(kernel, 2):
        ops.linear_bwd(dzg, xg, wg, dw, db, dx, yprev=yprev, act_prev=ACTS[act])
    torch.cuda.synchronize()
    return dw, db


BWD_SHAPES = [(187, 512), (512, 187), (187, 20), (20, 64)]   # (N out, K in): 6, 16, 6 and 1 K-steps per dX tile
BWD_CASES = [(M, N, K) for (N, K) in BWD_SHAPES for M in (1, 63, 129, 257, 1025)] + [(16385, 187, 512)]


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("M,N,K", BWD_CASES)
def test_linear_bwd_ring_equals_staged_bit_for_bit(gpu, M, N, K, act):
    x, w, dz, xg, wg, dzg, Kp, Np = _bwd_inputs(M, N, K, act, gpu)
    # buffers the ring kernel takes
    dx = torch.zeros(M, Kp, device=gpu)
    dw, db = _run_bwd(dzg, xg, wg, xg, dx, act, N, Kp, Np, gpu)
    # copies it refuses: dx and yprev with a pitch of Kp + 1 floats
    _, yprev_s = _sliced(xg, Kp + 1)
    _, dx_s = _sliced(torch.zeros(M, Kp, device=gpu), Kp + 1)
    dw_s, db_s = _run_bwd(dzg, xg, wg, yprev_s, dx_s, act, N, Kp, Np, gpu, kernel="staged")
    assert torch.equal(dx, dx_s)
    assert torch.equal(dw, dw_s) and torch.equal(db, db_s)
    # determinism
    dx2 = torch.zeros(M, Kp, device=gpu)
    dw2, db2 = _run_bwd(dzg, xg, wg, xg, dx2, act, N, Kp, Np, gpu)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    # float64 (bounds of test_fused_backward_equals_the_separate_calls_bit_for_bit / test_linear_bwd_input)
    dx_ref = dz.double() @ w.double()
    dx_ref = dx_ref * ((1 - x.double() ** 2) if act == "tanh" else (x.double() > 0))
    dw_ref = dz.double().t() @ x.double()
    db_ref = dz.double().sum(0)
    print("dx max err", (dx.cpu().double() - dx_ref).abs().max().item(), "rel", _rel(dx.cpu().double(), dx_ref))
    assert (dx.cpu().double() - dx_ref).abs().max() < 1e-5 * max(1.0, dx_ref.abs().max().item())
    assert _rel(dx.cpu().double(), dx_ref) < 2e-6
    assert (dw.cpu().double() - dw_ref).abs().max() < 2e-4 * max(1.0, dw_ref.abs().max().item())
    assert (db.cpu().double() - db_ref).abs().max() < 2e-4 * max(1.0, db_ref.abs().max().item())
    assert (dx[:, K:] == 0).all()            # pad columns inside the pitch: zeros


def _valid_rows(M, g):
    """Invalid rows at the first row, the last row and, from three row tiles on, the whole first tile of 128 rows."""
    valid = (torch.rand(M, generator=g) > 0.2).to(torch.uint8)
    if M == 1:
        valid[0] = 1
    if M > 1:
        valid[0] = 0
        valid[M - 1] = 0
        valid[M // 2] = 1
    if M > 256:
        valid[:128] = 0
    return valid


MSE_CASES = [(M, N, 96) for N in (187, 64, 1) for M in (1, 129, 257, 1025)] + [(257, 187, 512), (22017, 187, 64)]


@pytest.mark.parametrize("padded_target", [False, True])
@pytest.mark.parametrize("M,N,K", MSE_CASES)
def test_linear_fwd_mse_ring_equals_staged(gpu, M, N, K, padded_target):
    from idiaptts_amd import ops
    g = torch.Generator().manual_seed(100 * N + M + K)
    x = torch.randn(M, K, generator=g).to(gpu)
    w = (torch.randn(N, K, generator=g) * 0.1).to(gpu)
    b = torch.randn(N, generator=g).to(gpu)
    target = torch.randn(M, N, generator=g).to(gpu)
    if padded_target:
        _, target = _sliced(target, _pad4(N) + 4)
    valid = _valid_rows(M, g).to(gpu)
    n_valid = float(valid.sum().item())
    assert n_valid > 0

    def fused():
        dz = torch.zeros(M, _pad4(N), device=gpu)[:, :N]
        with _ran_on("ring", 3):
            loss, dz = ops.linear_fwd_mse(x, w, b, target, valid, n_valid, grad=dz)
        torch.cuda.synchronize()
        return loss, dz

    loss, dz = fused()
    # the staged kernel: x with a pitch of K + 1 floats
    _, x_s = _sliced(x, K + 1)
    with _ran_on("staged", 1):
        y = ops.linear_fwd(x_s, w, b, ops.ACT_NONE)
    loss_ref, dz_ref = ops.masked_mse(y, target, valid, n_valid)
    assert torch.equal(dz, dz_ref)
    print("loss", float(loss), "staged", float(loss_ref))
    assert abs(float(loss) - float(loss_ref)) <= 1e-6 * abs(float(loss_ref))
    # determinism: the loss partials are summed in a fixed order
    loss2, dz2 = fused()
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2)
    # float64
    yd = x.double().cpu() @ w.double().cpu().T + b.double().cpu()
    d = (yd - target.double().cpu()) * valid.cpu().double()[:, None]
    assert abs(float(loss) - float((d ** 2).sum() / (n_valid * N))) < 1e-5 * float(loss_ref)
    assert (dz[valid == 0] == 0).all()
    # the gradient, element by element, within what fp32 allows (u = 2^-24): the product is a chain of K fused
    # multiply-adds, off by at most K u sum_k |x_k w_k|; adding the bias and subtracting the target round once
    # each (u |y|, u |y - t|); the factor 2 / (n_valid N) is rounded to fp32 and so is the product with it (2 u of
    # the result).  A bound relative to the NORM of y - t would not hold for a single element: y - t cancels.
    u = 2.0 ** -24
    sum_abs = x.double().cpu().abs() @ w.double().cpu().abs().T
    gs = 2.0 / (n_valid * N)
    bound = gs * (K * u * sum_abs + u * yd.abs() + u * d.abs()) * 1.001 + 3 * u * gs * d.abs()   # 1.001: second-order terms
    err = (dz.cpu().double() - gs * d).abs()
    print("gradient: largest error / bound", float((err / (bound + 1e-300)).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("M", [129, 1025])
def test_linear_bwd_between_guard_columns(gpu, M, act):
    """dx and yprev as column slices of wider buffers filled with 1e30: nothing outside the slices is
    written, nothing outside them is used.  (512 columns: whole 64-column tiles, so no pad column inside
    the pitch is there to be zeroed.)"""
    N, K = 187, 512
    x, w, dz, xg, wg, dzg, Kp, Np = _bwd_inputs(M, N, K, act, gpu)
    dx = torch.zeros(M, Kp, device=gpu)
    dw, db = _run_bwd(dzg, xg, wg, xg, dx, act, N, Kp, Np, gpu)
    W = Kp + 12
    yprev_big, yprev_s = _sliced(xg, W, offset=8, fill=1e30)
    dx_big, dx_s = _sliced(torch.zeros(M, Kp, device=gpu), W, offset=4, fill=1e30)
    dw_s, db_s = _run_bwd(dzg, xg, wg, yprev_s, dx_s, act, N, Kp, Np, gpu)
    assert torch.equal(dx_s, dx) and torch.equal(dw_s, dw) and torch.equal(db_s, db)
    assert (dx_big[:, :4] == 1e30).all() and (dx_big[:, 4 + Kp:] == 1e30).all()
    assert (yprev_big[:, :8] == 1e30).all() and (yprev_big[:, 8 + Kp:] == 1e30).all()


@pytest.mark.parametrize("M", [129, 1025])
def test_linear_fwd_mse_between_guard_columns(gpu, M):
    """The gradient and the target as column slices of wider buffers filled with 1e30 (64 columns: one
    whole tile wide)."""
    from idiaptts_amd import ops
    N, K = 64, 96
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(gpu)
    w = (torch.randn(N, K, generator=g) * 0.1).to(gpu)
    b = torch.randn(N, generator=g).to(gpu)
    target = torch.randn(M, N, generator=g).to(gpu)
    valid = _valid_rows(M, g).to(gpu)
    n_valid = float(valid.sum().item())
    loss, dz = ops.linear_fwd_mse(x, w, b, target, valid, n_valid, grad=torch.zeros(M, N, device=gpu))
    t_big, t_s = _sliced(target, N + 7, offset=3, fill=1e30)
    dz_big, dz_s = _sliced(torch.zeros(M, N, device=gpu), N + 8, offset=4, fill=1e30)
    with _ran_on("ring", 3):
        loss_s, _ = ops.linear_fwd_mse(x, w, b, t_s, valid, n_valid, grad=dz_s)
    torch.cuda.synchronize()
    assert torch.equal(loss_s, loss) and torch.equal(dz_s, dz)
    assert (dz_big[:, :4] == 1e30).all() and (dz_big[:, 4 + N:] == 1e30).all()
    assert (t_big[:, :3] == 1e30).all() and (t_big[:, 3 + N:] == 1e30).all()
