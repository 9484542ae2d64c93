"""The all-pass warping specification (tests/allpass_spec.py) against itself: the reference's closed-form table
equals the recursion, dW is the derivative of W, the block / halving wrapper does what it says, and the torch twin
(whose autograd gradients the layer tests use) equals the numpy lines.  No GPU."""
import numpy as np
import pytest
import torch

from tests import allpass_spec as spec

ALPHAS = np.array([-0.5, -0.3, -0.05, 0.0, 0.1, 0.2, 0.45, 0.5])


@pytest.mark.parametrize("N", [2, 5, 8])
def test_closed_form_equals_recursion(N):
    W, _ = spec.warp_matrices(ALPHAS, N)
    err = np.abs(spec.closed_form_matrices(ALPHAS, N) - W).max()
    print("N = {}: closed form - recursion, max abs {:.3g}".format(N, err))
    assert err <= 1e-12


def test_closed_form_degrees_stay_below_the_cut():
    table = spec.closed_form_table(6)
    r, c, p = np.nonzero(table)
    assert (p <= r + c).all() and p.max() == 2 * 6 - 2


@pytest.mark.parametrize("N", [1, 5, 64])
def test_zero_alpha_gives_the_identity(N):
    W, dW = spec.warp_matrices(np.zeros(3), N)
    assert (W == np.eye(N)).all()
    x = np.random.default_rng(0).normal(size=(3, 4 * N))
    assert np.array_equal(spec.forward(x, np.zeros(3), N), x)


@pytest.mark.parametrize("N", [5, 30, 64])
def test_dW_is_the_central_difference_of_W(N):
    a = np.array([-0.7, -0.45, -0.2, 0.0, 0.3, 0.45, 0.7])
    h = 1e-6
    _, dW = spec.warp_matrices(a, N)
    fd = (spec.warp_matrices(a + h, N)[0] - spec.warp_matrices(a - h, N)[0]) / (2 * h)
    rel = np.abs(dW - fd).max() / np.abs(dW).max()
    print("N = {}: dW against central differences, relative {:.3g}".format(N, rel))
    assert rel <= 1e-7


def test_entries_are_bounded_by_one():
    W, _ = spec.warp_matrices(np.linspace(-0.7, 0.7, 29), 64)
    assert np.abs(W).max() <= 1.0


def test_blocks_0_to_2_are_halved_and_block_3_is_not():
    N, a = 4, np.array([0.3])
    W = spec.warp_matrices(a, N)[0][0]
    x = np.random.default_rng(1).normal(size=(1, 4 * N))
    y = spec.forward(x, a, N)
    for b in range(4):
        xb = x[0, b * N:(b + 1) * N].copy()
        if b < 3:
            xb[0] /= 2
        yb = xb @ W
        if b < 3:
            yb[0] *= 2
        np.testing.assert_allclose(y[0, b * N:(b + 1) * N], yb, rtol=0, atol=1e-15)
    plain = x[0, :N] @ W
    assert abs(y[0, 0] - plain[0]) > 1e-3 or abs(y[0, 1] - plain[1]) > 1e-3      # the halving is not a no-op


def test_normalisation_wraps_the_warp():
    N = 3
    rng = np.random.default_rng(2)
    x, a = rng.normal(size=(5, 2 * N)), rng.uniform(-0.4, 0.4, 5)
    mean, sd = rng.normal(size=2 * N), rng.uniform(0.5, 2.0, 2 * N)
    y = spec.forward(x, a, N, mean, sd)
    np.testing.assert_allclose(y, (spec.forward(x * sd + mean, a, N) - mean) / sd, rtol=0, atol=1e-14)
    np.testing.assert_allclose(spec.forward(x, a, N, mean, None), spec.forward(x + mean, a, N) - mean, atol=1e-14)
    np.testing.assert_allclose(spec.forward(x, a, N, None, sd), spec.forward(x * sd, a, N) / sd, atol=1e-14)


@pytest.mark.parametrize("N,nb,norm", [(1, 1, False), (5, 4, True), (8, 3, False), (8, 1, True)])
def test_torch_twin_equals_numpy_spec_and_its_autograd_the_written_gradients(N, nb, norm):
    rng = np.random.default_rng(3)
    M, D = 6, nb * N
    x, a, dy = rng.normal(size=(M, D)), rng.uniform(-0.45, 0.45, M), rng.normal(size=(M, D))
    mean = rng.normal(size=D) if norm else None
    sd = rng.uniform(0.5, 2.0, D) if norm else None
    tx = torch.tensor(x, requires_grad=True)
    ta = torch.tensor(a[:, None], requires_grad=True)
    ty = spec.torch_forward(tx, ta, N, None if mean is None else torch.tensor(mean),
                            None if sd is None else torch.tensor(sd))
    np.testing.assert_allclose(ty.detach().numpy(), spec.forward(x, a, N, mean, sd), rtol=0, atol=1e-13)
    ty.backward(torch.tensor(dy))
    dx, da = spec.backward(dy, x, a, N, mean, sd)
    np.testing.assert_allclose(tx.grad.numpy(), dx, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ta.grad.numpy()[:, 0], da.sum(axis=1), rtol=0, atol=1e-12)


def test_float32_closed_form_breaks_where_the_recursion_holds():
    """why the kernel applies the recursion: at N = 60 the table's coefficients overflow float32"""
    with np.errstate(over="ignore"):
        assert not np.isfinite(spec.closed_form_table(60).astype(np.float32)).all()
    a = np.array([-0.45, 0.2, 0.45])
    W32, _ = spec.warp_matrices(a, 60, np.float32)
    assert np.abs(W32 - spec.warp_matrices(a, 60)[0]).max() <= 2.7e-7
