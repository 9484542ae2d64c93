"""The last launch of every loss entry point (loss_final_sum, csrc/nn.hip): `loss[0]` against the float64 sum of the
call's own per-row / per-element output, at one partial sum (where a wrong count shows) and at just over 256 (where
the final kernel's strided loop wraps).  The number of partial sums is read from the entry's workspace query.

The kernels add the same float32 values in double, in another order than torch: the two sums differ by at most
n * 2^-53 relative, which moves the float32 rounding by one step at the most -- one float32 ulp is allowed."""
import numpy as np
import pytest
import torch

from idiaptts_amd import lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

ENTRIES = ("masked_mse", "weighted_mse", "weighted_l1", "vae_kld", "softmax_xent", "softmax_xent_strided", "mol_loss")
SIZES = ("one", "wrap")


def _weights(gen, n):
    w = torch.rand(n, generator=gen) + 0.5
    w[::5] = 0.                            # masked rows
    return w


def run_case(entry, size):
    """-> dict(nb: partial sums of the call, loss [1], grads: list, elem or None, terms: float64 tensor whose sum the
    loss is) on the device.  Fixed seeds: the same inputs on every call."""
    L = lib.load()
    gen = torch.Generator().manual_seed(ENTRIES.index(entry) * 2 + SIZES.index(size))
    big = size == "wrap"
    if entry in ("masked_mse", "weighted_mse", "weighted_l1"):
        M, D = (257, 256) if big else (5, 7)
        nb = L.itts_masked_mse_workspace_bytes(M, D) // 8
        pred, target = torch.randn(M, D, generator=gen).to(DEV), torch.randn(M, D, generator=gen).to(DEV)
        if entry == "masked_mse":
            valid = (_weights(gen, M) > 0).to(torch.uint8).to(DEV)
            n_valid, loss_weight = float(valid.sum()), 0.75
            loss, grad = ops.masked_mse(pred, target, valid, n_valid, loss_weight=loss_weight)
            terms = ((pred - target).float().double() ** 2)[valid.bool()] * (loss_weight / (n_valid * D))
            return dict(nb=nb, loss=loss, grads=[grad], elem=None, terms=terms)
        loss, grad, elem = ops.weighted_loss(pred, target, _weights(gen, M).to(DEV), 0 if entry == "weighted_mse" else 1,
                                             want_elem=True)
    elif entry == "vae_kld":
        M, lat = (4 * 257, 4) if big else (3, 4)
        nb = L.itts_vae_kld_workspace_bytes(M, lat) // 8
        mu, lv = torch.randn(M, lat, generator=gen).to(DEV), torch.randn(M, lat, generator=gen).to(DEV)
        loss, dmu, dlv, elem = ops.vae_kld(mu, lv, _weights(gen, M).to(DEV), want_elem=True)
        return dict(nb=nb, loss=loss, grads=[dmu, dlv], elem=elem, terms=elem.double())
    elif entry == "softmax_xent":
        N, C = (257 * 256, 4) if big else (7, 4)
        nb = L.itts_softmax_xent_workspace_bytes(N, C) // 8
        x = torch.randn(N, C, generator=gen).to(DEV)
        t = torch.randint(0, C, (N,), generator=gen).to(DEV)
        loss, grad, elem = ops.softmax_xent(x, t, _weights(gen, N).to(DEV), want_elem=True)
    elif entry == "softmax_xent_strided":
        B, C, T, shift = (257, 3, 9, 1) if big else (1, 3, 9, 1)
        nb = L.itts_softmax_xent_strided_workspace_bytes(B, T) // 8
        x = torch.randn(B, C, T, generator=gen).to(DEV)
        onehot = torch.nn.functional.one_hot(torch.randint(0, C, (B, T), generator=gen), C).transpose(1, 2).float()
        loss, grad, elem = ops.softmax_xent_strided(x, onehot.to(DEV), _weights(gen, B * (T - shift)).to(DEV),
                                                    shift=shift, want_elem=True)
    else:
        B, K, T, shift = (257, 2, 9, 1) if big else (1, 2, 9, 1)
        nb = L.itts_mol_loss_workspace_bytes(B, T) // 8
        x = torch.randn(B, 3 * K, T, generator=gen).to(DEV)
        y = (torch.rand(B, 1, T, generator=gen) * 2 - 1).to(DEV)
        loss, grad, elem = ops.mol_loss(x, y, _weights(gen, B * (T - shift)).to(DEV), shift=shift, want_elem=True)
    return dict(nb=nb, loss=loss, grads=[grad], elem=elem, terms=elem.double())


def _within_one_ulp(loss, terms):
    got = np.float32(loss.cpu().numpy()[0])
    want = np.float32(float(terms.sum()))
    print("loss {!r}  float64 sum {!r}  as float32 {!r}".format(got, float(terms.sum()), want))
    assert np.isfinite(want) and want != 0
    assert got in (want, np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))), (got, want)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_loss_is_the_sum_of_the_calls_own_values(entry, size):
    case = run_case(entry, size)
    assert case["nb"] == 1 if size == "one" else 256 < case["nb"] <= 264, case["nb"]
    _within_one_ulp(case["loss"], case["terms"])


@pytest.mark.parametrize("size", SIZES)
def test_masked_mse_inside_deferred_reductions(size):
    """the deferred branch: the final sum runs as a segment of the queued launch, the same bits as on its own"""
    alone = run_case("masked_mse", size)
    with ops.deferred_reductions():
        case = run_case("masked_mse", size)
    _within_one_ulp(case["loss"], case["terms"])
    assert torch.equal(case["loss"].cpu().view(torch.int32), alone["loss"].cpu().view(torch.int32))
