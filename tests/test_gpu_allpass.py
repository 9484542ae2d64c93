"""The all-pass warping kernels (csrc/allpass.hip) through ops against the float64 specification
(tests/allpass_spec.py): forward, dx and dalpha for every block size class, block count, lane-tile edge, row pitch and
normalisation.

Tolerance.  The yardstick is the specification's own recursion evaluated in float32 numpy (`dtype=np.float32`: code
of the test, not code under test) on the same inputs; a kernel result may be off the float64 truth by at most 8 times
what the yardstick is off, both as the largest absolute error over the case (relative to the same max|truth|, which
cancels).  The factor covers a different summation order and FMA contraction over at most 64 terms.  One floor under
the yardstick's error: half a unit in the last place of the case's largest value, 2^-24 max|truth| -- any float32
evaluation rounds its result at least once, so a smaller yardstick error (a one-row case where numpy happened to round
every entry exactly) is luck and says nothing about precision.

One reference per (N, normalisation) at 257 rows and 4 blocks serves every case: rows do not mix, and blocks do not
mix in y and dx (the specification returns dalpha per block, summed here over the case's blocks)."""
import functools

import numpy as np
import pytest
import torch

from idiaptts_amd import ops
from tests import allpass_spec as spec

pytestmark = pytest.mark.gpu

M_MAX, NB_MAX = 257, 4
ROWS = (1, 63, 64, 65, 257)          # the 64-row lane tile: one row, one short of a tile, a tile, one more, five tiles


@functools.lru_cache(maxsize=None)
def reference(N, norm):
    """inputs (float32) and, for float64 and float32, (y, dx, dalpha per block) -- read-only"""
    rng = np.random.default_rng(1000 * N + norm)
    D = NB_MAX * N
    x = rng.normal(size=(M_MAX, D)).astype(np.float32)
    dy = rng.normal(size=(M_MAX, D)).astype(np.float32)
    a = rng.uniform(-0.45, 0.45, M_MAX).astype(np.float32)
    a[[0, 65]], a[[1, 256]], a[[2, 64]] = 0.45, -0.45, 0.0      # both ends and exact 0, in every row count >= 3
    mean = rng.normal(size=D).astype(np.float32) if norm else None
    sd = rng.uniform(0.5, 2.0, D).astype(np.float32) if norm else None
    out = {"x": x, "dy": dy, "a": a, "mean": mean, "sd": sd}
    for dtype in (np.float64, np.float32):
        y = spec.forward(x, a, N, mean, sd, dtype)
        dx, da = spec.backward(dy, x, a, N, mean, sd, dtype)
        out[dtype] = (y, dx, da)
    for v in out.values():
        for arr in (v if isinstance(v, tuple) else (v,)):
            if arr is not None:
                arr.setflags(write=False)
    return out


def pitched(arr, pad, dev, fill=float("nan")):
    """[M, D] view with a row pitch of D + pad of a buffer filled with `fill`, and the buffer"""
    M, D = arr.shape
    buf = torch.full((M, D + pad), fill, dtype=torch.float32, device=dev)
    buf[:, :D] = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    return buf[:, :D], buf


within = spec.within_yardstick


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("nb", [1, 3, 4])
@pytest.mark.parametrize("N", [1, 2, 5, 30, 60, 64])
def test_forward_dx_dalpha_match_the_float64_spec(gpu, N, nb, norm):
    ref = reference(N, norm)
    D = nb * N
    y64, dx64, da64 = ref[np.float64]
    y32, dx32, da32 = ref[np.float32]
    mean = torch.from_numpy(ref["mean"][:D].copy()).to(gpu) if norm else None
    sd = torch.from_numpy(ref["sd"][:D].copy()).to(gpu) if norm else None
    for M in ROWS:
        a = torch.from_numpy(ref["a"][:M].copy()).to(gpu)
        for pad in (0, 3):
            where = "N={} nb={} M={} pad={} norm={}".format(N, nb, M, pad, norm)
            x, xbuf = pitched(ref["x"][:M, :D], pad, gpu)
            dy, _ = pitched(ref["dy"][:M, :D], pad, gpu)
            out, obuf = pitched(np.zeros((M, D), np.float32), pad, gpu, fill=-7.0)
            before = xbuf.clone()
            y = ops.allpass_warp_fwd(x, a, N, mean, sd, out=out)
            dx, da = ops.allpass_warp_bwd(dy, x, a, N, mean, sd)
            torch.cuda.synchronize()
            assert y.data_ptr() == out.data_ptr()
            assert (obuf[:, D:] == -7.0).all(), where + ": wrote between the rows"
            assert torch.equal(xbuf[:, :D], before[:, :D]), where + ": x was modified"
            assert dx.shape == (M, D) and da.shape == (M,)
            within("y", y.cpu().numpy(), y64[:M, :D], y32[:M, :D], where)
            within("dx", dx.cpu().numpy(), dx64[:M, :D], dx32[:M, :D], where)
            within("dalpha", da.cpu().numpy(), da64[:M, :nb].sum(axis=1),
                   da32[:M, :nb].sum(axis=1, dtype=np.float32), where)


@pytest.mark.parametrize("N,nb", [(1, 2), (5, 4), (30, 1), (60, 3), (64, 5)])
def test_zero_alpha_returns_the_input_bit_for_bit(gpu, N, nb):
    x = torch.randn(130, nb * N, device=gpu)
    y = ops.allpass_warp_fwd(x, torch.zeros(130, device=gpu), N)
    assert torch.equal(y, x)


def test_repeated_calls_are_bit_identical_and_leave_x_alone(gpu):
    ref = reference(60, True)
    D = 180
    x = torch.from_numpy(ref["x"][:, :D].copy()).to(gpu)
    dy = torch.from_numpy(ref["dy"][:, :D].copy()).to(gpu)
    a = torch.from_numpy(ref["a"].copy()).to(gpu)
    mean, sd = (torch.from_numpy(ref[k][:D].copy()).to(gpu) for k in ("mean", "sd"))
    keep = x.clone()
    first = (ops.allpass_warp_fwd(x, a, 60, mean, sd),) + ops.allpass_warp_bwd(dy, x, a, 60, mean, sd)
    again = (ops.allpass_warp_fwd(x, a, 60, mean, sd),) + ops.allpass_warp_bwd(dy, x, a, 60, mean, sd)
    for u, v in zip(first, again):
        assert torch.equal(u, v)
    assert torch.equal(x, keep)


def test_size_60_is_finite_where_the_float32_table_is_not(gpu):
    """the reference's float32 coefficient table holds infinities at N = 60 (tests/test_allpass_spec.py) and its
    outputs are NaN; the kernel's are finite and right for every |alpha| up to 0.7"""
    M, N = 141, 60
    rng = np.random.default_rng(60)
    x = rng.normal(size=(M, 3 * N)).astype(np.float32)
    a = np.linspace(-0.7, 0.7, M).astype(np.float32)
    y = ops.allpass_warp_fwd(torch.from_numpy(x).to(gpu), torch.from_numpy(a).to(gpu), N).cpu().numpy()
    assert np.isfinite(y).all()
    within("y", y, spec.forward(x, a, N), spec.forward(x, a, N, dtype=np.float32), "N=60 |alpha|<=0.7")


def test_more_blocks_than_one_sweep_carries(gpu):
    """7 blocks: three sweeps of 3 + 3 + 1 blocks, dalpha summed over all of them by the row's lane"""
    M, N, nb = 70, 6, 7
    rng = np.random.default_rng(7)
    x, dy = (rng.normal(size=(M, nb * N)).astype(np.float32) for _ in range(2))
    a = rng.uniform(-0.45, 0.45, M).astype(np.float32)
    xg, dyg, ag = (torch.from_numpy(v).to(gpu) for v in (x, dy, a))
    y = ops.allpass_warp_fwd(xg, ag, N).cpu().numpy()
    dx, da = (t.cpu().numpy() for t in ops.allpass_warp_bwd(dyg, xg, ag, N))
    dx64, da64 = spec.backward(dy, x, a, N)
    dx32, da32 = spec.backward(dy, x, a, N, dtype=np.float32)
    within("y", y, spec.forward(x, a, N), spec.forward(x, a, N, dtype=np.float32), "nb=7")
    within("dx", dx, dx64, dx32, "nb=7")
    within("dalpha", da, da64.sum(axis=1), da32.sum(axis=1, dtype=np.float32), "nb=7")
