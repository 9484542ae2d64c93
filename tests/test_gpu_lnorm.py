"""The LayerNorm row kernels (csrc/layernorm.hip) through ops and the C ABI against the float64 restatement of
lnorm_cases.py (pinned to torch in float64 by tests/test_lnorm_config.py): every width class and its edges, one row to
several slabs, pitched and misaligned rows with sentinels around the output, absent gamma / beta / dgamma / dbeta, both
eps, four activations, the ill-conditioned rows, and bit-for-bit determinism across calls, batch sizes and load forms."""
import pytest
import torch

from lnorm_cases import (HAZARDS, N_SLABS, SWEEP, check, hazard_inputs, reference64, sweep_inputs,
                         torch32 as torch_float32)
from idiaptts_amd import lib, ops

pytestmark = pytest.mark.gpu

# options of a run: (gamma, beta, eps, activation, want dgamma, want dbeta)
OPTIONS = [(True, True, 1e-5, None, True, True), (False, False, 1e-3, "ReLU", False, False),
           (True, False, 1e-5, "Tanh", True, False), (True, True, 1e-3, "ELU", False, True)]


def _run(gpu, x, gamma, beta, dy, eps, act_name, want_gamma=True, want_beta=True):
    """forward and backward through ops on device copies: dict of y, mean, rstd, dx, dgamma, dbeta (CPU)"""
    act = ops.ACT_BY_NAME[act_name.lower()] if act_name else ops.ACT_NONE
    dev = [t.to(gpu) if t is not None else None for t in (x, gamma, beta, dy)]
    y, mean, rstd = ops.layer_norm_fwd(dev[0], dev[1], dev[2], eps, act)
    dx, dgamma, dbeta = ops.layer_norm_bwd(dev[3], dev[0], mean, rstd, dev[1], y=y, act=act,
                                           want_gamma=want_gamma, want_beta=want_beta)
    out = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)
    return {k: v.cpu() if v is not None else None for k, v in out.items()}


@pytest.mark.parametrize("N,D", SWEEP)
def test_shape_sweep_against_float64(gpu, N, D):
    x, gamma, beta, dy = sweep_inputs(torch, N, D)
    for has_gamma, has_beta, eps, act, want_gamma, want_beta in OPTIONS:
        ga, be = gamma if has_gamma else None, beta if has_beta else None
        ref = reference64(torch, x, ga, be, dy, eps, act)
        got = _run(gpu, x, ga, be, dy, eps, act, want_gamma, want_beta)
        for product in ("y", "dx"):
            check(product, got[product], ref[product])
        assert (got["mean"].double() - ref["mean"]).abs().max() < 2e-6 * max(1.0, ref["mean"].abs().max().item())
        assert ((got["rstd"].double() - ref["rstd"]).abs() / ref["rstd"]).max() < 2e-6
        for product, wanted in (("dgamma", want_gamma), ("dbeta", want_beta)):
            if wanted:
                check(product, got[product], ref[product])
            else:
                assert got[product] is None


def test_slab_count_of_the_column_sums():
    L = lib.load()
    assert N_SLABS == 2 * 32 + 5                     # two full slabs of 32 rows and a partial one
    for D in (67, 256, 4096):
        assert L.itts_layernorm_workspace_bytes(N_SLABS, D) == 3 * 2 * D * 4
    assert L.itts_layernorm_workspace_bytes(4400, 67) == 138 * 2 * 67 * 4


@pytest.mark.parametrize("name", HAZARDS)
def test_ill_conditioned_rows(gpu, name):
    """D = 1, D = 3, rows of variance 0 and a row offset of 1e4 (which E[x^2] - mean^2 does not survive): the bound
    is the larger of the dense one and twice the error of torch's own float32 layer_norm on the same data"""
    x, gamma, beta, dy, eps = hazard_inputs(torch, name)
    for act in (None, "Tanh"):
        ref = reference64(torch, x, gamma, beta, dy, eps, act)
        t32 = torch_float32(torch, x, gamma, beta, dy, eps, act)
        got = _run(gpu, x, gamma, beta, dy, eps, act)
        for product in ("y", "dx", "dgamma", "dbeta"):
            assert torch.isfinite(got[product]).all()
            check(product, got[product], ref[product], case=name, torch32=t32[product])
    got = _run(gpu, x, gamma, beta, dy, eps, None)
    if name == "constant_row":
        assert torch.equal(got["y"][2], beta)        # variance exactly 0: the output is beta
        assert (got["y"][4] - beta).abs().max() < 2e-5 * max(1.0, beta.abs().max().item())
        assert got["rstd"][2].item() == pytest.approx(1e-5 ** -0.5, rel=1e-6)
    if name == "D1":
        assert torch.equal(got["y"], beta.expand(x.shape[0], 1)) and not got["dx"].any()


def test_only_the_named_cases_may_relax_the_bound():
    x = torch.zeros(2, 16, dtype=torch.float64)
    with pytest.raises(AssertionError, match="only the named"):
        check("y", x, x, case="sweep", torch32=x)
    with pytest.raises(AssertionError, match="only the named"):
        check("y", x, x, torch32=x)


def _wide(gpu, t, width, c0, fill):
    """t as the column slice [c0, c0 + D) of a [N, width] device tensor filled with `fill` elsewhere"""
    full = torch.full((t.shape[0], width), fill, dtype=torch.float32, device=gpu)
    full[:, c0:c0 + t.shape[1]] = t.to(gpu)
    return full, full[:, c0:c0 + t.shape[1]]


@pytest.mark.parametrize("D,width,c0", [(67, 72, 4), (67, 71, 1), (64, 80, 8), (64, 80, 3), (257, 300, 0), (1025, 1031, 5)])
@pytest.mark.parametrize("act_name", [None, "ELU"])
def test_pitched_and_misaligned_rows(gpu, D, width, c0, act_name):
    """operands and results as column slices of wider tensors -- a pitch above D on a 16-byte aligned base (16-byte
    loads) and a base 4 .. 12 bytes off (plain loads): the same bits as contiguous rows, 1e30 in the pad columns of
    x, dy and y changes nothing, and no element around the written slices changes"""
    N = 37
    x, gamma, beta, dy = sweep_inputs(torch, N, D, seed=1)
    act = ops.ACT_BY_NAME[act_name.lower()] if act_name else ops.ACT_NONE
    base = _run(gpu, x, gamma, beta, dy, 1e-5, act_name)
    _, xs = _wide(gpu, x, width, c0, 1e30)
    _, dys = _wide(gpu, dy, width, c0, 1e30)
    y_full, ys = _wide(gpu, torch.zeros(N, D), width, c0, 1e30)
    dx_full, dxs = _wide(gpu, torch.zeros(N, D), width, c0, -7.25)
    if c0 % 4:
        assert xs.data_ptr() % 16 != 0
    else:
        assert xs.data_ptr() % 16 == 0
    y, mean, rstd = ops.layer_norm_fwd(xs, gamma.to(gpu), beta.to(gpu), 1e-5, act, out=ys)
    dx, dgamma, dbeta = ops.layer_norm_bwd(dys, xs, mean, rstd, gamma.to(gpu), y=ys, act=act, dx=dxs)
    assert y.data_ptr() == ys.data_ptr() and dx.data_ptr() == dxs.data_ptr()
    for k, v in (("y", y), ("mean", mean), ("rstd", rstd), ("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        assert torch.equal(v.cpu(), base[k]), k
    for full, fill in ((y_full, 1e30), (dx_full, -7.25)):
        outside = torch.ones(width, dtype=torch.bool)
        outside[c0:c0 + D] = False
        assert torch.equal(full.cpu()[:, outside], torch.full((N, width - D), fill))


def test_same_bits_again_and_anywhere_in_a_batch(gpu):
    """repeated calls give identical bits for every output (no atomics); a row gives identical y and dx bits alone
    (N = 1) and as row 4 321 of a large batch"""
    for D in (67, 1024):
        N, row = 4400, 4321
        x, gamma, beta, dy = sweep_inputs(torch, N, D, seed=2)
        for act in (None, "Tanh"):
            a = _run(gpu, x, gamma, beta, dy, 1e-5, act)
            b = _run(gpu, x, gamma, beta, dy, 1e-5, act)
            for k in a:
                assert torch.equal(a[k], b[k]), (D, act, k)
            one = _run(gpu, x[row:row + 1], gamma, beta, dy[row:row + 1], 1e-5, act)
            for k in ("y", "dx", "mean", "rstd"):
                assert torch.equal(one[k][0], a[k][row]), (D, act, k)
            ref = reference64(torch, x, gamma, beta, dy, 1e-5, act)
            for product in ("dgamma", "dbeta"):
                check(product, a[product], ref[product])


def test_no_rows(gpu):
    for D in (1, 67):
        x = torch.empty(0, D, device=gpu)
        gamma, beta = torch.ones(D, device=gpu), torch.zeros(D, device=gpu)
        y, mean, rstd = ops.layer_norm_fwd(x, gamma, beta)
        assert y.shape == (0, D) and mean.shape == (0,) and rstd.shape == (0,)
        dx, dgamma, dbeta = ops.layer_norm_bwd(x, x, mean, rstd, gamma)
        assert dx.shape == (0, D) and not dgamma.any() and not dbeta.any()


def test_arguments_are_checked(gpu):
    x = torch.zeros(4, 4097, device=gpu)
    with pytest.raises(lib.IttsError, match="4097"):
        ops.layer_norm_fwd(x, None, None)
    x = torch.zeros(4, 8, device=gpu)
    with pytest.raises(lib.IttsError, match="unknown activation"):
        ops.layer_norm_fwd(x, None, None, act=ops.ACT_HARDSIGMOID + 1)
    with pytest.raises(ValueError, match="needs the forward's output"):
        ops.layer_norm_bwd(x, x, x[:, 0], x[:, 0], None, act=ops.ACT_TANH)
    with pytest.raises(lib.IttsError, match="no CPU fallback"):
        ops.layer_norm_fwd(x.cpu(), None, None)
