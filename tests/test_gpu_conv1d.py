"""itts_conv1d_fwd / _bwd_input / _bwd_weight (csrc/conv1d.hip) against torch's conv1d in float64 on the CPU: the
Conv1d groups of rnn_dyn/CNNWrapper.py.  Tolerances of the dense-layer tests (test_gpu_nn.py): relative error
||got - ref|| / ||ref|| < 2e-6 (3e-6 for the weight and bias gradients, sums over B * T_out rows), and on every
element |got - ref| <= 2e-5 * max(1, max|ref|).

The small shapes below (SHAPES, the strided / module / activation cases) all take the 64-wide tile with one slab.
The code that runs at production sizes -- the 128-wide tile, weight gradients summed over many slabs, a short last
slab, fewer slabs than the workspace was sized for, the non-vector loads at such sizes -- is compared under CASES
(tests/conv_harness.py) against tests/conv_ref.py (float64 im2col + matrix products on the GPU, pinned to torch on
the CPU by test_conv_ref.py) with the same bounds; every case asserts the plan ops.conv1d_plan names for it, so a change of the
dispatch rule fails here instead of quietly testing other code."""
import collections

import numpy as np
import pytest
import torch

from conv_harness import CASES, expected_vec, run_case
from conv_ref import SHAPES, conv_ref, same_pad
from idiaptts_amd import ops

pytestmark = pytest.mark.gpu

ACTS = {"none": ops.ACT_NONE, "tanh": ops.ACT_TANH, "relu": ops.ACT_RELU}


def _ref_fwd(x, w, b, pad, dil, bf, act):
    """x [B, T, C] / [T, B, C] -> torch.conv1d in float64 on the CPU, same layout"""
    xc = x.double().cpu()
    xc = xc.permute(0, 2, 1) if bf else xc.permute(1, 2, 0)
    y = torch.nn.functional.conv1d(xc, w.double().cpu(), None if b is None else b.double().cpu(), padding=pad,
                                   dilation=dil)
    if act == "tanh":
        y = torch.tanh(y)
    elif act == "relu":
        y = torch.relu(y)
    return y.permute(0, 2, 1) if bf else y.permute(2, 0, 1)


WORST = collections.defaultdict(float)   # product -> worst error of the CASES as a fraction of its tolerance


def _check(got, ref, K, what, rel=2e-6, key=None):
    got = got.double().to(ref.device)
    err = float((got - ref).norm()) / (float(ref.norm()) + 1e-30)
    amax = float((got - ref).abs().max())
    tol = 2e-5 * max(1.0, float(ref.abs().max()))
    if key is not None:
        WORST[key] = max(WORST[key], err / rel, amax / tol)
        print("{}: relative error {:.3g} (bound {:g}), max abs error {:.3g} (bound {:.3g})".format(what, err, rel, amax,
                                                                                                 tol))
    assert err < rel, "{}: relative error {:.3g}".format(what, err)
    assert amax <= tol, "{}: max abs error {:.3g}".format(what, amax)


def _make(gpu, B, T, Cin, Cout, Kw, bf, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T, Cin) if bf else (T, B, Cin), generator=g)
    w = torch.randn((Cout, Cin, Kw), generator=g) / (Cin * Kw) ** 0.5
    b = torch.randn((Cout,), generator=g) if bias else None
    return x.to(gpu), w.to(gpu), (b.to(gpu) if bias else None)


def _grads_ref(x, w, b, pad, dil, bf, dy):
    xr = x.double().cpu().requires_grad_(True)
    wr = w.double().cpu().requires_grad_(True)
    br = None if b is None else b.double().cpu().requires_grad_(True)
    y = _ref_fwd(xr, wr, br, pad, dil, bf, "none")
    y.backward(dy.double().cpu())
    return xr.grad, wr.grad, (None if br is None else br.grad)


_pad = same_pad


@pytest.mark.parametrize("bf", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_gradients(gpu, shape, bf):
    B, T, Cin, Cout, Kw, dil, pad = shape
    pad = _pad(pad, Kw, dil)
    x, w, b = _make(gpu, B, T, Cin, Cout, Kw, bf, seed=SHAPES.index(shape))
    y = ops.conv1d_fwd(x, w, b, pad, dil, bf)
    ref = _ref_fwd(x, w, b, pad, dil, bf, "none")
    assert y.shape == ref.shape
    _check(y, ref, Kw * Cin, "forward")
    dy = torch.randn(y.shape, device=gpu)
    gx, gw, gb = _grads_ref(x, w, b, pad, dil, bf, dy)
    dx = ops.conv1d_bwd_input(dy, w, T, pad, dil, bf)
    _check(dx, gx, Kw * Cout, "input gradient")
    dw, db = ops.conv1d_bwd_weight(dy, x, Kw, pad, dil, bf)
    T_out = y.shape[1 if bf else 0]
    _check(dw, gw, B * T_out, "weight gradient", rel=3e-6)
    _check(db, gb, B * T_out, "bias gradient", rel=3e-6)
    # accumulate adds to what is there
    dw2, db2 = ops.conv1d_bwd_weight(dy, x, Kw, pad, dil, bf, dw=dw.clone(), db=db.clone(), accumulate=True)
    _check(dw2, 2 * gw, B * T_out, "accumulated weight gradient", rel=3e-6)
    _check(db2, 2 * gb, B * T_out, "accumulated bias gradient", rel=3e-6)


@pytest.mark.parametrize("act", ["none", "tanh", "relu"])
@pytest.mark.parametrize("bias", [True, False])
def test_activation_and_bias_none(gpu, act, bias):
    x, w, b = _make(gpu, 3, 21, 409, 16, 3, True, seed=5, bias=bias)
    y = ops.conv1d_fwd(x, w, b, 1, 1, True, ACTS[act])
    _check(y, _ref_fwd(x, w, b, 1, 1, True, act), 3 * 409, "forward " + act)


@pytest.mark.parametrize("act_prev", ["tanh", "relu"])
@pytest.mark.parametrize("bf", [True, False])
def test_input_gradient_fused_act_prev(gpu, act_prev, bf):
    B, T, Cin, Cout, Kw, dil, pad = 3, 26, 20, 24, 5, 2, 4
    x, w, b = _make(gpu, B, T, Cin, Cout, Kw, bf, seed=8)
    yprev = torch.tanh(x) if act_prev == "tanh" else torch.relu(x)
    dz = torch.randn(ops.conv1d_fwd(x, w, b, pad, dil, bf).shape, device=gpu)
    gx, _, _ = _grads_ref(x, w, b, pad, dil, bf, dz)
    deriv = (1 - yprev.double().cpu() ** 2) if act_prev == "tanh" else (yprev.double().cpu() > 0).double()
    dx = ops.conv1d_bwd_input(dz, w, T, pad, dil, bf, yprev=yprev, act_prev=ACTS[act_prev])
    _check(dx, gx * deriv, Kw * Cout, "fused input gradient")


def test_nonpositive_output_length_raises(gpu):
    x, w, b = _make(gpu, 2, 4, 3, 5, 5, True, seed=1)
    with pytest.raises(ValueError):
        ops.conv1d_fwd(x, w, b, 0, 1, True)
    with pytest.raises(ValueError):
        ops.conv1d_bwd_weight(torch.zeros(2, 1, 5, device=gpu), x, 5, 0, 2, True)
    with pytest.raises(ValueError):
        ops.conv1d_bwd_input(torch.zeros(2, 1, 5, device=gpu), w, 4, 0, 1, True)


def test_repeated_calls_are_bit_identical(gpu):
    """(8 x 300, 512 -> 512, k5: the weight gradient sums 6 slabs on the 128-wide tile) three runs agree bit for bit,
    and the values are those of the float64 restatement"""
    x, w, b = _make(gpu, 8, 300, 512, 512, 5, True, seed=3)
    dy = torch.randn(8, 300, 512, device=gpu)
    assert ops.conv1d_plan(ops.CONV_BWD_WEIGHT, 8, 300, 512, 512, 5, 2, 1) == (128, 6, 416)
    outs = []
    for _ in range(3):
        y = ops.conv1d_fwd(x, w, b, 2, 1, True, ops.ACT_TANH)
        dx = ops.conv1d_bwd_input(dy, w, 300, 2, 1, True)
        dw, db = ops.conv1d_bwd_weight(dy, x, 5, 2, 1, True)
        outs.append([t.cpu().numpy() for t in (y, dx, dw, db)])
    for o in outs[1:]:
        for a, r in zip(o, outs[0]):
            assert np.array_equal(a, r)
    ry, rdx, rdw, rdb = conv_ref(x, w, b, 2, 1, True, act="tanh", dz=dy)
    _check(y, ry, 5 * 512, "forward")
    _check(dx, rdx, 5 * 512, "input gradient")
    _check(dw, rdw, 8 * 300, "weight gradient", rel=3e-6)
    _check(db, rdb, 8 * 300, "bias gradient", rel=3e-6)


@pytest.mark.parametrize("bf", [True, False])
def test_strided_rows(gpu, bf):
    """x and dz as column slices of wider buffers (row pitch > channels, 16-byte and odd pitches)"""
    B, T, Cin, Cout, Kw = 3, 19, 409, 67, 3
    for pitch_in, pitch_out in ((412, 68), (415, 70)):
        xs, w, b = _make(gpu, B, T, pitch_in, Cout, Kw, bf, seed=pitch_in)
        x = xs[..., :Cin]
        w = w[:, :Cin].contiguous()
        y = ops.conv1d_fwd(x, w, b, 1, 1, bf)
        _check(y, _ref_fwd(x, w, b, 1, 1, bf, "none"), Kw * Cin, "strided forward")
        dys = torch.randn(y.shape[:2] + (pitch_out,), device=gpu)
        dy = dys[..., :Cout]
        gx, gw, gb = _grads_ref(x, w, b, 1, 1, bf, dy)
        _check(ops.conv1d_bwd_input(dy, w, T, 1, 1, bf), gx, Kw * Cout, "strided input gradient")
        dw, db = ops.conv1d_bwd_weight(dy, x, Kw, 1, 1, bf)
        _check(dw, gw, B * T, "strided weight gradient", rel=3e-6)
        _check(db, gb, B * T, "strided bias gradient", rel=3e-6)


def test_autograd_module_matches_torch(gpu):
    from idiaptts_amd.nn.modules import Conv1dAct
    torch.manual_seed(0)
    ref = torch.nn.Conv1d(30, 18, 5, padding=3, dilation=2)
    torch.manual_seed(0)
    mod = Conv1dAct(30, 18, 5, padding=3, dilation=2, act="tanh", batch_first=False).to(gpu)
    assert torch.equal(mod.weight.cpu(), ref.weight) and torch.equal(mod.bias.cpu(), ref.bias)
    x = torch.randn(23, 4, 30, device=gpu, requires_grad=True)
    y = mod(x)
    xr = x.detach().double().cpu().requires_grad_(True)
    yr = torch.tanh(torch.nn.functional.conv1d(xr.permute(1, 2, 0), ref.weight.double(), ref.bias.double(),
                                               padding=3, dilation=2)).permute(2, 0, 1)
    _check(y, yr, 150, "module forward")
    g = torch.randn(y.shape, device=gpu)
    y.backward(g)
    wr = ref.weight.detach().double().requires_grad_(True)
    br = ref.bias.detach().double().requires_grad_(True)
    xr.grad = None
    yr = torch.tanh(torch.nn.functional.conv1d(xr.permute(1, 2, 0), wr, br, padding=3, dilation=2)).permute(2, 0, 1)
    yr.backward(g.double().cpu())
    _check(x.grad, xr.grad, 90, "module input gradient")
    _check(mod.weight.grad, wr.grad, 4 * 23, "module weight gradient", rel=3e-6)
    _check(mod.bias.grad, br.grad, 4 * 23, "module bias gradient", rel=3e-6)


@pytest.mark.parametrize("act", ["none", "tanh"])
@pytest.mark.parametrize("Cin,Cout", [(64, 128), (67, 45)])
def test_kernel_size_one_is_the_dense_layer(gpu, Cin, Cout, act):
    """Kw = 1, padding 0: the forward and the input gradient are the dense layer's GEMMs with the same K order
    (padded channels add zeros), so they equal itts_linear_fwd / itts_linear_bwd_input bit for bit; 64 channels
    take the dense ring kernel, 67 its register-staged kernel"""
    B, T = 3, 70
    x, w, b = _make(gpu, B, T, Cin, Cout, 1, True, seed=Cin)
    w2 = w[:, :, 0].contiguous()
    y = ops.conv1d_fwd(x, w, b, 0, 1, True, ACTS[act])
    assert torch.equal(y.reshape(B * T, Cout), ops.linear_fwd(x.reshape(B * T, Cin), w2, b, ACTS[act]))
    dz = torch.randn(B, T, Cout, device=gpu)
    yprev = torch.tanh(x) if act == "tanh" else None
    dx = ops.conv1d_bwd_input(dz, w, T, 0, 1, True, yprev=yprev, act_prev=ACTS[act])
    dx2 = ops.linear_bwd_input(dz.reshape(B * T, Cout), w2, None if yprev is None else yprev.reshape(B * T, Cin),
                               ACTS[act])
    assert torch.equal(dx.reshape(B * T, Cin), dx2)


# ------------------------------------------------------------------ the code that runs at production sizes
@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    if WORST:
        print("\nConv1d CASES, worst error as a fraction of its tolerance:",
              {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_production_size_paths(gpu, case):
    """All three products of one CASES entry (tests/conv_harness.py) against conv_ref with the bounds of _check: the
    plan asserted first; outputs written into column slices of sentinel-filled buffers (the columns around them stay
    bit-unchanged); in the pad4 cases whose channels are no multiple of 4 (425, 409, 130, 70: the rows that 16-byte
    loads read beyond their width) 1e30 in the pad floats of x / dz changes no bit of any result; and where the entry
    says so the dense kernels on an explicit im2col pass the same bounds on the same data."""
    g = case.geo
    vec = expected_vec(g)
    for product in range(3):
        assert ops.conv1d_plan(product, g.B, g.T, g.Cin, g.Cout, g.Kw, g.pad, g.dil, vec[product]) \
            == case.plan[product], product
    res = run_case(gpu, g, torch.Generator(device=gpu).manual_seed(CASES.index(case)), case.name)
    for key, got, ref, rel in res.items():
        _check(got, ref, None, key, rel=rel, key=key)
    if case.yardstick:
        for key, got, ref, rel in res.items():
            _check(res.yardstick(key), ref, None, "yardstick " + key, rel=rel, key="yardstick " + key)
