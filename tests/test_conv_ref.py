"""tests/conv_ref.py (the float64 im2col restatement the Conv1d GPU tests and scripts/conv_fuzz.py compare the kernels
with) pinned to torch.nn.functional.conv1d + autograd in float64 on the CPU: y with each activation, dx (plain and
with the previous layer's derivative fused), dw, db, in both layouts, on the 9 small shapes of test_gpu_conv1d.py
plus T_out = 1, Kw = 1 and 1 .. 5 input channels.  Both sides are float64 sums of at most Kw * Cin (or B * T_out)
terms of size O(1), so they agree to |a - b| <= 1e-12 * max(1, max|b|) with orders of margin."""
import pytest
import torch

from conv_ref import SHAPES, conv_ref, same_pad

EXTRA = [   # B, T, Cin, Cout, Kw, dil, pad
    (3, 5, 7, 4, 5, 1, 0),             # T_out = 1
    (2, 9, 6, 3, 3, 4, 0),             # T_out = 1 with dilation
    (2, 11, 9, 8, 1, 3, 2),            # Kw = 1 (padding only widens the output)
] + [(2, 13, c, 6, 3, 2, 1) for c in range(1, 6)]


def _close(a, b, what):
    assert a.shape == b.shape, what
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), "{}: {:.3g}".format(what, err)


def _torch_fwd(x, w, b, pad, dil, bf, act):
    xc = x.permute(0, 2, 1) if bf else x.permute(1, 2, 0)
    z = torch.nn.functional.conv1d(xc, w, b, padding=pad, dilation=dil)
    y = {"none": lambda v: v, "tanh": torch.tanh, "relu": torch.relu}[act](z)
    return (y.permute(0, 2, 1) if bf else y.permute(2, 0, 1)), (z.permute(0, 2, 1) if bf else z.permute(2, 0, 1))


@pytest.mark.parametrize("bf", [True, False])
@pytest.mark.parametrize("shape", SHAPES + EXTRA)
def test_restatement_matches_torch_conv1d_float64(shape, bf):
    B, T, Cin, Cout, Kw, dil, pad = shape
    pad = same_pad(pad, Kw, dil)
    g = torch.Generator().manual_seed(2 * (SHAPES + EXTRA).index(shape) + bf)
    x = torch.randn((B, T, Cin) if bf else (T, B, Cin), generator=g, dtype=torch.float64)
    w = torch.randn((Cout, Cin, Kw), generator=g, dtype=torch.float64) / (Cin * Kw) ** 0.5
    b = torch.randn((Cout,), generator=g, dtype=torch.float64)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    _, z = _torch_fwd(xr, wr, br, pad, dil, bf, "none")
    dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    z.backward(dz)
    for chunk in (1 << 27, 1):          # whole batch at once, and one utterance per chunk
        y, dx, dw, db = conv_ref(x, w, b, pad, dil, bf, dz=dz, chunk_bytes=chunk)
        _close(y, z.detach(), "y")
        _close(dx, xr.grad, "dx")
        _close(dw, wr.grad, "dw")
        _close(db, br.grad, "db")
    for act in ("tanh", "relu"):
        _close(conv_ref(x, w, b, pad, dil, bf, act=act)[0], _torch_fwd(x, w, b, pad, dil, bf, act)[0], "y " + act)
        # the previous layer's activation: x = act(u), so d/du = dx * act'(x) through its output
        u = torch.randn(x.shape, generator=g, dtype=torch.float64).requires_grad_(True)
        yprev = torch.tanh(u) if act == "tanh" else torch.relu(u)
        _torch_fwd(yprev, w, b, pad, dil, bf, "none")[1].backward(dz)
        _, du, dw2, _ = conv_ref(yprev.detach(), w, b, pad, dil, bf, dz=dz, yprev=yprev.detach(), act_prev=act)
        _close(du, u.grad, "dx through " + act)
    # no bias
    _close(conv_ref(x, w, None, pad, dil, bf)[0], _torch_fwd(x, w, None, pad, dil, bf, "none")[0], "y without bias")


def test_shapes_reach_the_edges_named():
    from conv_ref import out_len
    assert [out_len(s[1], s[4], same_pad(s[6], s[4], s[5]), s[5]) for s in EXTRA[:2]] == [1, 1]
    assert EXTRA[2][4] == 1 and sorted(s[2] for s in EXTRA[3:]) == [1, 2, 3, 4, 5]
    assert len(SHAPES) == 9
