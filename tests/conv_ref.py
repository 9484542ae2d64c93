"""A plain float64 restatement of the three Conv1d products (csrc/conv1d.hip) that scales to the production sizes:
an explicit im2col (zero outside [0, T_in) of each utterance) and three matrix products,

    z  = x_col W^T + b,  y = act(z)              x_col [B * T_out, Kw * Cin],  W[n][k * Cin + c] = w[n][c][k]
    dx = col2im(dz W) (* act_prev'(yprev))       dz is the gradient at z, as the kernels take it
    dw = dz^T x_col,  db = colsum(dz)

on whatever device the operands are on (float64 matrix products only: no convolution primitive of any library), over
chunks of utterances so that the im2col of a 32 x 1600 x 512 x 5 batch (1 GB in float64) is never held whole.
tests/test_conv_ref.py pins it to torch.nn.functional.conv1d + autograd in float64 on the CPU.  Stride 1, groups 1,
any padding / dilation with T_out = T_in + 2 pad - dil (Kw - 1) > 0; activations [B, T, C] (batch_first) or
[T, B, C]."""
import torch

SHAPES = [   # B, T, Cin, Cout, Kw, dil, pad ("same" = dil * (Kw - 1) // 2): the small shapes of test_gpu_conv1d.py
    (3, 37, 409, 16, 3, 1, "same"),
    (2, 29, 67, 67, 5, 2, "same"),
    (1, 50, 1, 5, 1, 1, 0),
    (2, 64, 512, 512, 5, 1, "same"),
    (3, 45, 13, 7, 31, 1, "same"),
    (2, 20, 6, 9, 3, 4, 0),
    (2, 9, 10, 11, 5, 2, 12),          # padding wider than the kernel span
    (1, 3, 5, 6, 5, 1, 2),             # T shorter than the kernel span
    (4, 17, 33, 65, 3, 4, "same"),
]

CHUNK_BYTES = 128 << 20     # of im2col held at a time


def same_pad(p, Kw, dil):
    return dil * (Kw - 1) // 2 if p == "same" else p


def out_len(T_in, Kw, pad, dil):
    return T_in + 2 * pad - dil * (Kw - 1)


def _taps(T_in, T_out, Kw, shift0, dil):
    """per tap k: (k, t_lo, t_hi, ti_lo) with output steps t_lo .. t_hi - 1 reading input steps ti_lo .. inside
    [0, T_in): input time = t + k * dil + shift0"""
    for k in range(Kw):
        s = k * dil + shift0
        t_lo, t_hi = max(0, -s), min(T_out, T_in - s)
        if t_lo < t_hi:
            yield k, t_lo, t_hi, t_lo + s


def im2col(x, Kw, shift0, dil, T_out):
    """x [b, T_in, C] (batch first, any dtype) -> [b, T_out, Kw * C] tap-major: element (t, k * C + c) is
    x[t + k * dil + shift0, c], zero outside [0, T_in) (shift0 = -pad for the forward)"""
    b, T_in, C = x.shape
    col = x.new_zeros((b, T_out, Kw, C))
    for k, t_lo, t_hi, ti in _taps(T_in, T_out, Kw, shift0, dil):
        col[:, t_lo:t_hi, k] = x[:, ti:ti + t_hi - t_lo]
    return col.reshape(b, T_out, Kw * C)


def col2im(dcol, T_in, Kw, shift0, dil):
    """the transpose of im2col: dcol [b, T_out, Kw * C] -> [b, T_in, C]"""
    b, T_out = dcol.shape[:2]
    dcol = dcol.reshape(b, T_out, Kw, -1)
    dx = dcol.new_zeros((b, T_in, dcol.shape[3]))
    for k, t_lo, t_hi, ti in _taps(T_in, T_out, Kw, shift0, dil):
        dx[:, ti:ti + t_hi - t_lo] += dcol[:, t_lo:t_hi, k]
    return dx


def weight_matrix(w):
    """w [Cout, Cin, Kw] -> W [Cout, Kw * Cin], W[n][k * Cin + c] = w[n][c][k]"""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1)


def _act(z, act):
    return {"none": lambda v: v, "tanh": torch.tanh, "relu": torch.relu}[act](z)


def _act_grad(y, act):
    return {"tanh": lambda v: 1 - v * v, "relu": lambda v: (v > 0).to(v.dtype)}[act](y)


def conv_ref(x, w, b, pad, dil, batch_first, act="none", dz=None, yprev=None, act_prev="none",
             chunk_bytes=CHUNK_BYTES):
    """float64 (y, dx, dw, db) in the layout of x; dx, dw, db are None without dz.  dz is the
    gradient at the pre-activation z; with yprev (shaped as x) dx is multiplied by act_prev'(yprev)."""
    Cout, Cin, Kw = w.shape
    xb = x if batch_first else x.permute(1, 0, 2)
    B, T_in = xb.shape[:2]
    T_out = out_len(T_in, Kw, pad, dil)
    assert T_out > 0 and xb.shape[2] == Cin
    W = weight_matrix(w.double())
    bd = None if b is None else b.double()
    y = torch.empty((B, T_out, Cout), dtype=torch.float64, device=x.device)
    dx = dw = db = None
    if dz is not None:
        dzb = dz if batch_first else dz.permute(1, 0, 2)
        assert tuple(dzb.shape) == (B, T_out, Cout)
        dx = torch.empty((B, T_in, Cin), dtype=torch.float64, device=x.device)
        dw = torch.zeros((Cout, Kw * Cin), dtype=torch.float64, device=x.device)
        db = torch.zeros((Cout,), dtype=torch.float64, device=x.device)
    step = max(1, chunk_bytes // (8 * T_out * Kw * Cin))
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        col = im2col(xb[sl].double(), Kw, -pad, dil, T_out)
        z = col @ W.t()
        if bd is not None:
            z = z + bd
        y[sl] = _act(z, act)
        if dz is not None:
            d = dzb[sl].double()
            dx[sl] = col2im(d @ W, T_in, Kw, -pad, dil)
            dw += d.reshape(-1, Cout).t() @ col.reshape(-1, Kw * Cin)
            db += d.sum(dim=(0, 1))
    if dz is not None:
        if yprev is not None:
            yp = yprev if batch_first else yprev.permute(1, 0, 2)
            dx = dx * _act_grad(yp.double(), act_prev)
        dw = dw.reshape(Cout, Kw, Cin).permute(0, 2, 1).contiguous()
    if not batch_first:
        y = y.permute(1, 0, 2)
        dx = None if dx is None else dx.permute(1, 0, 2)
    return y, dx, dw, db
