"""torch.autograd glue for the HIP acoustic-model kernels (PyTorch-ROCm only provides autograd,
device memory and streams; every forward / backward computation below is a C-ABI call)."""
import collections
import ctypes
import threading

import torch

from .. import lib as _lib
from .. import ops


# The gradient a scalar loss's backward starts from, as an object the loss functions can recognise: `loss.backward()`
# makes a fresh tensor of ones per call, and a Function's backward cannot tell ones from any other factor without
# reading the value back, so it multiplies its stored gradient by it -- a pass over [frames x features] for a factor
# of 1.  The training loop starts backward from `unit_gradient(loss)` instead; autograd hands that very tensor to
# the root's backward, which then skips the product (x * 1.0 is x).
_unit_gradients = {}


def unit_gradient(like):
    key = (like.device, like.dtype)
    unit = _unit_gradients.get(key)
    if unit is None:
        unit = _unit_gradients[key] = torch.ones((), dtype=like.dtype, device=like.device)
    return unit


def is_unit_gradient(grad):
    unit = _unit_gradients.get((grad.device, grad.dtype))
    return unit is not None and grad.dim() == 0 and grad.data_ptr() == unit.data_ptr()


class LinearActFunction(torch.autograd.Function):
    """y = act(x W^T + b) on rows (any leading shape); rnn_dyn/FFWrapper.py:63-73.
    An input whose last extent is `in_features` rounded up to a multiple of four (and not `in_features` itself:
    425 -> 428) is taken as rows with ZEROED pad columns (ValidRows.pack writes them): the weight gets the same zero
    columns for the products, so every operand has a 16-byte row pitch and the GEMM entry points take their LDS-DMA
    kernels -- the register-staged ones took 201 instead of 110 us for the first layer of the 425-512-512-187 model
    and 179 instead of 125 for its weight gradient.  The zeros add nothing to any sum: the same bits."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        N, K = weight.shape
        w = weight.contiguous()
        ctx.k_pad = 0
        if shape[-1] != K and shape[-1] == (K + 3) // 4 * 4:
            ctx.k_pad = shape[-1] - K
            w = torch.nn.functional.pad(w, (0, ctx.k_pad))
        # an output width that is no multiple of four floats (187: the acoustic features) gets rows of a
        # 16-byte multiple (the result is a view of them): the GEMM entry points then take their LDS-DMA
        # kernel instead of the register-staged one -- 0.7 + 0.6 ms per BiLSTM training step otherwise
        out = None
        if N % 4:
            full = torch.empty((x2.shape[0], (N + 3) // 4 * 4), dtype=torch.float32, device=x2.device)
            full[:, N:] = 0          # pad columns: read again by act_bwd over the whole rows
            out = full[:, :N]
        y = ops.linear_fwd(x2, w, bias, act, out=out)
        ctx.save_for_backward(x2, w, y)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.in_shape = shape
        # (callers get contiguous rows, as from torch's own linear: a `.view` on the result must keep working)
        return (y if out is None else y.contiguous()).reshape(*shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w, y = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(-1) != 1:
            dy2 = dy2.contiguous()
        if dy2.stride(0) % 4:                      # the same for the incoming gradient (pad columns zero)
            N = dy2.shape[1]
            buf = torch.empty((dy2.shape[0], (N + 3) // 4 * 4), dtype=torch.float32, device=dy2.device)
            buf[:, N:] = 0
            buf[:, :N] = dy2
            dy2 = buf[:, :N]
        dz = ops.act_bwd(dy2, y, ctx.act) if ctx.act != ops.ACT_NONE else dy2
        dx = dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = ops.linear_bwd_weight(dz, x2, want_bias=ctx.has_bias)
            if ctx.k_pad:
                dw = dw[:, :dw.shape[1] - ctx.k_pad]
        if ctx.needs_input_grad[0]:
            dx = ops.linear_bwd_input(dz, w).reshape(ctx.in_shape)
        return dx, dw, (db if ctx.has_bias else None), None


def _conv_pitch4(t):
    """t ([B, T, C] / [T, B, C]) itself when its rows have a 16-byte pitch, else a view of a copy whose rows do:
    the conv1d kernels then take 16-byte loads (the pad floats are read and masked, never used)."""
    C = t.shape[2]
    if C % 4 == 0 and t.is_contiguous():
        return t
    full = torch.empty(t.shape[:2] + ((C + 3) // 4 * 4,), dtype=torch.float32, device=t.device)
    full[:, :, C:] = 0
    full[:, :, :C] = t
    return full[:, :, :C]


class Conv1dActFunction(torch.autograd.Function):
    """y = act(conv1d(x, w, b)) over time on channels-last activations ([B, T, C] batch_first, else [T, B, C]);
    rnn_dyn/CNNWrapper.py:55-61 (torch.nn.Conv1d + Tanh / ReLU).  Saves x and y; backward applies act' through y
    and returns dx, dw, db (csrc/conv1d.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, padding, dilation, batch_first, act):
        x = _conv_pitch4(x)
        w = weight.contiguous()
        y = ops.conv1d_fwd(x, w, bias, padding, dilation, batch_first, act)
        ctx.save_for_backward(x, w, y)
        ctx.geometry = (int(padding), int(dilation), bool(batch_first))
        ctx.act = act
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        padding, dilation, batch_first = ctx.geometry
        dz = ops.act_bwd(dy, y, ctx.act) if ctx.act != ops.ACT_NONE else dy
        dz = _conv_pitch4(dz)
        dx = dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = ops.conv1d_bwd_weight(dz, x, w.shape[2], padding, dilation, batch_first,
                                           want_bias=ctx.has_bias)
        if ctx.needs_input_grad[0]:
            T_in = x.shape[1 if batch_first else 0]
            dx = ops.conv1d_bwd_input(dz, w, T_in, padding, dilation, batch_first)
        return dx, dw, (db if ctx.has_bias else None), None, None, None, None


class LayerNormActFunction(torch.autograd.Function):
    """y = act(layer_norm(x) * weight + bias) over the last extent (any leading shape); rnn_dyn/FFWrapper.py: a
    LayerNorm group, torch.nn.LayerNorm + the group's non-linearity.  Saves x, mean and rstd, and y only under an
    activation (its derivative goes through y).  2-D rows stay rows with a 16-byte pitch, like the outputs inside
    a LinearChainFunction: an input of D rounded up to a multiple of four columns (and not D itself: what
    ValidRows.pack hands out, pad columns zero) is taken as rows of D columns, and the [N, D] result is a view of
    rows of that pitch, so the GEMMs of a following Linear group take their 16-byte loads."""

    @staticmethod
    def forward(ctx, x, weight, bias, D, eps, act):
        shape = x.shape
        ctx.col_pad = 0
        if x.dim() == 2:
            x2 = x
            if shape[1] != D and shape[1] == (D + 3) // 4 * 4:
                ctx.col_pad = shape[1] - D
                x2 = x[:, :D]
        else:
            x2 = x.reshape(-1, shape[-1])
        if x2.shape[1] != D:
            raise RuntimeError("LayerNorm over {} features got an input of {} (shape {})"
                               .format(D, x2.shape[1], tuple(shape)))
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        y, mean, rstd = ops.layer_norm_fwd(x2, weight, bias, eps, act, out=_rows_padded(x2.shape[0], D, x2.device))
        ctx.save_for_backward(x2, mean, rstd, weight if weight is not None else x2.new_empty(0),
                              y if act != ops.ACT_NONE else x2.new_empty(0))
        ctx.act, ctx.in_shape = act, shape
        ctx.has = (weight is not None, bias is not None)
        return y if x.dim() == 2 else y.contiguous().reshape(shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, weight, y = ctx.saved_tensors
        has_weight, has_bias = ctx.has
        M, D = x2.shape
        dy2 = dy if dy.dim() == 2 else dy.reshape(-1, D)
        if dy2.stride(-1) != 1 or (M > 1 and dy2.stride(0) < D):     # (an expanded gradient: rows of stride 0)
            dy2 = dy2.contiguous()
        full = torch.empty((M, (D + 3) // 4 * 4), dtype=torch.float32, device=x2.device)
        if full.shape[1] != D:
            full[:, D:] = 0
        dx, dw, db = ops.layer_norm_bwd(dy2, x2, mean, rstd, weight if has_weight else None,
                                        y=y if ctx.act != ops.ACT_NONE else None, act=ctx.act,
                                        want_gamma=has_weight and ctx.needs_input_grad[1],
                                        want_beta=has_bias and ctx.needs_input_grad[2], dx=full[:, :D])
        if len(ctx.in_shape) != 2:
            dx = dx.contiguous().reshape(ctx.in_shape)
        elif ctx.col_pad:
            dx = full
        return (dx if ctx.needs_input_grad[0] else None), dw, db, None, None, None


class AttentionFunction(torch.autograd.Function):
    """o = softmax(q k^T / sqrt(dh)) v per utterance and head on the in-projection's output qkv ([B, T, 3 D] when
    batch_first, else [T, B, 3 D]): torch.nn.MultiheadAttention between its two projections, inside
    torch.nn.TransformerEncoderLayer (rnn_dyn/FFWrapper.py:62-73 builds it by name).  klen: int32 [B] keys per
    utterance on the device, or None for all T.  (p, seed, salt): dropout on the probabilities, p = 0 for none.
    Saves qkv, o and the [B, nhead, T] log-sum-exp: no [T, T] tensor and no mask (csrc/attention.hip)."""

    @staticmethod
    def forward(ctx, qkv, klen, nhead, batch_first, p, seed, salt):
        qkv = qkv.contiguous()
        ctx.args = (int(nhead), klen, bool(batch_first), float(p), int(seed), int(salt))
        o, lse = ops.attention_forward(qkv, *ctx.args)
        ctx.save_for_backward(qkv, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        dqkv = ops.attention_backward(do.contiguous(), qkv, o, lse, *ctx.args)
        return dqkv, None, None, None, None, None, None


class AllPassWarpFunction(torch.autograd.Function):
    """y = all-pass warp of x by alpha (layers/AllPassWarp.py forward, with layers/AllPassWarpLayer.py's
    de-normalisation before and normalisation after inside the same kernel).  x: [.., .., D] with D = nb * N,
    alpha: the same leading shape with a last extent of 1 (or none); mean / std_dev: [D] or None.  One node: saves
    x and alpha only, the backward recomputes the warp; gradients for x and alpha, none for mean / std_dev.  x is
    never written."""

    @staticmethod
    def forward(ctx, x, alpha, mean, std_dev, N):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        if x2.stride(-1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < shape[-1]):
            x2 = x2.contiguous()
        if alpha.numel() != x2.shape[0]:
            raise ValueError("alpha of shape {} does not hold one factor per frame of an input of shape {}"
                             .format(tuple(alpha.shape), tuple(shape)))
        a1 = alpha.reshape(-1).contiguous()
        mean = mean.contiguous() if mean is not None else None
        std_dev = std_dev.contiguous() if std_dev is not None else None
        y = ops.allpass_warp_fwd(x2, a1, N, mean, std_dev)
        ctx.save_for_backward(x2, a1)
        ctx.norm = (mean, std_dev)            # (buffers, not differentiated: no graph hangs on them)
        ctx.N, ctx.in_shape, ctx.alpha_shape = N, shape, alpha.shape
        return y.reshape(shape)

    @staticmethod
    def backward(ctx, dy):
        x2, a1 = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(-1) != 1 or (dy2.shape[0] > 1 and dy2.stride(0) < dy2.shape[1]):
            dy2 = dy2.contiguous()
        dx, da = ops.allpass_warp_bwd(dy2, x2, a1, ctx.N, *ctx.norm)
        return (dx.reshape(ctx.in_shape) if ctx.needs_input_grad[0] else None,
                da.reshape(ctx.alpha_shape) if ctx.needs_input_grad[1] else None, None, None, None)


class MlpgFunction(torch.autograd.Function):
    """The MLPG trajectories of several streams of the same rows as one differentiable node: rows [N, C] (float32 or
    float64; a pitched view is read in place), streams = [(col0, dim, variances [3 * dim] float64), ...], the
    utterances' offsets (or an ops.MlpgPlan made from them) -> [N, sum of dims] in the rows' dtype, the streams side by
    side in the order given.  The forward is `ops.mlpg_generation` per stream (one plan for all of them, as
    MLPG.generation_streams); the backward one `ops.mlpg_adjoint` launch per stream into one [N, C] gradient whose
    other columns are zero.  The trajectory is linear in the rows, so nothing but the plan is saved.  The variances
    are statistics, not parameters: one that requires grad is refused; differentiating the backward is refused too."""

    @staticmethod
    def forward(ctx, rows, streams, offsets, plan):
        for _, _, var in streams:
            if var.requires_grad:
                raise ValueError("MlpgFunction: variances that require grad are not supported (the variances are "
                                 "statistics of the corpus, not parameters)")
        if rows.dtype not in (torch.float32, torch.float64):
            raise TypeError("MlpgFunction: rows must be float32 or float64, got {}".format(rows.dtype))
        if rows.dim() != 2 or rows.stride(1) != 1:
            rows = rows.contiguous()
        if plan is None and len(streams) > 1:
            plan = ops.MlpgPlan(offsets)
        total = sum(int(dim) for _, dim, _ in streams)
        out = torch.empty((rows.shape[0], total), dtype=torch.float64, device=rows.device)
        o0 = 0
        for col0, dim, var in streams:
            ops.mlpg_generation(rows, var, int(dim), offsets, col0=int(col0), out=out, ocol0=o0, plan=plan)
            o0 += int(dim)
        ctx.streams, ctx.offsets, ctx.plan = streams, offsets, plan
        ctx.width, ctx.dtype = rows.shape[1], rows.dtype
        return out if rows.dtype == torch.float64 else out.to(rows.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if grad.dtype != ctx.dtype:
            grad = grad.to(ctx.dtype)
        if grad.stride(1) != 1:
            grad = grad.contiguous()
        gfeat = torch.zeros((grad.shape[0], ctx.width), dtype=ctx.dtype, device=grad.device)
        o0 = 0
        for col0, dim, var in ctx.streams:
            ops.mlpg_adjoint(grad, var, int(dim), ctx.offsets, gcol0=o0, out=gfeat, col0=int(col0), plan=ctx.plan)
            o0 += int(dim)
        return gfeat, None, None, None


def _pitched3(x):
    """x ([B, T, D] / [T, B, D]) as the pooling kernels take it: unit stride on the features, evenly spaced
    positions; anything else is copied"""
    if x.dim() != 3:
        raise ValueError("pooling over time needs a 3-D padded batch, got shape {}".format(tuple(x.shape)))
    return x if ops.pool_pitch(x) is not None else x.contiguous()


class TimePoolFunction(torch.autograd.Function):
    """[B, T, D] / [T, B, D] -> the same with a time extent of 1 (rnn_dyn/Pooling.py: SelectLastPooling row
    len_b - 1, MeanPooling sum over ALL T positions / len_b).  Saves the lengths only; the backward writes every
    position of dx in one launch."""

    @staticmethod
    def forward(ctx, x, lens, batch_first, mode):
        x = _pitched3(x)
        time_dim = 1 if batch_first else 0
        n_utts, t_max = x.shape[1 - time_dim], x.shape[time_dim]
        lens = ops._pool_lens(lens, n_utts, t_max, mode, x.device)
        y = ops.time_pool_fwd(x, lens, batch_first, mode)
        ctx.lens, ctx.t_max, ctx.batch_first, ctx.mode = lens, t_max, batch_first, mode
        return y.unsqueeze(time_dim)

    @staticmethod
    def backward(ctx, dy):
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(-1) != 1 or (dy2.shape[0] > 1 and dy2.stride(0) < dy2.shape[1]):
            dy2 = dy2.contiguous()
        return ops.time_pool_bwd(dy2, ctx.lens, ctx.t_max, ctx.batch_first, ctx.mode), None, None, None


def _fa_operand(t):
    """a [B, R, W] operand the fixed-attention kernels take as it is (unit stride on W, rows and utterances apart),
    else a dense copy"""
    B, R, W = t.shape
    ok = (W <= 1 or t.stride(2) == 1) and (R <= 1 or t.stride(1) >= W) and \
        (B <= 1 or t.stride(0) >= R * (t.stride(1) if R > 1 else W))
    return t if ok else t.contiguous()


class FixedAttentionFunction(torch.autograd.Function):
    """(ctx [B, K, C], Abar [B, K, P]) of the attention matrix A [B, T, P] and the encoder output enc [B, P, C]
    (enc_dec_dyn/attention/FixedAttention.py) on csrc/fixed_attention.hip.  A is a ground-truth input: it gets no
    gradient, and Abar -- what the model returns as "attention" -- is not differentiable.  Saves Abar only."""

    @staticmethod
    def forward(ctx, A, enc, n_frames_per_step, partial_last):
        context, abar = ops.fixed_attention(_fa_operand(A), _fa_operand(enc), n_frames_per_step, partial_last)
        ctx.save_for_backward(abar)
        ctx.mark_non_differentiable(abar)
        return context, abar

    @staticmethod
    def backward(ctx, dctx, _dabar):
        (abar,) = ctx.saved_tensors
        return None, ops.fixed_attention_bwd(abar, _fa_operand(dctx)), None, None


def fixed_attention(A, enc, n_frames_per_step=1, partial_last=False):
    """-> (context, Abar) with the gradient of context flowing into enc; an A that requires grad is refused"""
    if A.requires_grad:
        raise ValueError("fixed_attention: A.requires_grad is set, but the attention matrix is a ground-truth input "
                         "and has no gradient")
    return FixedAttentionFunction.apply(A, enc, int(n_frames_per_step), bool(partial_last))


def _rows2(t, width):
    """[.., width] -> [M, width] rows the kernels take (unit stride on the last extent, rows not overlapping)"""
    t2 = t.reshape(-1, width)
    if t2.stride(-1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < width):
        t2 = t2.contiguous()
    return t2


class VAEReparamFunction(torch.autograd.Function):
    """(z, mu, log_var) of hidden = mu | log_var and a standard-normal draw eps (rnn_dyn/VAE.py:19-27).  mu and
    log_var are views of hidden; the three outputs hang on this ONE node, so the gradient of a reconstruction loss
    into z and the gradient of the KL term into mu / log_var meet in one kernel that writes the whole d(hidden)."""

    @staticmethod
    def forward(ctx, hidden, eps):
        lat = hidden.shape[-1] // 2
        h2 = _rows2(hidden, 2 * lat)
        e2 = _rows2(eps, lat)
        z = ops.vae_reparam_fwd(h2, e2)
        ctx.save_for_backward(h2, e2)
        ctx.set_materialize_grads(False)
        ctx.in_shape = hidden.shape
        mu, log_var = torch.split(hidden, lat, dim=-1)
        return z.reshape(*hidden.shape[:-1], lat), mu, log_var

    @staticmethod
    def backward(ctx, dz, dmu, dlv):
        h2, e2 = ctx.saved_tensors
        lat = e2.shape[1]
        if dz is None and dmu is None and dlv is None:
            return None, None
        grads = [_rows2(g, lat) if g is not None else None for g in (dz, dmu, dlv)]
        return ops.vae_reparam_bwd(grads[0], grads[1], grads[2], h2, e2).reshape(ctx.in_shape), None


# ---- the loss Functions: one launch gives the loss and its gradient(s); backward only scales what forward saved ----
def _scale_saved(grad, dloss, lift=None):
    """d loss / d input from the gradient the forward saved and the gradient of the Function's output.  A summed loss
    (lift None) has a 0-dim dloss: the training loop's `unit_gradient` gives the saved tensor itself, no launch, any
    other factor one product.  An element-wise loss (reduction 'none') passes `lift`, which brings dloss to the saved
    gradient's shape."""
    if lift is not None:
        return grad * lift(dloss)
    return grad if is_unit_gradient(dloss) else grad * dloss


def _as_is(dloss):
    return dloss


def _over_classes(dloss):
    """[..] per-row values -> [.., 1] against logits [.., C]"""
    return dloss.unsqueeze(-1)


def _over_channels(shift):
    """[B, T - shift] per-frame values -> [B, 1, T] against [B, C, T]: the last `shift` frames have no loss"""
    return lambda dloss: (torch.nn.functional.pad(dloss, (0, shift)) if shift else dloss).unsqueeze(1)


# When the gradient is computed: MaskedMSEFunction and WeightedLossFunction always ask the kernel for it, the four
# others follow needs_input_grad (none under no_grad); making them one is a speed change for validation, not done here.
class MaskedMSEFunction(torch.autograd.Function):
    """sum over the valid rows of (pred - target)^2 / (n_valid * D): MSELoss under 'mean_per_frame'"""

    @staticmethod
    def forward(ctx, pred, target, row_valid, n_valid):
        D = pred.shape[-1]
        loss, grad = ops.masked_mse(_rows2(pred, D), _rows2(target, D), row_valid, n_valid, want_grad=True)
        ctx.save_for_backward(grad)
        ctx.shape = pred.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        return _scale_saved(grad, dloss).reshape(ctx.shape), None, None, None


class WeightedLossFunction(torch.autograd.Function):
    """sum_r w[r] sum_c e(pred - target) (e: squared / absolute error) or, with `elementwise`, the
    weighted element-wise values themselves (reduction 'none')."""

    @staticmethod
    def forward(ctx, pred, target, row_weight, kind, elementwise):
        D = pred.shape[-1]
        loss, grad, elem = ops.weighted_loss(_rows2(pred, D), _rows2(target, D), row_weight, kind, want_grad=True,
                                             want_elem=elementwise)
        ctx.save_for_backward(grad)
        ctx.shape, ctx.elementwise = pred.shape, elementwise
        return elem.reshape(pred.shape) if elementwise else loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        return _scale_saved(grad.reshape(ctx.shape), dloss, _as_is if ctx.elementwise else None), None, None, None, None


class VAEKLDFunction(torch.autograd.Function):
    """sum_r w[r] * 0.5 * sum_c (exp(log_var) + mu^2 - 1 - log_var), or with `elementwise` the weighted per-row
    values [.., 1] (reduction 'none'); loss/VAEKLDLoss.py:56-58 with the mask and the reduction folded into w as in
    WeightedLossFunction.  Loss and both gradients come from one launch."""

    @staticmethod
    def forward(ctx, mu, log_var, row_weight, elementwise):
        lat = mu.shape[-1]
        m2, l2 = _rows2(mu, lat), _rows2(log_var, lat)
        # (under no_grad -- validation -- nobody reads the gradients: the kernel then writes none)
        want_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, dmu, dlv, elem = ops.vae_kld(m2, l2, row_weight, want_grad=want_grad, want_elem=elementwise)
        if want_grad:
            ctx.save_for_backward(dmu, dlv)
        ctx.shape, ctx.elementwise = mu.shape, elementwise
        return elem.reshape(*mu.shape[:-1], 1) if elementwise else loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        lift = _as_is if ctx.elementwise else None        # ([.., 1] broadcasts over the latent axis)
        dmu, dlv = (_scale_saved(g.reshape(ctx.shape), dloss, lift) for g in ctx.saved_tensors)
        return dmu, dlv, None, None


class SoftmaxXentFunction(torch.autograd.Function):
    """sum_r w[r] cw[t_r] (lse_r - x[r, t_r]) on logits [.., C] with int64 targets [..], or with `elementwise` the
    weighted per-row values [..] (reduction 'none'); torch.nn.CrossEntropyLoss(reduction='none') with the mask and
    the reduction folded into w as in WeightedLossFunction.  Loss and gradient come from one launch."""

    @staticmethod
    def forward(ctx, logits, target, row_weight, class_weight, ignore_index, elementwise):
        C = logits.shape[-1]
        x2 = _rows2(logits, C)
        want_grad = ctx.needs_input_grad[0]         # (validation runs under no_grad: the kernel then writes none)
        loss, grad, elem = ops.softmax_xent(x2, target.reshape(-1), row_weight, class_weight, ignore_index,
                                            want_grad=want_grad, want_elem=elementwise)
        if want_grad:
            ctx.save_for_backward(grad)
        ctx.shape, ctx.elementwise = logits.shape, elementwise
        return elem.reshape(logits.shape[:-1]) if elementwise else loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        lift = _over_classes if ctx.elementwise else None
        return _scale_saved(grad.reshape(ctx.shape), dloss, lift), None, None, None, None, None


class SoftmaxXentStridedFunction(torch.autograd.Function):
    """The same loss on class-strided logits [B, C, T] against a one-hot target of the same shape, input frame t
    scored against target frame t + shift (loss/OneHotCrossEntropyLoss.py:16-30); the per-frame values are
    [B, T - shift].  The shift is applied by offsets inside the kernel: no sliced copy."""

    @staticmethod
    def forward(ctx, logits, onehot, row_weight, class_weight, ignore_index, shift, elementwise):
        want_grad = ctx.needs_input_grad[0]
        loss, grad, elem = ops.softmax_xent_strided(logits, onehot, row_weight, class_weight, ignore_index, shift,
                                                    want_grad=want_grad, want_elem=elementwise)
        if want_grad:
            ctx.save_for_backward(grad)
        ctx.lift = _over_channels(int(shift or 0)) if elementwise else None
        return elem if elementwise else loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        return _scale_saved(grad, dloss, ctx.lift), None, None, None, None, None, None


class MolLossFunction(torch.autograd.Function):
    """Discretized mixture-of-logistics loss of x [B, 3K, T] against y [B, 1, T], input frame t scored against
    target frame t + shift (loss/DiscretizedMixturelogisticLoss.py): sum of the weighted per-frame values
    [B, T - shift], or with `elementwise` the values themselves.  Loss and gradient come from one launch."""

    @staticmethod
    def forward(ctx, x, y, row_weight, num_classes, log_scale_min, shift, hinge, elementwise):
        want_grad = ctx.needs_input_grad[0]
        loss, grad, elem = ops.mol_loss(x, y, row_weight, num_classes, log_scale_min, shift, hinge,
                                        want_grad=want_grad, want_elem=elementwise)
        if want_grad:
            ctx.save_for_backward(grad)
        ctx.lift = _over_channels(int(shift or 0)) if elementwise else None
        return elem if elementwise else loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        return _scale_saved(grad, dloss, ctx.lift), None, None, None, None, None, None, None


class GluGateFunction(torch.autograd.Function):
    """z [..., G / 2] = tanh(a + ca) * sigmoid(b + cb) of x [..., G] = a | b and an optional c [..., G] = ca | cb: the
    gate of a WaveNet residual layer (csrc/wavenet.hip).  Saves the pre-activations; backward recomputes the two
    activations and returns ONE buffer dx [..., G] for both x and c (c enters by addition)."""

    @staticmethod
    def forward(ctx, x, c):
        G = x.shape[-1]
        x2 = x.reshape(-1, G)
        c2 = c.reshape(-1, G) if c is not None else None
        z = ops.glu_gate(x2, c2)
        ctx.save_for_backward(x2, c2)
        ctx.in_shape = x.shape
        return z.reshape(*x.shape[:-1], G // 2)

    @staticmethod
    def backward(ctx, dz):
        x2, c2 = ctx.saved_tensors
        dx = ops.glu_gate_bwd(dz.reshape(-1, dz.shape[-1]), x2, c2).reshape(ctx.in_shape)
        return (dx if ctx.needs_input_grad[0] else None), (dx if c2 is not None and ctx.needs_input_grad[1] else None)


class grad_scaling(torch.autograd.Function):
    """Identity whose gradient is multiplied by a constant (reference GradientScaling.py: grad_scaling)."""

    @staticmethod
    def forward(ctx, input_, lambda_):
        ctx.lambda_ = float(lambda_)
        return input_.view_as(input_)

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output * ctx.lambda_, None


def _rows_padded(M, N, device):
    """[M, N] view of a fresh buffer whose row pitch is N rounded up to four floats, pad columns zero"""
    Np = (N + 3) // 4 * 4
    full = torch.empty((M, Np), dtype=torch.float32, device=device)
    if Np != N:
        full[:, N:] = 0
    return full[:, :N]


class DropoutStream(object):
    """Seeds of the fused dropout (csrc/dropout.h): next() is a 63-bit integer from a host generator private to the
    package.  It is seeded lazily from torch.initial_seed() plus the process's distributed rank (every rank draws its
    own masks) and seeded again when torch.initial_seed() has changed (a torch.manual_seed between two runs makes the
    runs repeat); reseed(value) sets it to a known state, restart() makes the next draw seed it from torch's seed
    again (the handler's seed() does, so that a second run with the same seed repeats the first).  No public torch
    generator is consumed and nothing touches the device."""

    def __init__(self):
        self._gen = torch.Generator(device="cpu")
        self._torch_seed = None

    def reseed(self, value):
        self._gen.manual_seed(int(value) & 0x7FFFFFFFFFFFFFFF)
        self._torch_seed = torch.initial_seed()

    def restart(self):
        self._torch_seed = None

    def next(self):
        seed = torch.initial_seed()
        if seed != self._torch_seed:
            rank = 0
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                rank = torch.distributed.get_rank()
            self._gen.manual_seed((seed + rank) & 0x7FFFFFFFFFFFFFFF)
            self._torch_seed = seed
        return int(torch.randint(0, 0x7FFFFFFFFFFFFFFF, (1,), generator=self._gen, dtype=torch.int64).item())


_default_dropout_stream = DropoutStream()


def default_dropout_stream():
    """the process's one stream of dropout seeds"""
    return _default_dropout_stream


# `acts` of a LinearChainFunction whose layers carry dropout: drops[i] = (p, salt) of layer i, one seed per call
ChainDropout = collections.namedtuple("ChainDropout", "acts drops seed")


class DropoutFunction(torch.autograd.Function):
    """y = x * m / (1 - p) on rows of any leading shape, mask from (seed, salt, position): the backward is the same
    launch on the gradient and no mask is stored (dropout behind a LayerNorm or pooling group)."""

    @staticmethod
    def forward(ctx, x, p, seed, salt):
        ctx.rule = (float(p), int(seed), int(salt))
        x2 = x.reshape(-1, x.shape[-1])
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        y = torch.empty((x2.shape[0], x2.shape[1]), dtype=torch.float32, device=x.device)
        return ops.dropout_apply(x2, *ctx.rule, out=y).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        d2 = dy.reshape(-1, dy.shape[-1])
        if d2.stride(-1) != 1:
            d2 = d2.contiguous()
        dx = torch.empty((d2.shape[0], d2.shape[1]), dtype=torch.float32, device=dy.device)
        return ops.dropout_apply(d2, *ctx.rule, out=dx).view(dy.shape), None, None, None


class LinearChainFunction(torch.autograd.Function):
    """A run of Linear (+ activation) layers on rows -- the layers of consecutive FFWrapper groups
    (rnn_dyn/FFWrapper.py:63-73) -- as ONE autograd node: forward the same `itts_linear_fwd` launches as the layers
    one by one (the same bits), backward as the flat step runs it (native_ff.py): per layer ONE launch for weight
    gradient, bias gradient and input gradient (`itts_linear_bwd`), the previous layer's activation derivative in its
    epilogue -- no `act_bwd` pass over the rows, no second launch per layer, one node instead of one per layer.
    x: [M, K0] rows, or [M, K0 rounded up to 4] with zeroed pad columns (LinearActFunction's convention);
    acts: tuple of ops.ACT_*, or ChainDropout(acts, drops, seed) for layers with a dropout behind them (drops[i] =
    (p, salt) of layer i; the masks come from the position, so the backward recomputes them and none is saved; with
    every p == 0 the launches are those of the plain tuple); wb: weight0, bias0, weight1, bias1, ..."""

    @staticmethod
    def forward(ctx, x, acts, *wb):
        drops, seed = None, 0
        if isinstance(acts, ChainDropout):
            acts, drops, seed = acts
            if not any(p > 0 for p, _ in drops):
                drops = None
        n = len(acts)
        if x.stride(-1) != 1:
            x = x.contiguous()
        ws, hs, h = [], [], x
        for i in range(n):
            w, b = wb[2 * i], wb[2 * i + 1]
            N, K = w.shape
            w = w.contiguous()
            if i == 0 and h.shape[1] != K and h.shape[1] == (K + 3) // 4 * 4:
                w = torch.nn.functional.pad(w, (0, h.shape[1] - K))
            drop = ops._drop_args(drops[i][0], seed, drops[i][1], 0) if drops is not None and drops[i][0] > 0 else None
            h = ops._linear_fwd(h, w, b, acts[i], _rows_padded(h.shape[0], N, h.device), drop)
            ws.append(w)
            hs.append(h)
        ctx.save_for_backward(x, *hs, *ws)
        ctx.acts, ctx.n = tuple(acts), n
        ctx.drops, ctx.seed = (None if drops is None else tuple((float(p), int(s)) for p, s in drops)), int(seed)
        ctx.k0 = wb[0].shape[1]
        return hs[-1]

    @staticmethod
    def backward(ctx, dy):
        n = ctx.n
        saved = ctx.saved_tensors
        x, hs, ws = saved[0], saved[1:1 + n], saved[1 + n:]
        M = x.shape[0]
        dz = dy
        if dz.stride(-1) != 1 or dz.stride(0) % 4:
            buf = _rows_padded(M, dy.shape[1], dy.device)
            buf.copy_(dy)
            dz = buf
        drops, seed = ctx.drops, ctx.seed
        if drops is not None and drops[-1][0] > 0:
            # back through the last layer's dropout and activation in one pass (its output is the dropped one)
            dz = ops.dropout_act_bwd(dz, hs[-1], ctx.acts[-1], drops[-1][0], seed, drops[-1][1])
        elif ctx.acts[-1] != ops.ACT_NONE:
            dz = ops.act_bwd(dz, hs[-1], ctx.acts[-1])
        grads = [None] * (2 * n)
        dx = None
        for i in range(n - 1, -1, -1):
            w = ws[i]
            N, K = w.shape
            dw = torch.empty((N, K), dtype=torch.float32, device=x.device)
            db = torch.empty((N,), dtype=torch.float32, device=x.device)
            if i > 0:
                dz_in = _rows_padded(M, K, x.device)
                drop = (ops._drop_args(drops[i - 1][0], seed, drops[i - 1][1], 0)
                        if drops is not None and drops[i - 1][0] > 0 else None)
                ops._linear_bwd(dz, hs[i - 1], w, dw, db, dz_in, hs[i - 1], ctx.acts[i - 1], False, drop)
                grads[2 * i], grads[2 * i + 1] = dw, db
                dz = dz_in
            else:
                if ctx.needs_input_grad[0]:
                    dx = torch.empty((M, K), dtype=torch.float32, device=x.device)
                    ops.linear_bwd(dz, x, w, dw, db, dx)
                else:
                    ops.linear_bwd_weight(dz, x, dw=dw, db=db)
                grads[0], grads[1] = (dw[:, :ctx.k0] if K != ctx.k0 else dw), db
        return (dx, None) + tuple(grads)


def _iptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class PackedBatch(object):
    """Index bookkeeping of pack_padded_sequence(enforce_sorted=False) (rnn_dyn/RNNWrapper.py:89-92)
    for a padded batch: rows sorted by decreasing length (stable), packed row of frame t of sorted
    row b = row_off[t] + b.  `flat_index` maps every packed row to its row in the padded tensor
    flattened over (time, batch) -- or (batch, time) when batch_first -- so packing is one
    index_select and unpacking one index_copy."""

    _cache = collections.OrderedDict()      # (lengths, padded_time, batch_first, device) -> instance
    _cache_max = 16

    @classmethod
    def get(cls, lengths, padded_time, batch_first, device):
        """The bookkeeping of a batch whose lengths were seen recently is reused (its tables are ~1 ms of
        numpy and eight small uploads during which the GPU has nothing to do: validation passes and
        trainers that keep their batches fixed over the epochs meet the same length vectors again)."""
        import numpy as np
        lens = np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64)
        key = (lens.tobytes(), int(padded_time), bool(batch_first), str(device))
        pb = cls._cache.get(key)
        if pb is None:
            pb = cls(lens, padded_time, batch_first, device)
            cls._cache[key] = pb
            while len(cls._cache) > cls._cache_max:
                cls._cache.popitem(last=False)
        else:
            cls._cache.move_to_end(key)
        return pb

    def __init__(self, lengths, padded_time, batch_first, device):
        import numpy as np
        lengths = np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64)
        if lengths.ndim != 1 or len(lengths) == 0 or lengths.min() < 1:
            raise ValueError("lengths must be a non-empty vector of positive values")
        if lengths.max() > padded_time:
            raise ValueError("a length exceeds the padded time extent")
        self.B, self.T = len(lengths), int(lengths.max())
        perm = np.argsort(-lengths, kind="stable")
        sorted_len = lengths[perm]
        nact = (sorted_len[None, :] > np.arange(self.T)[:, None]).sum(axis=1)      # [T]
        row_off = np.concatenate([[0], np.cumsum(nact)[:-1]])
        self.N = int(nact.sum())
        t_of = np.repeat(np.arange(self.T), nact)
        b_of = np.arange(self.N) - row_off[t_of]
        flat = perm[b_of] * padded_time + t_of if batch_first else t_of * self.B + perm[b_of]
        self.h_lengths = torch.from_numpy(sorted_len.astype(np.int32))            # host, sorted
        self.d_lengths = self.h_lengths.to(device)
        self.d_row_off = torch.from_numpy(row_off.astype(np.int32)).to(device)
        # packed row the reverse direction visits at step s for sorted row b (0 where inactive)
        t_rev = np.maximum(sorted_len[None, :] - 1 - np.arange(self.T)[:, None], 0)  # [T, B]
        rev = row_off[t_rev] + np.arange(self.B)[None, :]
        self.d_rev_row = torch.from_numpy(np.ascontiguousarray(rev, dtype=np.int32)).to(device)
        self.flat_index = torch.from_numpy(flat.astype(np.int64)).to(device)
        # padded position -> packed row (-1: padding), for the way back
        inv = np.full(self.B * int(padded_time), -1, dtype=np.int64)
        inv[flat] = np.arange(self.N)
        self.inv_flat = torch.from_numpy(inv).to(device)
        # packed row of the previous frame of the same sequence in each direction's visiting order
        # (forward: t - 1, reverse: t + 1); first frames point at row N, where shift() puts h0
        prev_f = np.where(t_of > 0, row_off[np.maximum(t_of - 1, 0)] + b_of, self.N)
        nxt = np.minimum(t_of + 1, self.T - 1)
        prev_r = np.where(t_of + 1 < sorted_len[b_of], row_off[nxt] + b_of, self.N)
        self.prev_row = [torch.from_numpy(p_.astype(np.int64)).to(device) for p_ in (prev_f, prev_r)]
        self.perm = torch.from_numpy(perm.astype(np.int64)).to(device)
        self.inv_perm = torch.from_numpy(np.argsort(perm).astype(np.int64)).to(device)

    def pack(self, padded, pad_cols=False):
        """[T, B, F] (or [B, T, F]) -> [N, F]; pad_cols: -> [N, F rounded up to a multiple of 4] with zero
        columns (rows of 16-byte multiples let the GEMM entry points take their LDS-DMA kernel)."""
        flat2 = padded.reshape(-1, padded.shape[-1])
        F = flat2.shape[1]
        return RowsGatherFunction.apply(flat2, self.flat_index, self.inv_flat, (F + 3) // 4 * 4 if pad_cols else F)

    def unpack(self, packed, padded_shape):
        """[N, D] -> zero-padded [T, B, D] / [B, T, D] (pad_packed_sequence)"""
        out = RowsGatherFunction.apply(packed, self.inv_flat, self.flat_index, packed.shape[-1])
        return out.reshape(padded_shape[0], padded_shape[1], packed.shape[-1])

    def shift(self, y, h0, ndir, H):
        """h_{t-1} of every packed frame: the layer output [N, ndir*H] moved by one frame along each
        sequence (per direction), the initial state h0 [ndir, H] (or zeros) at the first frame."""
        out = torch.empty_like(y)
        for d in range(ndir):
            ops.rows_gather(y[:, d * H:(d + 1) * H], self.prev_row[d], fill_row=h0[d] if h0 is not None else None,
                            out=out[:, d * H:(d + 1) * H])
        return out

    def first_rows(self, d):
        """Packed rows of the first frame direction d processes in every sequence ([B] indices):
        where the recurrence starts from the initial state."""
        cache = self.__dict__.setdefault("_first_rows", {})
        if d not in cache:
            cache[d] = (self.prev_row[d] == self.N).nonzero().reshape(-1)
        return cache[d]

    def last_rows(self, d):
        """Packed row of the last frame direction d processes in every sequence ([B] indices in sorted row order):
        where the final state h_n comes from.  Forward: frame len_b - 1, the reverse direction's first; reverse:
        frame 0."""
        cache = self.__dict__.setdefault("_last_rows", {})
        if d not in cache:
            cache[d] = self.d_rev_row[0].long() if d == 0 else torch.arange(self.B, device=self.d_rev_row.device)
        return cache[d]

    def _hptr(self):
        return ctypes.c_void_p(self.h_lengths.data_ptr())


_padding_state = threading.local()


class padding_rows_identical(object):
    """Context in which the caller vouches that all padding positions of the padded batches it hands to the model
    hold the same row (true of ModularModelHandlerPyTorch.prepare_batch: pad_sequence writes zeros): the
    frame-independent layer groups then run on the valid rows plus one representative row (ValidRows) instead of
    every position of the padded tensor.  Outside such a context they compute all positions, as the reference
    does."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = getattr(_padding_state, "identical", False)
        _padding_state.identical = self.on
        return self

    def __exit__(self, *exc):
        _padding_state.identical = self.prev


def padding_is_identical():
    return getattr(_padding_state, "identical", False)


class ValidRows(object):
    """Bookkeeping of a padded batch for layers that treat every frame on its own (the Linear groups of
    rnn_dyn/FFWrapper.py): they run on the VALID rows of the batch, stored back to back in the batch's own order
    (utterance b at rows starts[b] ..), plus ONE row for all the padding positions -- the reference computes every
    padding position of [B, T, F] (a third of an LJSpeech batch of 32 utterances), and every one of them holds the
    same row (pad_sequence / pad_packed_sequence write zeros, an embedding of a padded index the same vector), so
    one representative gives their common value: `representative` is the flat position (in the batch's layout) of
    the last frame of the shortest utterance.  Unlike PackedBatch nothing is sorted and nothing but the lengths is
    uploaded: starts / lens are what the kernels of csrc/batch_rows.hip index with."""

    _cache = collections.OrderedDict()
    _cache_max = 16

    @classmethod
    def get(cls, lengths, padded_time, batch_first, device):
        import numpy as np
        lens = np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64)
        key = (lens.tobytes(), int(padded_time), bool(batch_first), str(device))
        vr = cls._cache.get(key)
        if vr is None:
            vr = cls(lens, padded_time, batch_first, device)
            cls._cache[key] = vr
            while len(cls._cache) > cls._cache_max:
                cls._cache.popitem(last=False)
        else:
            cls._cache.move_to_end(key)
        return vr

    def __init__(self, lengths, padded_time, batch_first, device):
        import numpy as np
        if lengths.ndim != 1 or len(lengths) == 0 or lengths.min() < 0:
            raise ValueError("lengths must be a non-empty vector of non-negative values")
        if lengths.max() > padded_time:
            raise ValueError("a length exceeds the padded time extent")
        self.B, self.T, self.batch_first = len(lengths), int(padded_time), bool(batch_first)
        self.N = int(lengths.sum())
        self.n_pad = self.B * self.T - self.N
        table = np.empty((2, self.B), dtype=np.int64)
        table[0, 0] = 0
        np.cumsum(lengths[:-1], out=table[0, 1:])
        table[1] = lengths
        host = torch.from_numpy(table)
        if torch.cuda.is_available():
            host = host.pin_memory()
        self.table = host.to(device, non_blocking=True)       # ONE upload: starts, lens
        self.starts, self.lens = self.table[0], self.table[1]
        b = int(np.argmin(lengths))
        self.representative = (b * self.T + self.T - 1) if batch_first else ((self.T - 1) * self.B + b)

    def pack(self, padded, pad_cols=True):
        """[B, T, F] / [T, B, F] -> [N (+ 1 when the batch has padding), F rounded up to a multiple of 4]"""
        return PackValidFunction.apply(padded, self, pad_cols)

    def unpack(self, rows):
        """[N (+ 1), D] -> [B, T, D] / [T, B, D]; the padding positions take the last row's value"""
        return UnpackValidFunction.apply(rows, self)


class PackValidFunction(torch.autograd.Function):
    """Valid rows of a padded batch back to back, then (when the batch has padding) the representative padding
    row.  Backward: valid positions take their row's gradient; the gradient of the extra row -- the SUM over all
    padding positions of what the layers passed back -- lands on the representative position, the other padding
    positions get zero: whatever produced the identical padding rows sees the same total."""

    @staticmethod
    def forward(ctx, padded, vr, pad_cols):
        if not padded.is_contiguous():
            padded = padded.contiguous()
        F = padded.shape[2]
        width = (F + 3) // 4 * 4 if pad_cols else F
        out = torch.empty((vr.N + (1 if vr.n_pad else 0), width), dtype=torch.float32, device=padded.device)
        ops.batch_pack_rows(padded, vr.starts, vr.lens, vr.batch_first, vr.N, out_width=width, out=out,
                            rep_pos=vr.representative if vr.n_pad else -1, rep_dst_row=vr.N)
        ctx.vr, ctx.F = vr, F
        return out             # (with its zeroed pad columns: LinearActFunction pads its weight to match)

    @staticmethod
    def backward(ctx, grad):
        vr, F = ctx.vr, ctx.F
        g = grad[:, :F] if grad.stride(-1) == 1 else grad[:, :F].contiguous()
        dx, _ = ops.batch_pad_gather(g[:vr.N], vr.starts, vr.lens, vr.B, vr.T, vr.batch_first, width=F,
                                     rep_pos=vr.representative if vr.n_pad else -1,
                                     rep_row=g[vr.N] if vr.n_pad else None)
        return dx, None, None


class UnpackValidFunction(torch.autograd.Function):
    """[N (+ 1), D] rows -> the padded batch, every padding position holding the extra row (zeros without one).
    Backward: the rows of the valid positions, and for the extra row the column sums over the padding
    positions (csrc/batch_rows.hip: fixed summation order)."""

    @staticmethod
    def forward(ctx, rows, vr):
        if rows.stride(-1) != 1:
            rows = rows.contiguous()
        fill = rows[vr.N] if vr.n_pad else None
        out, _ = ops.batch_pad_gather(rows[:vr.N], vr.starts, vr.lens, vr.B, vr.T, vr.batch_first, fill_row=fill)
        ctx.vr = vr
        return out

    @staticmethod
    def backward(ctx, grad):
        vr = ctx.vr
        if not grad.is_contiguous():
            grad = grad.contiguous()
        D = grad.shape[2]
        # rows of 16-byte multiples for the GEMMs of the layers' backward (LinearActFunction.backward pads otherwise)
        width = (D + 3) // 4 * 4
        full = torch.empty((vr.N + (1 if vr.n_pad else 0), width), dtype=torch.float32, device=grad.device)
        ops.batch_pack_rows(grad, vr.starts, vr.lens, vr.batch_first, vr.N, out_width=width, out=full)
        if vr.n_pad:
            ops.batch_pad_colsum(grad, vr.lens, vr.batch_first, out=full[vr.N])
        return full[:, :D], None


class RowsGatherFunction(torch.autograd.Function):
    """out[r] = src[idx[r]] (zeros where idx[r] < 0), optionally widened by zero columns; the gradient
    is the gather through the inverse map `idx_back` (pack and unpack are each other's adjoint)."""

    @staticmethod
    def forward(ctx, src, idx, idx_back, out_width):
        ctx.save_for_backward(idx_back)
        ctx.width = src.shape[1]
        if src.stride(-1) != 1:
            src = src.contiguous()
        return ops.rows_gather(src, idx, out_width=out_width)

    @staticmethod
    def backward(ctx, grad):
        (idx_back,) = ctx.saved_tensors
        g = grad if grad.stride(-1) == 1 else grad.contiguous()
        return ops.rows_gather(g, idx_back, width=ctx.width), None, None, None


class StatesToCallerOrder(torch.autograd.Function):
    """The final states of the layers -- each [ndir, B, Hl] in the batch's sorted row order, Hl >= H when the
    hidden size was padded -- as ONE [layers * ndir, B, H] tensor in the caller's row order (what torch.nn.LSTM /
    GRU return as h_n / c_n): one native row gather per layer straight into its slice (the index_select per
    layer and the torch.cat over the layers were the last torch kernels between the recurrent layers)."""

    @staticmethod
    def forward(ctx, inv_perm, perm, H, *states):
        ndir, B = states[0].shape[0], states[0].shape[1]
        out = torch.empty((len(states) * ndir, B, H), dtype=torch.float32, device=states[0].device)
        o2 = out.view(-1, H)
        for i, st in enumerate(states):
            st = st if st.is_contiguous() else st.contiguous()
            for d in range(ndir):
                ops.rows_gather(st[d], inv_perm, width=H, out=o2[(i * ndir + d) * B:(i * ndir + d + 1) * B])
        ctx.save_for_backward(perm)
        ctx.meta = (ndir, B, H, [st.shape[2] for st in states])
        return out

    @staticmethod
    def backward(ctx, grad):
        (perm,) = ctx.saved_tensors
        ndir, B, H, widths = ctx.meta
        g2 = (grad if grad.is_contiguous() else grad.contiguous()).view(-1, H)
        outs = []
        for i, Hl in enumerate(widths):
            g = torch.empty((ndir, B, Hl), dtype=torch.float32, device=grad.device)
            for d in range(ndir):
                ops.rows_gather(g2[(i * ndir + d) * B:(i * ndir + d + 1) * B], perm, width=H, out=g[d], out_width=Hl)
            outs.append(g)
        return (None, None, None) + tuple(outs)


def _pad4_cols(t):
    """[R, F] -> [R, F rounded up to a multiple of 4] (zero columns): rows of 16-byte multiples let
    the GEMM entry points take their LDS-DMA kernel; F = 425 (the question labels) otherwise sends
    the first recurrent layer's three GEMMs through the register-staged one (3.2 + 2.7 + 0.7 ms
    instead of ~2.1 + 2.3 + 0.5 ms per training step at the bench size)."""
    F = t.shape[1]
    if F % 4 == 0:
        return t
    return torch.nn.functional.pad(t, (0, 4 - F % 4))


def _input_projection(x2, w_ih, b_ih, b_hh=None):
    """The input projection of all frames of a recurrent layer, one GEMM on packed rows x2 [N, F] (they may arrive
    with their rows already padded to 16-byte multiples) against w_ih [ndir, G*H, F] plus b_ih (+ b_hh: the LSTM
    adds both biases here, the GRU's b_hh stays inside its reset gate).
    -> (x2 and w_ih [ndir*G*H, F] with 4-column rows, gin [N, ndir*G*H], pre_padded)"""
    F = w_ih.shape[-1]
    pre_padded = x2.shape[1] != F
    x2 = _pad4_cols(x2.contiguous())
    w_ih_cat = _pad4_cols(w_ih.reshape(-1, F))
    gin = ops.linear_fwd(x2, w_ih_cat, (b_ih if b_hh is None else b_ih + b_hh).reshape(-1), ops.ACT_NONE)
    return x2, w_ih_cat, gin, pre_padded


def _initial_state_grad(dg, w_hh, pb, ndir):
    """Trainable initial states (RNNWrapper train_hidden_init): one vector per direction shared by all rows, so
    the rows' W_hh^T dG at their first processed frame, summed over the rows -> [ndir, H]."""
    G = dg.shape[1] // ndir
    return torch.stack([ops.linear_bwd_input(
        ops.rows_gather(dg[:, d * G:(d + 1) * G], pb.first_rows(d)).sum(0, keepdim=True), w_hh[d])[0]
        for d in range(ndir)], dim=0)


def _weight_grads(dgi, dgh, x2, hprev, F, ndir, want_hh_bias):
    """dW_hh (+ db_hh) from the gradient wrt the hidden projections dgh [N, ndir*G*H] and the states that entered
    each step hprev [N, ndir*H], then dW_ih [ndir, G*H, F] and db_ih [ndir*G*H] from dgi and the layer's input x2.
    The launch right behind a recurrence runs 20-25 % slow (the chip comes back from light load: LABNOTES 12g):
    the small products W_hh' take that place, the large one follows (95.9 -> 95.6 ms per 3 x 512 BiLSTM step,
    two A/B pairs against dW_ih first).  -> (dw_ih, db_ih, dw_hh, db_hh or None)"""
    H = hprev.shape[1] // ndir
    G = dgh.shape[1] // ndir
    dw_hh = torch.empty((ndir, G, H), dtype=torch.float32, device=dgh.device)
    db_hh = torch.empty((ndir, G), dtype=torch.float32, device=dgh.device) if want_hh_bias else None
    for d in range(ndir):
        _, db = ops.linear_bwd_weight(dgh[:, d * G:(d + 1) * G], hprev[:, d * H:(d + 1) * H],
                                      dw=dw_hh[d], want_bias=want_hh_bias)
        if want_hh_bias:
            db_hh[d] = db
    dw_ih, db_ih = ops.linear_bwd_weight(dgi, x2)                 # [ndir*G*H, F (padded)], [ndir*G*H]
    return dw_ih[:, :F].reshape(ndir, G, F), db_ih, dw_hh, db_hh


def _input_grad(dgi, w_ih_cat, F, pre_padded):
    """dX = dG W_ih, cut back to the F columns the layer received unless its rows arrived padded"""
    dx = ops.linear_bwd_input(dgi, w_ih_cat)
    return dx if pre_padded else dx[:, :F]


class LSTMLayerFunction(torch.autograd.Function):
    """One (bi)directional LSTM layer on packed rows x [N, F] (see PackedBatch)."""

    @staticmethod
    def forward(ctx, x2, pb, w_ih, w_hh, b_ih, b_hh, h0, c0, training):
        L = _lib.load()
        N = x2.shape[0]
        F = w_ih.shape[-1]
        ndir, G4, H = w_hh.shape
        T, B = pb.T, pb.B
        x2, w_ih_cat, gin, pre_padded = _input_projection(x2, w_ih, b_ih, b_hh)
        dev = x2.device
        y = torch.empty((N, ndir * H), dtype=torch.float32, device=dev)
        keep = bool(training)
        gates = torch.empty((N, ndir * G4), dtype=torch.float32, device=dev) if keep else None
        csave = torch.empty((N, ndir * H), dtype=torch.float32, device=dev) if keep else None
        hn = torch.empty((ndir, B, H), dtype=torch.float32, device=dev)
        cn = torch.empty((ndir, B, H), dtype=torch.float32, device=dev)
        state = torch.empty(L.itts_lstm_state_bytes(B, H, ndir), dtype=torch.uint8, device=dev)
        w_hh_c = w_hh.contiguous()
        h0c = h0.contiguous() if h0 is not None else None
        c0c = c0.contiguous() if c0 is not None else None
        _lib.check(L.itts_lstm_layer_fwd(_iptr(gin), _iptr(w_hh_c), _iptr(h0c), _iptr(c0c),
                                         _iptr(pb.d_lengths), pb._hptr(), _iptr(pb.d_row_off),
                                         _iptr(pb.d_rev_row), T, B, H, ndir, _iptr(y),
                                         _iptr(gates), _iptr(csave), _iptr(hn), _iptr(cn),
                                         _iptr(state), ops._stream()), "itts_lstm_layer_fwd")
        ctx.set_materialize_grads(False)      # unused h_n / c_n arrive as None in backward
        if not keep:
            ctx.mark_non_differentiable(y, hn, cn)
        if keep:
            empty = torch.empty(0, device=dev)
            ctx.save_for_backward(x2, w_ih_cat, w_hh_c, gates, csave, y,
                                  h0c if h0c is not None else empty,
                                  c0c if c0c is not None else empty)
            ctx.pb = pb
            ctx.dims = (F, H, ndir, h0c is not None, c0c is not None, pre_padded)
        return y, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn, dcn):
        if dhn is not None or dcn is not None:
            raise NotImplementedError("Gradients through the final states h_n / c_n are not "
                                      "implemented (the acoustic models only use the output).")
        L = _lib.load()
        x2, w_ih_cat, w_hh, gates, csave, y, h0, c0 = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(y)
        pb = ctx.pb
        F, H, ndir, has_h0, has_c0, pre_padded = ctx.dims
        hprev = pb.shift(y, h0 if has_h0 else None, ndir, H)
        G4 = 4 * H
        dev = dy.device
        dy2 = dy.contiguous()
        dg = torch.empty((pb.N, ndir * G4), dtype=torch.float32, device=dev)
        state = torch.empty(L.itts_lstm_state_bytes(pb.B, H, ndir), dtype=torch.uint8, device=dev)
        want_h0, want_c0 = ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        dc0_rows = torch.empty((ndir, pb.B, H), dtype=torch.float32, device=dev) if want_c0 else None
        _lib.check(L.itts_lstm_layer_bwd(_iptr(dy2), _iptr(w_hh), _iptr(c0 if has_c0 else None),
                                         _iptr(gates), _iptr(csave), pb._hptr(),
                                         _iptr(pb.d_row_off), _iptr(pb.d_rev_row), pb.T, pb.B, H, ndir,
                                         _iptr(dg), _iptr(dc0_rows), _iptr(state), ops._stream()),
                   "itts_lstm_layer_bwd")
        dh0 = _initial_state_grad(dg, w_hh, pb, ndir) if want_h0 else None
        dc0 = dc0_rows.sum(dim=1) if want_c0 else None
        dw_ih, db, dw_hh, _ = _weight_grads(dg, dg, x2, hprev, F, ndir, want_hh_bias=False)
        dx = _input_grad(dg, w_ih_cat, F, pre_padded) if ctx.needs_input_grad[0] else None
        db = db.reshape(ndir, G4)
        return dx, None, dw_ih, dw_hh, db, db.clone(), dh0, dc0, None


class GRULayerFunction(torch.autograd.Function):
    """One (bi)directional GRU layer on packed rows x [N, F] (torch.nn.GRU on a PackedSequence,
    rnn_dyn/RNNWrapper.py:45-107)."""

    @staticmethod
    def forward(ctx, x2, pb, w_ih, w_hh, b_ih, b_hh, h0, training):
        L = _lib.load()
        N = x2.shape[0]
        F = w_ih.shape[-1]
        ndir, G3, H = w_hh.shape
        T, B = pb.T, pb.B
        x2, w_ih_cat, gin, pre_padded = _input_projection(x2, w_ih, b_ih)
        dev = x2.device
        y = torch.empty((N, ndir * H), dtype=torch.float32, device=dev)
        keep = bool(training)
        gates = torch.empty((N, ndir * H * 4), dtype=torch.float32, device=dev) if keep else None
        hn = torch.empty((ndir, B, H), dtype=torch.float32, device=dev)
        state = torch.empty(L.itts_gru_state_bytes(B, H, ndir), dtype=torch.uint8, device=dev)
        w_hh_c, b_hh_c = w_hh.contiguous(), b_hh.contiguous()
        h0c = h0.contiguous() if h0 is not None else None
        _lib.check(L.itts_gru_layer_fwd(_iptr(gin), _iptr(w_hh_c), _iptr(b_hh_c), _iptr(h0c),
                                        _iptr(pb.d_lengths), pb._hptr(), _iptr(pb.d_row_off),
                                        _iptr(pb.d_rev_row), T, B, H, ndir, _iptr(y), _iptr(gates),
                                        _iptr(hn), _iptr(state), ops._stream()),
                   "itts_gru_layer_fwd")
        ctx.set_materialize_grads(False)
        if not keep:
            ctx.mark_non_differentiable(y, hn)
        if keep:
            ctx.save_for_backward(x2, w_ih_cat, w_hh_c, gates, y,
                                  h0c if h0c is not None else torch.empty(0, device=dev))
            ctx.pb = pb
            ctx.dims = (F, H, ndir, h0c is not None, pre_padded)
        return y, hn

    @staticmethod
    def backward(ctx, dy, dhn):
        if dhn is not None:
            raise NotImplementedError("Gradients through the final state h_n are not implemented "
                                      "(the acoustic models only use the output).")
        L = _lib.load()
        x2, w_ih_cat, w_hh, gates, y, h0 = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(y)
        pb = ctx.pb
        F, H, ndir, has_h0, pre_padded = ctx.dims
        hprev = pb.shift(y, h0 if has_h0 else None, ndir, H)
        G3 = 3 * H
        dev = dy.device
        dy2 = dy.contiguous()
        dgi = torch.empty((pb.N, ndir * G3), dtype=torch.float32, device=dev)
        dgh = torch.empty((pb.N, ndir * G3), dtype=torch.float32, device=dev)
        state = torch.empty(L.itts_gru_state_bytes(pb.B, H, ndir), dtype=torch.uint8, device=dev)
        want_h0 = ctx.needs_input_grad[6]
        dh0_rows = torch.empty((ndir, pb.B, H), dtype=torch.float32, device=dev) if want_h0 else None
        _lib.check(L.itts_gru_layer_bwd(_iptr(dy2), _iptr(w_hh), _iptr(gates),
                                        _iptr(hprev), pb._hptr(), _iptr(pb.d_row_off),
                                        _iptr(pb.d_rev_row), pb.T, pb.B, H, ndir, _iptr(dgi),
                                        _iptr(dgh), _iptr(dh0_rows), _iptr(state), ops._stream()),
                   "itts_gru_layer_bwd")
        dh0 = None
        if want_h0:      # direct part dh * z from the kernel + recurrent part W_hh^T dGh, summed over rows
            dh0 = dh0_rows.sum(dim=1) + _initial_state_grad(dgh, w_hh, pb, ndir)
        dw_ih, db_ih, dw_hh, db_hh = _weight_grads(dgi, dgh, x2, hprev, F, ndir, want_hh_bias=True)
        dx = _input_grad(dgi, w_ih_cat, F, pre_padded) if ctx.needs_input_grad[0] else None
        return dx, None, dw_ih, dw_hh, db_ih.reshape(ndir, G3), db_hh, dh0, None


class RNNLayerFunction(torch.autograd.Function):
    """One (bi)directional vanilla RNN layer, h_t = act(gin_t + W_hh h_{t-1}) with act = ops.ACT_TANH / ACT_RELU, on
    packed rows x [N, F] (torch.nn.RNN on a PackedSequence, rnn_dyn/RNNWrapper.py:45-107).  Saves nothing of the
    recurrence but y.  Unlike the LSTM / GRU functions it takes a gradient into h_n: h_n of a row is y at the last
    frame its direction processes, so that gradient is added to dy there."""

    @staticmethod
    def forward(ctx, x2, pb, w_ih, w_hh, b_ih, b_hh, h0, training, act):
        L = _lib.load()
        N = x2.shape[0]
        F = w_ih.shape[-1]
        ndir, H, _ = w_hh.shape
        x2, w_ih_cat, gin, pre_padded = _input_projection(x2, w_ih, b_ih, b_hh)
        dev = x2.device
        y = torch.empty((N, ndir * H), dtype=torch.float32, device=dev)
        hn = torch.empty((ndir, pb.B, H), dtype=torch.float32, device=dev)
        state = torch.empty(L.itts_rnn_layer_state_bytes(pb.B, H, ndir), dtype=torch.uint8, device=dev)
        w_hh_c = w_hh.contiguous()
        h0c = h0.contiguous() if h0 is not None else None
        _lib.check(L.itts_rnn_layer_fwd(_iptr(gin), _iptr(w_hh_c), _iptr(h0c), _iptr(pb.d_lengths), pb._hptr(),
                                        _iptr(pb.d_row_off), _iptr(pb.d_rev_row), pb.T, pb.B, H, ndir, act, _iptr(y),
                                        _iptr(hn), _iptr(state), ops._stream()), "itts_rnn_layer_fwd")
        ctx.set_materialize_grads(False)
        if training:
            ctx.save_for_backward(x2, w_ih_cat, w_hh_c, y, h0c if h0c is not None else torch.empty(0, device=dev))
            ctx.pb = pb
            ctx.dims = (F, H, ndir, h0c is not None, pre_padded, act)
        else:
            ctx.mark_non_differentiable(y, hn)
        return y, hn

    @staticmethod
    def backward(ctx, dy, dhn):
        L = _lib.load()
        x2, w_ih_cat, w_hh, y, h0 = ctx.saved_tensors
        pb = ctx.pb
        F, H, ndir, has_h0, pre_padded, act = ctx.dims
        dy2 = torch.zeros_like(y) if dy is None else dy.contiguous()
        if dhn is not None:
            dy2 = dy2.clone() if dy2 is dy else dy2
            for d in range(ndir):
                dy2[:, d * H:(d + 1) * H].index_add_(0, pb.last_rows(d), dhn[d])
        hprev = pb.shift(y, h0 if has_h0 else None, ndir, H)
        dg = torch.empty((pb.N, ndir * H), dtype=torch.float32, device=y.device)
        state = torch.empty(L.itts_rnn_layer_state_bytes(pb.B, H, ndir), dtype=torch.uint8, device=y.device)
        _lib.check(L.itts_rnn_layer_bwd(_iptr(dy2), _iptr(w_hh), _iptr(y), pb._hptr(), _iptr(pb.d_row_off),
                                        _iptr(pb.d_rev_row), pb.T, pb.B, H, ndir, act, _iptr(dg), _iptr(state),
                                        ops._stream()), "itts_rnn_layer_bwd")
        dh0 = _initial_state_grad(dg, w_hh, pb, ndir) if ctx.needs_input_grad[6] else None
        dw_ih, db, dw_hh, _ = _weight_grads(dg, dg, x2, hprev, F, ndir, want_hh_bias=False)
        dx = _input_grad(dg, w_ih_cat, F, pre_padded) if ctx.needs_input_grad[0] else None
        db = db.reshape(ndir, H)
        return dx, None, dw_ih, dw_hh, db, db.clone(), dh0, None, None
