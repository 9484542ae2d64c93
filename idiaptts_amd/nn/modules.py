"""nn.Modules with torch.nn-compatible parameter names on top of the HIP kernels, so that the
reference's state dicts load unchanged (`module.0.weight`,
`module.weight_ih_l0[_reverse]`, ...)."""
import collections
import math
import os

import numpy as np
import torch
from torch import nn

from .. import ops
from .functional import (AllPassWarpFunction, AttentionFunction, ChainDropout, Conv1dActFunction, DropoutFunction,
                         GRULayerFunction, LayerNormActFunction, LinearActFunction, LinearChainFunction, LSTMLayerFunction,
                         MlpgFunction, PackedBatch, RNNLayerFunction, StatesToCallerOrder, TimePoolFunction,
                         VAEReparamFunction, default_dropout_stream, grad_scaling)


class LinearAct(nn.Linear):
    """torch.nn.Linear whose forward/backward run the fp32-MFMA kernels; `act` (a name of ops.ACT_BY_NAME, any
    case, or an ops.ACT_* code) fuses the following activation of an FFWrapper group into the GEMM epilogue."""

    def __init__(self, in_features, out_features, bias=True, act=None):
        code = ops.act_code(act)
        super().__init__(in_features, out_features, bias=bias)
        self.act = code

    def forward(self, input_):
        return LinearActFunction.apply(input_, self.weight, self.bias, self.act)


class Conv1dAct(nn.Conv1d):
    """torch.nn.Conv1d (same parameters, same initialisation, same RNG draws) whose forward/backward run the
    fp32-MFMA implicit-GEMM kernels of csrc/conv1d.hip; `act` fuses the following Tanh / ReLU into the epilogue.
    Activations are channels-last and keep the model's layout: input [B, T, Cin] when `batch_first`, else
    [T, B, Cin]; output [B, T_out, Cout] / [T_out, B, Cout] (torch's Conv1d takes [B, Cin, T]).
    Built: stride 1, groups 1, padding_mode 'zeros', integer padding; anything else raises NotImplementedError."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, padding_mode="zeros", act=None, batch_first=True):
        if isinstance(padding, str):
            raise NotImplementedError("Conv1d padding={!r}: only integer padding is implemented".format(padding))
        for name, value in (("kernel_size", kernel_size), ("stride", stride), ("padding", padding),
                            ("dilation", dilation)):
            if isinstance(value, (tuple, list)) and len(value) != 1:
                raise NotImplementedError("Conv1d {}={}: only 1-D convolutions are implemented".format(name, value))
        if _first(stride) != 1:
            raise NotImplementedError("Conv1d stride={}: only stride 1 is implemented".format(stride))
        if groups != 1:
            raise NotImplementedError("Conv1d groups={}: only groups=1 is implemented".format(groups))
        if padding_mode != "zeros":
            raise NotImplementedError("Conv1d padding_mode={!r}: only 'zeros' is implemented".format(padding_mode))
        code = ops.act_code(act, ops.CONV_ACTS, "Conv1d")
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                         groups=groups, bias=bias, padding_mode=padding_mode)
        self.act = code
        self.batch_first = batch_first

    def forward(self, input_):
        return Conv1dActFunction.apply(input_, self.weight, self.bias, self.padding[0], self.dilation[0],
                                       self.batch_first, self.act)

    def output_length(self, lengths):
        """T_out of inputs of T_in steps (tensor or int)"""
        return lengths + 2 * self.padding[0] - self.dilation[0] * (self.kernel_size[0] - 1)


class LayerNormAct(nn.LayerNorm):
    """torch.nn.LayerNorm over the last extent (same parameters `weight` / `bias`, ones and zeros) whose
    forward/backward run the row kernels of csrc/layernorm.hip; `act` (as LinearAct's) fuses the following
    activation of an FFWrapper group.  `normalized_shape` is an int or a one-element list / tuple of at most
    ops.LAYER_NORM_MAX_WIDTH; the input is [N, D] rows or a padded batch [B, T, D] / [T, B, D] (any leading shape).
    CPU tensors go through torch.nn.functional.layer_norm and the torch activation."""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True, bias=True, act=None, **kwargs):
        code = ops.act_code(act, where="LayerNorm")
        if isinstance(normalized_shape, (tuple, list, torch.Size)) and len(normalized_shape) != 1:
            raise NotImplementedError("LayerNorm normalized_shape={}: only the last dimension is normalised"
                                      .format(tuple(normalized_shape)))
        width = int(_first(normalized_shape))
        if not 1 <= width <= ops.LAYER_NORM_MAX_WIDTH:
            raise NotImplementedError("LayerNorm over {} features: the kernel takes 1 .. {}"
                                      .format(width, ops.LAYER_NORM_MAX_WIDTH))
        super().__init__(normalized_shape, eps=eps, elementwise_affine=elementwise_affine, bias=bias, **kwargs)
        self.act = code

    def forward(self, input_):
        if not input_.is_cuda:
            y = torch.nn.functional.layer_norm(input_, self.normalized_shape, self.weight, self.bias, self.eps)
            return y if self.act == ops.ACT_NONE else getattr(nn, ops.ACT_TORCH_NAME[self.act])()(y)
        return LayerNormActFunction.apply(input_, self.weight, self.bias, self.normalized_shape[0], self.eps,
                                          self.act)


class _SelfAttentionParameters(nn.Module):
    """The parameters of torch.nn.MultiheadAttention for self-attention with one embedding width, under its names
    (`in_proj_weight`, `in_proj_bias`, `out_proj.weight`, `out_proj.bias`), created and initialised in its order:
    the out-projection as a Linear, then xavier_uniform_ on the in-projection and zeros in both biases."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty((3 * embed_dim, embed_dim)))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.0)
        nn.init.constant_(self.out_proj.bias, 0.0)

    def extra_repr(self):
        return "embed_dim={}, num_heads={}".format(self.embed_dim, self.num_heads)


class TransformerEncoderLayer(nn.Module):
    """torch.nn.TransformerEncoderLayer (same constructor arguments, parameter names, shapes and initial values,
    so its state dicts and the reference's load key for key) on the HIP kernels: the in-projection is one GEMM to
    [rows, 3 d_model], the attention core runs csrc/attention.hip (no [T, T] tensor), the out-projection is a GEMM,
    the feed-forward is one LinearChainFunction node with ReLU and its dropouts fused, both norms run the LayerNorm
    row kernel.  `norm_first` reorders, nothing else.

    forward(x, lengths=None, mask_padding=False): x is [B, T, d_model] when batch_first, else [T, B, d_model].
    Without lengths or with mask_padding=False every position of the padded tensor is a key (what the reference
    computes: it passes no mask); with mask_padding=True the keys of utterance b are its first lengths[b] positions
    (torch's src_key_padding_mask).  Every query position is computed either way.

    `dropout` applies, as in torch, to the attention probabilities, behind the attention and the feed-forward
    branches, and inside the feed-forward; in train() only.  Masks follow the counter rule of csrc/dropout.h: one
    seed per forward from `nn.functional.DropoutStream`, and the salts 4 * salt + 0 .. 3 for the four places, `salt`
    being the block's index in its model.

    Refused by name (NotImplementedError): an activation other than "relu" (GELU needs the stored pre-activation),
    a callable activation, bias=False, and sizes outside the kernel's envelope (ops.attention_check_envelope)."""

    salt = 0

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", layer_norm_eps=1e-5,
                 batch_first=False, norm_first=False, bias=True):
        super().__init__()
        if d_model % nhead != 0:
            raise ValueError("d_model = {} must be divisible by nhead = {}".format(d_model, nhead))
        if not isinstance(activation, str):
            raise NotImplementedError("TransformerEncoderLayer activation {!r}: a callable activation is not "
                                      "implemented, only \"relu\"".format(activation))
        if activation != "relu":
            raise NotImplementedError("TransformerEncoderLayer activation={!r} is not implemented, only \"relu\" "
                                      "(the backward of GELU needs the stored pre-activation)".format(activation))
        if not bias:
            raise NotImplementedError("TransformerEncoderLayer bias=False is not implemented")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("TransformerEncoderLayer dropout must be in [0, 1), got {}".format(dropout))
        ops.attention_check_envelope(d_model, nhead)
        self.d_model, self.nhead, self.dim_feedforward = d_model, nhead, dim_feedforward
        self.p = float(dropout)
        self.batch_first, self.norm_first = bool(batch_first), bool(norm_first)
        self.self_attn = _SelfAttentionParameters(d_model, nhead)
        self.linear1 = LinearAct(d_model, dim_feedforward, act="relu")
        self.linear2 = LinearAct(dim_feedforward, d_model)
        self.norm1 = LayerNormAct(d_model, eps=layer_norm_eps)
        self.norm2 = LayerNormAct(d_model, eps=layer_norm_eps)

    def extra_repr(self):
        return "d_model={}, nhead={}, dim_feedforward={}, dropout={}, batch_first={}, norm_first={}".format(
            self.d_model, self.nhead, self.dim_feedforward, self.p, self.batch_first, self.norm_first)

    def key_lengths(self, x, lengths):
        """int32 [B] on x's device (what the kernel reads), clipped to the padded extent"""
        T = x.shape[1 if self.batch_first else 0]
        if torch.is_tensor(lengths) and lengths.dtype == torch.int32 and lengths.device == x.device:
            return lengths
        return torch.as_tensor(lengths).to(device=x.device, dtype=torch.int32).clamp(1, T).contiguous()

    def _attention(self, x, klen, p, seed):
        sa = self.self_attn
        qkv = LinearActFunction.apply(x, sa.in_proj_weight, sa.in_proj_bias, ops.ACT_NONE)
        a = AttentionFunction.apply(qkv, klen, self.nhead, self.batch_first, p, seed, 4 * self.salt)
        a = LinearActFunction.apply(a, sa.out_proj.weight, sa.out_proj.bias, ops.ACT_NONE)
        return DropoutFunction.apply(a, p, seed, 4 * self.salt + 1) if p > 0.0 else a

    def _feed_forward(self, x, p, seed):
        acts = (self.linear1.act, self.linear2.act)
        if p > 0.0:
            acts = ChainDropout(acts, ((p, 4 * self.salt + 2), (p, 4 * self.salt + 3)), seed)
        rows = LinearChainFunction.apply(x.reshape(-1, x.shape[-1]), acts, self.linear1.weight, self.linear1.bias,
                                         self.linear2.weight, self.linear2.bias)
        return rows.reshape(x.shape)

    def forward(self, x, lengths=None, mask_padding=False):
        if x.dim() != 3 or x.shape[2] != self.d_model:
            raise ValueError("TransformerEncoderLayer over d_model = {} got an input of shape {}"
                             .format(self.d_model, tuple(x.shape)))
        klen = self.key_lengths(x, lengths) if mask_padding and lengths is not None else None
        p = self.p if self.training else 0.0
        seed = default_dropout_stream().next() if p > 0.0 else 0
        if self.norm_first:
            x = x + self._attention(self.norm1(x), klen, p, seed)
            return x + self._feed_forward(self.norm2(x), p, seed)
        x = self.norm1(x + self._attention(x, klen, p, seed))
        return self.norm2(x + self._feed_forward(x, p, seed))


class AllPassWarp(nn.Module):
    """All-pass frequency warping of cepstral features, the reference's layers/AllPassWarp.py: every block of
    `warp_matrix_size` coefficients of a frame is multiplied by the all-pass matrix of the frame's warping factor.
    `forward(in_tensor, alphas) -> (out, combined_alphas)` with in_tensor [B, T, D] or [T, B, D] and alphas one
    tensor, or a list / tuple of tensors, of the same two leading extents and a last extent of 1.  The matrix is
    never built: csrc/allpass.hip applies its recursion per frame, so there is no coefficient buffer (the
    reference's `w_matrix_3d` is non-persistent: state dicts are the same), the results are finite at any size up
    to ops.ALLPASS_MAX_SIZE, and the input is not modified (the reference halves columns of it in place).  `mean` /
    `std_dev` [D] de-normalise the input and normalise the output inside the same kernel."""

    def __init__(self, warp_matrix_size):
        super().__init__()
        warp_matrix_size = int(warp_matrix_size)
        if warp_matrix_size < 1:
            raise ValueError("warp_matrix_size must be at least 1, got {}".format(warp_matrix_size))
        if warp_matrix_size > ops.ALLPASS_MAX_SIZE:
            raise NotImplementedError("warp_matrix_size={}: the kernel takes at most {}"
                                      .format(warp_matrix_size, ops.ALLPASS_MAX_SIZE))
        self.warp_matrix_size = warp_matrix_size

    def init_hidden(self, batch_size=1):
        return None

    @staticmethod
    def combine_warping_parameters(alphas):
        """Successive all-pass warps by a1, a2, .. are one warp by the reduction (a1 + a2) / (1 + a1 a2)."""
        if not isinstance(alphas, (list, tuple)):
            return alphas
        combined = alphas[0]
        for alpha in alphas[1:]:
            combined = (combined + alpha) / (1 + combined * alpha)
        return combined

    def forward(self, in_tensor, alphas, mean=None, std_dev=None):
        width = in_tensor.shape[-1]
        if width % self.warp_matrix_size != 0:
            raise ValueError("feature width {} is not a multiple of warp_matrix_size {}"
                             .format(width, self.warp_matrix_size))
        combined = AllPassWarp.combine_warping_parameters(alphas)
        out = AllPassWarpFunction.apply(in_tensor, combined, mean, std_dev, self.warp_matrix_size)
        return out, combined

    def extra_repr(self):
        return "warp_matrix_size={}".format(self.warp_matrix_size)


def mlpg_dense(rows, dim, variances):
    """The MLPG trajectory [T, dim] of ONE utterance's rows [T, 3 * dim] (static | delta | delta-delta) by torch ops
    on a dense precision matrix: P = sum_w W_w^T diag(tau_w) W_w per dimension and torch.linalg.solve, differentiable
    by autograd.  O(dim T^3): MLPGLayer's path for CPU tensors, for tests and small inputs only."""
    T = rows.shape[0]
    eye = torch.eye(T, dtype=rows.dtype, device=rows.device)
    up, down = torch.diag_embed(eye.new_ones(max(T - 1, 0)), 1), torch.diag_embed(eye.new_ones(max(T - 1, 0)), -1)
    windows = (eye, 0.5 * (up - down), up + down - 2.0 * eye)
    edge = eye.new_ones(T, 1)
    if T > 0:
        edge[0] = edge[T - 1] = 0.0
    P, b = 0.0, 0.0
    for w, W in enumerate(windows):
        tau = (1.0 / variances[w * dim:(w + 1) * dim]).to(rows.dtype).expand(T, dim)
        if w > 0:      # the delta variances of the first and last frame are 1e11 (misc/mlpg.py:114-117)
            tau = tau * edge + (1.0 - edge) * 1e-11
        P = P + torch.einsum("ti,td,tj->dij", W, tau, W)
        b = b + W.t() @ (tau * rows[:, w * dim:(w + 1) * dim])
    return torch.linalg.solve(P, b.t().unsqueeze(-1)).squeeze(-1).t()


class MLPGLayer(nn.Module):
    """MLPG as a differentiable layer: the trajectories of the streams of a padded batch of static | delta |
    delta-delta features, so that a loss can be taken on what the listener hears (trajectory training).

    `streams` is a list of (col0, dim, variances): the stream's 3 * dim columns start at input column col0, variances
    [3 * dim] is the diagonal of its covariance.  `passthrough` lists single input columns (V/UV) that are copied.
    The output has sum(dim) + len(passthrough) columns, the streams' trajectories and the passthrough columns in the
    order of their first input column -- for a WORLD reader coded_sp | lf0 | vuv | bap, the layout of a reader with
    add_deltas=False.  With `mean` / `std_dev` ([C], both or neither) the valid frames are de-normalised (x * std_dev +
    mean) before the solve and the output is normalised again with the entries of the columns it came from (a stream's
    static columns).  Padding positions of the output are zero; lengths pass through unchanged.

    `forward(input_, seq_lengths_input=..., max_length_inputs=..., **kwargs) -> (output, kwargs)` with input_
    [B, T, C] (`batch_first`) or [T, B, C], float32 or float64; without lengths every frame is valid.
    `select_only=True` solves nothing: it returns the same columns of its input unchanged (static columns instead of
    trajectories), to cut a target down to the layout of the prediction.

    Variances (`variances_0`, `variances_1`, .. in stream order, float64), `mean` and `std_dev` are buffers: they move
    with `.to()` and are in the state dict; there are no parameters.

    On the GPU the solve and its gradient are ops.mlpg_generation / ops.mlpg_adjoint (MlpgFunction).  CPU tensors go
    through `mlpg_dense`: float64 torch ops on a dense precision matrix per utterance, cubic in the length -- for
    tests and small inputs only."""

    class Config:
        def __init__(self, streams, passthrough=(), mean=None, std_dev=None, batch_first=True, select_only=False):
            self.streams = streams
            self.passthrough = passthrough
            self.mean = mean
            self.std_dev = std_dev
            self.batch_first = batch_first
            self.select_only = select_only

        def create_model(self):
            return MLPGLayer(self.streams, passthrough=self.passthrough, mean=self.mean, std_dev=self.std_dev,
                             batch_first=self.batch_first, select_only=self.select_only)

    _cache_max = 16

    def __init__(self, streams, passthrough=(), mean=None, std_dev=None, batch_first=True, select_only=False):
        super().__init__()
        if (mean is None) != (std_dev is None):
            raise ValueError("MLPGLayer: mean and std_dev are given together or not at all")
        self.batch_first, self.select_only = bool(batch_first), bool(select_only)
        self.stream_cols = []          # (col0, dim) per stream
        taken = {}                     # input column -> who reads it
        pieces = []                    # (first input column, static columns)
        for i, (col0, dim, variances) in enumerate(streams):
            col0, dim = int(col0), int(dim)
            var = torch.as_tensor(np.asarray(variances, dtype=np.float64)).reshape(-1).clone()
            if col0 < 0 or dim < 1 or var.numel() != 3 * dim:
                raise ValueError("MLPGLayer: stream {} (col0 {}, dim {}) needs col0 >= 0, dim >= 1 and 3 * dim "
                                 "variances, got {}".format(i, col0, dim, var.numel()))
            if not bool((var > 0).all()) or not bool(torch.isfinite(var).all()):
                raise ValueError("MLPGLayer: stream {} has non-positive variances".format(i))
            for c in range(col0, col0 + 3 * dim):
                if c in taken:
                    raise ValueError("MLPGLayer: stream {} overlaps {} at column {}".format(i, taken[c], c))
                taken[c] = "stream {}".format(i)
            self.register_buffer("variances_{}".format(i), var)
            self.stream_cols.append((col0, dim))
            pieces.append((col0, list(range(col0, col0 + dim))))
        for c in passthrough:
            c = int(c)
            if c < 0 or c in taken:
                raise ValueError("MLPGLayer: passthrough column {} {}".format(
                    c, "overlaps " + taken[c] if c in taken else "is negative"))
            taken[c] = "passthrough column {}".format(c)
            pieces.append((c, [c]))
        if not pieces:
            raise ValueError("MLPGLayer: no streams and no passthrough columns")
        self.passthrough = [int(c) for c in passthrough]
        self.min_width = max(taken) + 1
        if mean is not None:
            mean = torch.as_tensor(np.asarray(mean, dtype=np.float64)).reshape(-1).clone()
            std_dev = torch.as_tensor(np.asarray(std_dev, dtype=np.float64)).reshape(-1).clone()
            if mean.numel() != std_dev.numel():
                raise ValueError("MLPGLayer: mean has {} entries, std_dev {}".format(mean.numel(), std_dev.numel()))
            for i, (col0, dim) in enumerate(self.stream_cols):
                if col0 + 3 * dim > mean.numel():
                    raise ValueError("MLPGLayer: stream {} (columns {} .. {}) lies beyond the input width {}"
                                     .format(i, col0, col0 + 3 * dim - 1, mean.numel()))
            if self.min_width > mean.numel():
                raise ValueError("MLPGLayer: passthrough column {} lies beyond the input width {}"
                                 .format(max(self.passthrough), mean.numel()))
            self.register_buffer("mean", mean)
            self.register_buffer("std_dev", std_dev)
        else:
            self.mean = self.std_dev = None
        pieces.sort(key=lambda p: p[0])
        self.order = [p[0] for p in pieces]                  # first input column of every output piece, ascending
        # the input column every output column comes from (a stream's static columns); not part of the state dict
        self.register_buffer("out_cols", torch.tensor([c for _, cols in pieces for c in cols], dtype=torch.int64),
                             persistent=False)
        self._layouts = collections.OrderedDict()

    def init_hidden(self, batch_size=1):
        return None

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_layouts"] = collections.OrderedDict()          # (plans are handles of this process: made again on use)
        return state

    def extra_repr(self):
        return "streams={}, passthrough={}, normalised={}, batch_first={}, select_only={}".format(
            self.stream_cols, self.passthrough, self.mean is not None, self.batch_first, self.select_only)

    def _layout(self, lengths, B, T, device):
        """(flat positions of the valid frames in utterance order, the utterances' offsets, an ops.MlpgPlan on the
        GPU) for a batch of these lengths, kept for the batches that come again"""
        lens = np.full(B, T, dtype=np.int64) if lengths is None \
            else np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64).reshape(-1)
        if len(lens) != B or (B and (lens.min() < 0 or lens.max() > T)):
            raise ValueError("MLPGLayer: {} lengths (max {}) for a batch of {} x {} frames".format(
                len(lens), lens.max() if len(lens) else 0, B, T))
        key = (lens.tobytes(), T, str(device))
        hit = self._layouts.get(key)
        if hit is not None:
            self._layouts.move_to_end(key)
            return hit
        u = np.repeat(np.arange(B, dtype=np.int64), lens)
        offsets = np.concatenate(([0], np.cumsum(lens)))
        t = np.arange(int(offsets[-1]), dtype=np.int64) - offsets[u]
        idx = torch.from_numpy(u * T + t if self.batch_first else t * B + u).to(device)
        offsets = [int(o) for o in offsets]
        plan = ops.MlpgPlan(offsets) if device.type == "cuda" and len(self.stream_cols) > 1 else None
        self._layouts[key] = (idx, offsets, plan)
        while len(self._layouts) > self._cache_max:
            self._layouts.popitem(last=False)
        return idx, offsets, plan

    def _variances(self, i):
        var = getattr(self, "variances_{}".format(i))
        return var if var.dtype == torch.float64 else var.double()

    def forward(self, input_, seq_lengths_input=None, max_length_inputs=None, **kwargs):
        kwargs["seq_lengths_input"], kwargs["max_length_inputs"] = seq_lengths_input, max_length_inputs
        if input_.dim() != 3 or input_.shape[2] < self.min_width:
            raise ValueError("MLPGLayer: input of shape {} is not a padded batch of at least {} columns"
                             .format(tuple(input_.shape), self.min_width))
        if self.mean is not None and input_.shape[2] != self.mean.numel():
            raise ValueError("MLPGLayer: input width {} but {} normalisation entries"
                             .format(input_.shape[2], self.mean.numel()))
        if self.select_only:
            return input_.index_select(2, self.out_cols), kwargs
        B, T = (input_.shape[0], input_.shape[1]) if self.batch_first else (input_.shape[1], input_.shape[0])
        idx, offsets, plan = self._layout(seq_lengths_input, B, T, input_.device)
        rows = input_.reshape(B * T, input_.shape[2]).index_select(0, idx)
        on_gpu = input_.is_cuda
        if not on_gpu:
            rows = rows.double()
        if self.mean is not None:
            rows = rows * self.std_dev.to(rows.dtype) + self.mean.to(rows.dtype)
        streams = [(col0, dim, self._variances(i)) for i, (col0, dim) in enumerate(self.stream_cols)]
        if on_gpu:
            traj = MlpgFunction.apply(rows, streams, offsets, plan)
            trajs, o0 = {}, 0
            for col0, dim, _ in streams:
                trajs[col0] = traj[:, o0:o0 + dim]
                o0 += dim
        else:
            trajs = {col0: torch.cat([mlpg_dense(rows[offsets[u]:offsets[u + 1], col0:col0 + 3 * dim], dim, var)
                                      for u in range(B) if offsets[u + 1] > offsets[u]] or [rows[:0, :dim]], dim=0)
                     for col0, dim, var in streams}
        out_rows = torch.cat([trajs[c] if c in trajs else rows[:, c:c + 1] for c in self.order], dim=1)
        if self.mean is not None:
            out_rows = (out_rows - self.mean.to(rows.dtype)[self.out_cols]) / self.std_dev.to(rows.dtype)[self.out_cols]
        out_rows = out_rows.to(input_.dtype)
        out = out_rows.new_zeros((B * T, out_rows.shape[1])).index_copy(0, idx, out_rows)
        return out.reshape(input_.shape[:2] + (out_rows.shape[1],)), kwargs


class Pooling(nn.Module):
    """A padded batch [B, T, D] (batch_first) or [T, B, D] reduced to a time extent of 1 (reference
    rnn_dyn/Pooling.py); `forward` takes the pair `(input, seq_lengths_input)` that `select_inputs` makes.
    Deviation: `get_output_length` returns ones of the argument's kind WITHOUT writing into it -- the reference's
    `seq_lengths_input.fill_(1)` overwrites the caller's length tensor (the handler's own lengths of the input
    feature), and fails on the plain integers kept in `max_lengths`, which are accepted here."""
    mode = None

    def __init__(self, batch_first):
        super().__init__()
        self.batch_first = batch_first

    def extra_repr(self):
        return "batch_first={}".format(self.batch_first)

    def get_output_length(self, seq_lengths_input):
        if seq_lengths_input is None:
            return None
        if torch.is_tensor(seq_lengths_input):
            return torch.ones_like(seq_lengths_input)
        if isinstance(seq_lengths_input, (list, tuple)):
            return type(seq_lengths_input)(1 for _ in seq_lengths_input)
        return 1

    def select_inputs(self, input_, **kwargs):
        return input_, kwargs.pop("seq_lengths_input", None)

    def forward(self, input_):
        input_, lengths = input_
        return TimePoolFunction.apply(input_, lengths, self.batch_first, self.mode)


class SelectLastPooling(Pooling):
    """Each utterance's frame `length - 1` (frame T - 1 without lengths): reference Pooling.py:26-44."""
    mode = ops.POOL_LAST


class MeanPooling(Pooling):
    """The sum over ALL T positions of the padded batch, padding included, divided by the utterance's length:
    what the reference's MeanPooling.forward computes (Pooling.py:55-64) and what its checkpoints were trained
    with.  After a recurrent group the padding is zero and this is the masked mean; after Linear groups the padding
    rows hold act(bias) and are counted."""
    mode = ops.POOL_MEAN

    def __init__(self, batch_first):
        super().__init__(batch_first)
        self.time_dim = 1 if batch_first else 0


class VanillaVAE(nn.Module):
    """hidden = linear(input) (no bias, [2 * latent_dim, dim_in]: the reference's state-dict key `linear.weight`),
    mu | log_var = the two halves of hidden (views), z = eps * exp(0.5 * log_var) + mu; returns (z, mu, log_var)
    -- reference rnn_dyn/VAE.py.  eps comes from exactly one torch.randn_like call per forward on a dense tensor of
    z's shape, in training AND in evaluation, as the reference's `randn_like(std)`: under the same seed on the same
    device the draw is `randn_like` of such a tensor (pinned by tests/test_gpu_latent.py), and a test can substitute
    it."""

    def __init__(self, dim_in, latent_dim):
        super().__init__()
        self.linear = LinearAct(dim_in, latent_dim * 2, bias=False)

    def forward(self, input):
        hidden = self.linear(input)
        # (on a dense tensor of z's shape, like the reference's `randn_like(std)`)
        eps = torch.randn_like(hidden.new_empty(hidden.shape[:-1] + (hidden.shape[-1] // 2,)))
        return VAEReparamFunction.apply(hidden, eps)


class GradientScaling(nn.Module):
    """Identity in the forward, gradient times `lambda_` in the backward (reference GradientScaling.py)."""

    def __init__(self, lambda_):
        super().__init__()
        self.lambda_ = float(lambda_)

    def forward(self, input_):
        return grad_scaling.apply(input_, self.lambda_)

    def extra_repr(self):
        return "lambda={}".format(self.lambda_)


def _first(v):
    return v[0] if isinstance(v, (tuple, list, torch.Size)) else v


_cu_count = {}


def _persistent_width(H, rows, ndir, device):
    """512 when a layer of hidden size H < 512 is better run zero-padded to the width the persistent
    recurrences (csrc/rnn_persist.h) are built for, else None.  Those keep a whole recurrence inside one launch
    at ~4 us per time step where the per-step kernels other sizes take cost ~9 us, but they take 8 / ndir tiles of
    16 rows per round and the padded products are larger; measured on 3 x Bi-LSTM / GRU training steps of 2-10 s
    utterances (scripts/rnn_hidden_probe.py, profiles/r6_rnn_hidden_probe.txt): H 128 / 256 / 384 at 64
    utterances (one round) -15 / -17 / -22 % of the step, H 256 at 128 / 256 utterances 0 / +10 %, H 384 -17 / -3 %.
    ITTS_RNN_PAD_HIDDEN=0 / 1 forces it off / on; ITTS_RNN_PERSISTENT=0 (no persistent kernels) turns it off too."""
    force = os.environ.get("ITTS_RNN_PAD_HIDDEN")
    if not (128 <= H < 512) or force == "0" or os.environ.get("ITTS_RNN_PERSISTENT", "1")[:1] == "0":
        return None
    if force == "1":
        return 512
    if device.type != "cuda":
        return None
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _cu_count:
        _cu_count[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    if _cu_count[idx] != 256:
        return None
    rounds = -(-((rows + 15) // 16) // (8 // ndir))
    allowed = 1 if H < 320 else (2 if H < 448 else 4)
    return 512 if rounds <= allowed else None


def _pad_hidden(w_ih, w_hh, biases, h0s, G, H, rows=0, persistent=True):
    """The recurrence kernels tile the hidden units in groups of 16.  Any other hidden size runs
    zero-padded to the next multiple -- or to 512 where that puts the layer on the persistent recurrences
    (_persistent_width; `persistent`: the cell has them) --: a padded unit has zero weights and biases, so its gates sit
    at sigma(0) / tanh(0) / relu(0), its state stays exactly 0 and -- its W_hh columns being zero -- it never
    reaches a real unit.  Differentiable torch ops: autograd slices the gradients back.
    w_ih [ndir, G*H, F], w_hh [ndir, G*H, H], biases [ndir, G*H] each, h0s [ndir, H] or None."""
    Hp = (persistent and _persistent_width(H, rows, w_ih.shape[0], w_ih.device)) or (H + 15) // 16 * 16
    if Hp == H:
        return w_ih, w_hh, biases, h0s, H
    ndir, _, F = w_ih.shape
    pad = torch.nn.functional.pad
    w_ih = pad(w_ih.reshape(ndir, G, H, F), (0, 0, 0, Hp - H)).reshape(ndir, G * Hp, F)
    w_hh = pad(w_hh.reshape(ndir, G, H, H), (0, Hp - H, 0, Hp - H)).reshape(ndir, G * Hp, Hp)
    biases = [pad(b.reshape(ndir, G, H), (0, Hp - H)).reshape(ndir, G * Hp) for b in biases]
    h0s = [pad(h, (0, Hp - H)) if h is not None else None for h in h0s]
    return w_ih, w_hh, biases, h0s, Hp


def _unpad_rows(x, ndir, H, Hp):
    """[N, ndir*Hp] -> [N, ndir*H]"""
    if Hp == H:
        return x
    return x.reshape(x.shape[0], ndir, Hp)[:, :, :H].reshape(x.shape[0], ndir * H)


def _rows_share_state(h):
    """whether all rows of the state h [layers*dirs, B, H] are one row (None: the zero state)"""
    if h is None or h.shape[1] == 1 or h.stride(1) == 0 or getattr(h, "_itts_rows_shared", False):
        return True
    if getattr(h, "_itts_rows_own", False):      # (what a step returned: no comparison on the device, no wait)
        return False
    return bool((h == h[:, :1]).all())


def _shared_initial_state(h):
    """The recurrence kernels take ONE initial state per layer and direction, shared by all rows
    (what RNNWrapper.init_hidden passes: a [.., 1, H] vector expanded over the batch).  Anything
    else would silently be replaced by row 0's state, so it is refused.  (One frame on per-row states runs on the
    cell kernel instead: _RNNBase._step_forward.)"""
    if not _rows_share_state(h):
        raise NotImplementedError("Per-sequence initial states are implemented for one time step without gradients "
                                  "only (the step of an autoregressive decoder): all rows of hx must be equal (expand "
                                  "one [layers*dirs, 1, H] state) for longer inputs or under autograd.  "
                                  "Scheduled-sampling training is the follow-up.")


class _RNNBase(nn.Module):
    """What LSTM, GRU and RNN share: torch.nn's parameters (weight_ih_l0[_reverse], weight_hh_.., bias_ih_..,
    bias_hh_.. per layer and direction, in torch.nn's order -- the checkpoints' and the Adam arena's layout) with
    `_gates` blocks of hidden_size rows, their initialisation, packing and inter-layer dropout."""
    _gates = 1
    _persistent = True       # the cell has persistent recurrences (rnn_persist.h) worth padding a layer to 512 for
    _layer_extra = ()        # what the cell's layer function takes behind `training`

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=False,
                 dropout=0.0, bidirectional=False):
        super().__init__()
        assert bias, "bias=False is not supported"
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.batch_first, self.dropout, self.bidirectional = batch_first, dropout, bidirectional
        ndir = 2 if bidirectional else 1
        G = self._gates * hidden_size
        for layer in range(num_layers):
            in_size = input_size if layer == 0 else hidden_size * ndir
            for d in range(ndir):
                sfx = "_l{}{}".format(layer, "_reverse" if d == 1 else "")
                self.register_parameter("weight_ih" + sfx, nn.Parameter(torch.empty(G, in_size)))
                self.register_parameter("weight_hh" + sfx, nn.Parameter(torch.empty(G, hidden_size)))
                self.register_parameter("bias_ih" + sfx, nn.Parameter(torch.empty(G)))
                self.register_parameter("bias_hh" + sfx, nn.Parameter(torch.empty(G)))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.hidden_size)
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def _stack(self, name, layer):
        ndir = 2 if self.bidirectional else 1
        return torch.stack([getattr(self, "{}_l{}{}".format(name, layer, "_reverse" if d else ""))
                            for d in range(ndir)], dim=0)

    def _pack(self, input_, lengths, pad_cols):
        """-> (PackedBatch, the valid frames as packed rows, sorted by length)"""
        time_dim, batch_dim = (1, 0) if self.batch_first else (0, 1)
        if lengths is None:
            lengths = torch.full((input_.shape[batch_dim],), input_.shape[time_dim])
        pb = PackedBatch.get(lengths, input_.shape[time_dim], self.batch_first, input_.device)
        return pb, pb.pack(input_, pad_cols=pad_cols)

    def _dropout(self, x, layer):
        if self.dropout > 0 and self.training and layer < self.num_layers - 1:
            x = torch.nn.functional.dropout(x, self.dropout, True)
        return x

    _cell_kind = None        # ops.CELL_*

    def _step_forward(self, input_, h0s, lengths):
        """One frame for every row from the row's OWN state (the step of an autoregressive decoder, which comes back
        with the states its last call returned): per layer and direction the two products on the dense GEMM and the
        cell on csrc/rnn_cell.hip.  No autograd.  With one frame the backward direction's output is its first step,
        so both directions step from their [B, H] slice of the state.  -> what _recurrent_forward returns."""
        ndir = 2 if self.bidirectional else 1
        B, H = input_.shape[0 if self.batch_first else 1], self.hidden_size
        if lengths is not None and not (torch.is_tensor(lengths) and lengths.is_cuda) \
                and any(int(n) != 1 for n in lengths):
            raise ValueError("a step on per-row states takes one frame of every row: lengths must be all 1")
        with torch.no_grad():
            x = input_.reshape(B, input_.shape[-1]).contiguous()
            states = [h if h is not None else x.new_zeros(self.num_layers * ndir, B, H) for h in h0s]
            finals = [[] for _ in h0s]
            act = self._layer_extra[0] if self._layer_extra else ops.ACT_NONE
            for layer in range(self.num_layers):
                outs = []
                for d in range(ndir):
                    sfx = "_l{}{}".format(layer, "_reverse" if d == 1 else "")
                    b_ih, b_hh = getattr(self, "bias_ih" + sfx), getattr(self, "bias_hh" + sfx)
                    gru = self._cell_kind == ops.CELL_GRU
                    gi = ops.linear_fwd(x, getattr(self, "weight_ih" + sfx).contiguous(),
                                        b_ih if gru else b_ih + b_hh)
                    h = states[0][layer * ndir + d].contiguous()
                    gh = ops.linear_fwd(h, getattr(self, "weight_hh" + sfx).contiguous(), None)
                    c = states[1][layer * ndir + d].contiguous() if len(states) > 1 else None
                    h, c = ops.rnn_cell_step(self._cell_kind, gi, gh, h, c, b_hh if gru else None, act)
                    outs.append(h)
                    finals[0].append(h)
                    if c is not None:
                        finals[1].append(c)
                x = self._dropout(outs[0] if ndir == 1 else torch.cat(outs, dim=1), layer)
            out = x.reshape(input_.shape[:-1] + (ndir * H,))
            finals = [torch.stack(f, dim=0) for f in finals]
            for f in finals:
                f._itts_rows_own = True
            return out, finals

    def _recurrent_forward(self, input_, h0s, lengths):
        """The layers on the recurrence kernels: h0s = the initial states ((h_0, c_0) / (h_0,), each
        [num_layers*ndir, B, H] or None) -> (output, the final states, each [num_layers*ndir, B, H] in the
        caller's row order)."""
        ndir = 2 if self.bidirectional else 1
        if input_.shape[1 if self.batch_first else 0] == 1 and not all(_rows_share_state(h) for h in h0s) \
                and not (torch.is_grad_enabled() and (input_.requires_grad or any(
                    t.requires_grad for t in list(self.parameters()) + [h for h in h0s if h is not None]))):
            return self._step_forward(input_, h0s, lengths)
        pb, x = self._pack(input_, lengths, pad_cols=True)
        for h in h0s:
            _shared_initial_state(h)
        H = self.hidden_size
        # Every layer's operands are put together BEFORE the first recurrence is launched: the host waits for each
        # recurrence's verdict (rnn_persist.h), and what it still has to queue after that wait -- the stacking of
        # the two directions' weights, four small copies a layer -- stands between the recurrence and the next
        # layer's product on an idle device (90 us a layer boundary in the step's timeline).
        operands = []
        for layer in range(self.num_layers):
            # all rows share the initial state (init_hidden expands [.., 1, H]); use row 0
            states = [h[layer * ndir:(layer + 1) * ndir, 0, :] if h is not None else None for h in h0s]
            operands.append(_pad_hidden(
                self._stack("weight_ih", layer), self._stack("weight_hh", layer),
                [self._stack("bias_ih", layer), self._stack("bias_hh", layer)], states, self._gates, H, rows=pb.B,
                persistent=self._persistent))
        finals = []
        for layer, (w_ih, w_hh, (b_ih, b_hh), states, Hp) in enumerate(operands):
            x, *fin = self._layer_function.apply(x, pb, w_ih, w_hh, b_ih, b_hh, *states, torch.is_grad_enabled(),
                                                  *self._layer_extra)
            x = self._dropout(_unpad_rows(x, ndir, H, Hp), layer)
            finals.append(fin)
        out = pb.unpack(x, input_.shape)
        # back to the caller's row order, stacked over the layers
        return out, [StatesToCallerOrder.apply(pb.inv_perm, pb.perm, H, *[f[i] for f in finals])
                     for i in range(len(h0s))]


class LSTM(_RNNBase):
    """Drop-in for torch.nn.LSTM(input_size, hidden_size, num_layers, bidirectional, batch_first)
    as RNNWrapper uses it (rnn_dyn/RNNWrapper.py:45-54).  forward takes the padded tensor and
    the sequence lengths instead of a PackedSequence:
        output, (h_n, c_n) = lstm(padded, (h_0, c_0), lengths)
    with output zero-padded to the input's time extent (pad_packed_sequence(total_length=...))."""
    _gates = 4
    _layer_function = LSTMLayerFunction
    _cell_kind = ops.CELL_LSTM

    def forward(self, input_, hx=None, lengths=None):
        out, (hn, cn) = self._recurrent_forward(input_, hx if hx is not None else (None, None), lengths)
        return out, (hn, cn)


class GRU(_RNNBase):
    """Drop-in for torch.nn.GRU(input_size, hidden_size, num_layers, bidirectional, batch_first)
    as RNNWrapper uses it; same parameter names (weight_ih_l0[_reverse], ...), gate order r, z, n.
        output, h_n = gru(padded, h_0, lengths)"""
    _gates = 3
    _layer_function = GRULayerFunction
    _cell_kind = ops.CELL_GRU

    def forward(self, input_, hx=None, lengths=None):
        out, (hn,) = self._recurrent_forward(input_, (hx,), lengths)
        return out, hn


class RNN(_RNNBase):
    """Drop-in for torch.nn.RNN(input_size, hidden_size, num_layers, nonlinearity, bidirectional,
    batch_first) as RNNWrapper builds it for 'RNNTANH' / 'RNNRELU' groups (rnn_dyn/RNNWrapper.py:
    45-54, RNNDyn.py:268-272); same parameter names.
        output, h_n = rnn(padded, h_0, lengths)
    h_t = act(W_ih x_t + b_ih + b_hh + W_hh h_{t-1}): the input projection of all frames is one GEMM on packed rows,
    the recurrence runs on the step kernels of csrc/rnn_step.h (one launch per time step, both directions in it) at
    the hidden size rounded up to a multiple of 16.  Unlike LSTM / GRU, a loss may use h_n."""
    _layer_function = RNNLayerFunction
    _cell_kind = ops.CELL_RNN
    _persistent = False

    def __init__(self, input_size, hidden_size, num_layers=1, nonlinearity='tanh', bias=True,
                 batch_first=False, dropout=0.0, bidirectional=False):
        if nonlinearity.lower() not in ("tanh", "relu"):
            raise ValueError("Unknown nonlinearity '{}'".format(nonlinearity))
        super().__init__(input_size, hidden_size, num_layers, bias, batch_first, dropout, bidirectional)
        self.nonlinearity = nonlinearity.lower()

    @property
    def _layer_extra(self):
        return (ops.ACT_TANH if self.nonlinearity == "tanh" else ops.ACT_RELU,)

    def forward(self, input_, hx=None, lengths=None):
        out, (hn,) = self._recurrent_forward(input_, (hx,), lengths)
        return out, hn
