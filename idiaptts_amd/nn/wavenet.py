"""The WaveNet vocoder network (van den Oord et al. 2016; the architecture of r9y9's `wavenet_vocoder` package that the
reference's models/WaveNetWrapper.py wraps), written from the published architecture with the package's parameter
names and torch's [Cout, Cin, k] weight layout, so that a checkpoint of the package maps key for key.

Training composes the dense kernels that exist: every convolution is a Conv1dAct on channels-last rows [B, T, C], the
gate is csrc/wavenet.hip's kernel pair.  Generation is one launch of itts_wavenet_generate for the whole batch."""
import math
import warnings

import torch
from torch import nn

from .. import ops
from .functional import GluGateFunction
from .modules import Conv1dAct


def _conv(in_channels, out_channels, kernel_size, dropout, weight_normalization, dilation=1, bias=True):
    """a Conv1dAct drawn N(0, sqrt((1 - dropout) / (kernel_size * in_channels))) with zero bias, weight-normalised"""
    m = Conv1dAct(in_channels, out_channels, kernel_size, dilation=dilation, bias=bias, batch_first=True)
    nn.init.normal_(m.weight, mean=0.0, std=math.sqrt((1.0 - dropout) / (kernel_size * in_channels)))
    if m.bias is not None:
        nn.init.zeros_(m.bias)
    if weight_normalization:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")             # (the weight_g / weight_v names are the point)
            m = nn.utils.weight_norm(m)
    return m


def effective_weight(conv):
    """the weight a convolution computes with: g v / |v| under weight norm, else the parameter"""
    if hasattr(conv, "weight_g"):
        return torch._weight_norm(conv.weight_v, conv.weight_g, 0)
    return conv.weight


class ResidualLayer(nn.Module):
    """conv (dilated, causal) -> + conv1x1c(c) -> tanh * sigmoid -> conv1x1_skip, conv1x1_out + residual"""

    def __init__(self, residual_channels, gate_channels, kernel_size, skip_out_channels, cin_channels, dropout,
                 dilation, weight_normalization):
        super().__init__()
        self.dropout = dropout
        self.left_pad = (kernel_size - 1) * dilation
        self.conv = _conv(residual_channels, gate_channels, kernel_size, dropout, weight_normalization,
                          dilation=dilation)
        if cin_channels > 0:
            self.conv1x1c = _conv(cin_channels, gate_channels, 1, dropout, weight_normalization, bias=False)
        else:
            self.conv1x1c = None
        self.conv1x1_out = _conv(gate_channels // 2, residual_channels, 1, dropout, weight_normalization)
        self.conv1x1_skip = _conv(gate_channels // 2, skip_out_channels, 1, dropout, weight_normalization)

    def forward(self, x, c):
        """x [B, T, R], c [B, T, cin] or None -> (x' [B, T, R], skip [B, T, S])"""
        h = nn.functional.dropout(x, p=self.dropout, training=self.training)
        # causal: (kernel_size - 1) * dilation zeros in front, so that exactly the first T outputs are computed
        h = self.conv(nn.functional.pad(h, (0, 0, self.left_pad, 0)))
        z = GluGateFunction.apply(h, self.conv1x1c(c) if self.conv1x1c is not None else None)
        return (self.conv1x1_out(z) + x) * math.sqrt(0.5), self.conv1x1_skip(z)


class WaveNet(nn.Module):
    """first_conv -> conv_layers (dilation 2 ** (l % (layers // stacks))) -> summed skips -> last_conv_layers.
    forward(x, c) is the teacher-forced pass: x [B, out_channels, T] one-hot (or [B, 1, T] with scalar_input), c
    [B, cin_channels, T] at the sample rate -> [B, out_channels, T]; position t predicts sample t + 1.
    generate(c, lengths, ...) draws the samples on the device, whole batches in one launch."""

    def __init__(self, out_channels=256, layers=20, stacks=2, residual_channels=512, gate_channels=512,
                 skip_out_channels=512, kernel_size=3, dropout=1 - 0.95, cin_channels=-1, gin_channels=-1,
                 n_speakers=None, weight_normalization=True, upsample_conditional_features=False,
                 upsample_scales=None, freq_axis_kernel_size=3, scalar_input=False, use_speaker_embedding=False,
                 legacy=False, log_scale_min=-7.0):
        super().__init__()
        if upsample_conditional_features:
            raise NotImplementedError("WaveNet upsample_conditional_features=True is not implemented: bring the "
                                      "conditioning to the sample rate with misc.utils.sample_linearly_batch.")
        if gin_channels is not None and gin_channels > 0:
            raise NotImplementedError("WaveNet gin_channels={}: global conditioning is not implemented."
                                      .format(gin_channels))
        if use_speaker_embedding:
            raise NotImplementedError("WaveNet use_speaker_embedding=True: global conditioning is not implemented.")
        if legacy:
            raise NotImplementedError("WaveNet legacy=True (skip outputs scaled per layer) is not implemented.")
        if stacks < 1 or layers % stacks != 0:
            raise ValueError("WaveNet layers={} must be a multiple of stacks={}.".format(layers, stacks))
        cin_channels = max(int(cin_channels), 0)
        self.dilations = [2 ** (l % (layers // stacks)) for l in range(layers)]
        ops.wavenet_check_envelope(layers, self.dilations, kernel_size, residual_channels, gate_channels,
                                   skip_out_channels, cin_channels, out_channels, scalar_input)
        self.out_channels, self.scalar_input = out_channels, bool(scalar_input)
        self.cin_channels, self.kernel_size = cin_channels, kernel_size
        self.residual_channels, self.gate_channels = residual_channels, gate_channels
        self.skip_out_channels = skip_out_channels
        self.log_scale_min = float(log_scale_min)
        wn = weight_normalization
        self.first_conv = _conv(1 if scalar_input else out_channels, residual_channels, 1, dropout, wn)
        self.conv_layers = nn.ModuleList(
            ResidualLayer(residual_channels, gate_channels, kernel_size, skip_out_channels, cin_channels, dropout, d,
                          wn)
            for d in self.dilations)
        self.last_conv_layers = nn.ModuleList([
            nn.ReLU(), _conv(skip_out_channels, skip_out_channels, 1, dropout, wn),
            nn.ReLU(), _conv(skip_out_channels, out_channels, 1, dropout, wn)])

    @property
    def receptive_field(self):
        return 1 + (self.kernel_size - 1) * sum(self.dilations)

    def forward(self, x, c=None, g=None, softmax=False):
        if g is not None:
            raise NotImplementedError("WaveNet g: global conditioning is not implemented.")
        if softmax:
            raise NotImplementedError("WaveNet softmax=True is not implemented: the losses take logits.")
        if x.dim() != 3 or x.shape[1] != (1 if self.scalar_input else self.out_channels):
            raise ValueError("WaveNet input must be [B, {}, T], got {}.".format(
                1 if self.scalar_input else self.out_channels, tuple(x.shape)))
        if self.cin_channels > 0:
            if c is None or c.dim() != 3 or c.shape[1] != self.cin_channels or c.shape[2] != x.shape[2]:
                raise ValueError("WaveNet conditioning must be [B, {}, T = {}], got {}.".format(
                    self.cin_channels, x.shape[2], None if c is None else tuple(c.shape)))
            c = c.transpose(1, 2).contiguous()           # channels-last once, for every layer
        else:
            c = None
        h = self.first_conv(x.transpose(1, 2).contiguous())
        skips = None
        for layer in self.conv_layers:
            h, s = layer(h, c)
            skips = s if skips is None else skips + s
        h = skips
        for m in self.last_conv_layers:
            h = m(h)
        return h.transpose(1, 2)

    def generation_weights(self):
        """ops.WaveNetWeights: the effective (weight-normalised) weights as the generation kernel's images.  Reads
        the parameters and leaves them alone: weight norm stays in place, training may go on afterwards."""
        with torch.no_grad():
            k, R, G = self.kernel_size, self.residual_channels, self.gate_channels
            S, cin, C = self.skip_out_channels, self.cin_channels, self.out_channels
            ka = k * R + (cin + 15) // 16 * 16
            w1, b1, w2, b2 = [], [], [], []
            for layer in self.conv_layers:
                w = effective_weight(layer.conv).float()                        # [G, R, k]
                rows = [w.permute(2, 1, 0).reshape(k * R, G)]                   # row j R + r = tap j, channel r
                if layer.conv1x1c is not None:
                    rows.append(effective_weight(layer.conv1x1c).float()[:, :, 0].t())
                w1.append(ops.wavenet_pack(torch.cat(rows, 0), ka, G))
                b1.append(layer.conv.bias.float())
                wo = effective_weight(layer.conv1x1_out).float()[:, :, 0]      # [R, H]
                ws = effective_weight(layer.conv1x1_skip).float()[:, :, 0]     # [S, H]
                w2.append(ops.wavenet_pack(torch.cat([wo, ws], 0).t(), G // 2, R + S))
                b2.append(torch.cat([layer.conv1x1_out.bias.float(), layer.conv1x1_skip.bias.float()]))
            h1, h2 = self.last_conv_layers[1], self.last_conv_layers[3]
            cpad = (C + 15) // 16 * 16
            bh2 = torch.zeros(cpad, dtype=torch.float32, device=h2.bias.device)
            bh2[:C] = h2.bias.float()
            return ops.WaveNetWeights(
                wf=effective_weight(self.first_conv).float()[:, :, 0].t().contiguous(),
                bf=self.first_conv.bias.float().contiguous(),
                w1=torch.cat(w1), b1=torch.cat(b1), w2=torch.cat(w2), b2=torch.cat(b2),
                wh1=ops.wavenet_pack(effective_weight(h1).float()[:, :, 0].t(), S, S), bh1=h1.bias.float().contiguous(),
                wh2=ops.wavenet_pack(effective_weight(h2).float()[:, :, 0].t(), S, cpad), bh2=bh2,
                dilations=tuple(self.dilations), kernel_size=k, residual_channels=R, gate_channels=G,
                skip_out_channels=S, cin_channels=cin, out_channels=C, scalar_input=self.scalar_input,
                log_scale_min=self.log_scale_min)

    def generate(self, c, lengths, uniforms=None, generator=None, return_logits=False, initial_class=None):
        """lengths[b] samples of every row b, drawn step by step on the device (itts_wavenet_generate).
        c [B, cin_channels, T] conditioning at the sample rate (None without conditioning), T >= max(lengths).
        uniforms: the numbers the draws use, [B, max(lengths)] (classes) or [B, max(lengths), 2] (scalar input:
        mixture choice, logistic), float32 in (0, 1); None draws them with torch.rand and `generator`.  The kernel
        draws nothing itself: the result is a pure function of the arguments.
        Returns the class indices [B, max(lengths)] (int32), or with scalar_input the samples (float32), zeros past
        each row's length; with return_logits also the network outputs [B, max(lengths), out_channels]."""
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        dev = self.first_conv.bias.device
        T = max(lengths) if lengths else 0
        if uniforms is None:
            shape = (len(lengths), T, 2) if self.scalar_input else (len(lengths), T)
            uniforms = torch.rand(shape, generator=generator, device=dev, dtype=torch.float32)
            if self.scalar_input:
                uniforms = uniforms * (1.0 - 2e-5) + 1e-5            # the logistic draw takes log u and log(1 - u)
        if self.cin_channels > 0:
            if c is None or c.dim() != 3 or c.shape[1] != self.cin_channels:
                raise ValueError("WaveNet conditioning must be [B, {}, T], got {}.".format(
                    self.cin_channels, None if c is None else tuple(c.shape)))
            c = c.to(dev, torch.float32).transpose(1, 2).contiguous()
        else:
            c = None
        return ops.wavenet_generate(self.generation_weights(), c, lengths, uniforms.to(dev),
                                    initial_class=-1 if initial_class is None else int(initial_class),
                                    return_logits=return_logits)
