"""The reference's models/WaveNetWrapper.py on this package's own WaveNet (idiaptts_amd.nn.WaveNet): the same Config,
IDENTIFIER and forward contract.  The reference wraps r9y9's external `wavenet_vocoder` package, which is not part of
its tree; the network here is written from the published architecture with the package's parameter names, so a
checkpoint maps key for key (parity with the package itself -- initial values, bits, a skip scaling of its non-legacy
path -- is not pinned: neither the package nor a checkpoint of it is available to the tests).

Differences from the reference, both on purpose:
  * inference takes batches (the reference asserts "Batch synth is not supported") and runs as one kernel launch;
  * inference reads the effective weights and leaves weight norm in place (the reference calls
    make_generation_fast_(), after which training cannot continue): `has_weight_norm` stays True."""
import numpy as np
import torch
import torch.nn as nn

from idiaptts_amd import ops
from idiaptts_amd.nn.wavenet import WaveNet


class WaveNetWrapper(nn.Module):
    IDENTIFIER = "r9y9WaveNet"

    class Config:
        INPUT_TYPE_MULAW = "mulaw-quantize"
        INPUT_TYPE_RAW = "raw"
        # what the network takes of a Config, by the names of WaveNet's arguments
        MODEL_FIELDS = ("out_channels", "layers", "stacks", "residual_channels", "gate_channels", "skip_out_channels",
                        "kernel_size", "dropout", "weight_normalization", "cin_channels", "gin_channels", "n_speakers",
                        "upsample_conditional_features", "upsample_scales", "freq_axis_kernel_size", "scalar_input",
                        "use_speaker_embedding", "legacy")

        def __init__(self, cin_channels=80, dropout=0.05, freq_axis_kernel_size=3, gate_channels=512, gin_channels=-1,
                     hinge_regularizer=True, kernel_size=3, layers=24, log_scale_min=float(np.log(1e-14)),
                     n_speakers=1, out_channels=256, residual_channels=512, scalar_input=False, skip_out_channels=256,
                     stacks=4, upsample_conditional_features=False, upsample_scales=[5, 4, 2],
                     use_speaker_embedding=False, weight_normalization=True, legacy=False):
            # out_channels: the classes of mu-law input, or 3 * mixtures (logit, mean, log-scale) for INPUT_TYPE_RAW,
            # which also takes scalar_input=True; hinge_regularizer and log_scale_min belong to the MoL loss.
            # (scalar_input's default is the package's is_scalar_input(INPUT_TYPE_MULAW), which is False.)
            fields = dict(locals())
            del fields["self"]
            for name, value in fields.items():
                setattr(self, name, value)

        def create_model(self):
            return WaveNetWrapper(self)

    def __init__(self, config):
        super().__init__()
        self.len_in_out_multiplier = 1
        self.model = WaveNet(**{name: getattr(config, name) for name in config.MODEL_FIELDS})
        self.has_weight_norm = True

    def _lengths(self, seq_lengths):
        lengths = seq_lengths.tolist() if torch.is_tensor(seq_lengths) else list(seq_lengths)
        return [int(n) * int(self.len_in_out_multiplier) for n in lengths]

    def forward(self, input_, target, seq_lengths, *_, uniforms=None, generator=None):

        if target is not None:  # During training and testing with teacher forcing.
            output = self.model(target, c=input_, g=None, softmax=False)
            # Output shape is B x C x T, as CrossEntropyLoss requires it.
        else:  # During inference: seq_lengths[b] * len_in_out_multiplier samples per row.
            with torch.no_grad():
                lengths = self._lengths(seq_lengths)
                out = self.model.generate(input_, lengths, uniforms=uniforms, generator=generator)
                if self.model.scalar_input:
                    output = out.unsqueeze(1)                                   # B x 1 x T samples
                else:                                                           # B x C x T one-hot
                    output = nn.functional.one_hot(out.long(), self.model.out_channels).transpose(1, 2).float()
                    live = torch.arange(out.shape[1], device=out.device)[None, :] < torch.tensor(
                        lengths, device=out.device)[:, None]
                    output = output * live.unsqueeze(1)

        return output, None

    def generate_waveform(self, input_, seq_lengths, uniforms=None, generator=None):
        """The generated waveforms, one float64 tensor per row: the mu-law classes decoded by ops.mulaw_decode
        (RawWaveformLabelGen.mu_law_companding_reversed), or the samples themselves with scalar input."""
        with torch.no_grad():
            lengths = self._lengths(seq_lengths)
            out = self.model.generate(input_, lengths, uniforms=uniforms, generator=generator)
            rows = [out[b, :n] for b, n in enumerate(lengths)]
            if self.model.scalar_input:
                return [r.double() for r in rows]
            offsets = [0]
            for n in lengths:
                offsets.append(offsets[-1] + n)
            flat = ops.mulaw_decode(torch.cat(rows).long(), offsets, mu=self.model.out_channels - 1)
            return [flat[offsets[b]:offsets[b + 1]] for b in range(len(lengths))]

    def set_gpu_flag(self, use_gpu):
        self.use_gpu = use_gpu

    def init_hidden(self, batch_size=1):
        return None

    def parameters(self):
        return self.model.parameters()


class WaveNetVocoder(nn.Module):
    """The wrapper as a dict-in / dict-out module, the form ModularModelHandlerPyTorch drives
    (`model(data, lengths, max_lengths)`; the reference has no such module: its WaveNetVocoderTrainer predates the
    modular handler).  `data[input_names[0]]` is the conditioning [B, cin, T] at the sample rate (not read when the
    network has cin_channels 0), `data[target_name]` the one-hot / scalar target [B, C, T]; the logits [B, out_channels,
    T] go to `data[output_names[0]]` with the target's lengths.  `inference` generates lengths[input_names[0]] *
    len_in_out_multiplier samples a row and writes what WaveNetWrapper.forward(target=None) returns.
    The state dict is the wrapper's under `model.` (`model.model.first_conv.weight_g`, ...)."""

    class Config:
        def __init__(self, wavenet_config, input_names=None, target_name="target", output_names=None,
                     name="WaveNetVocoder", batch_first=True):
            self.wavenet_config = wavenet_config
            self.input_names = ["conditioning"] if input_names is None else list(input_names)
            self.target_name = target_name
            self.output_names = ["pred_target"] if output_names is None else list(output_names)
            self.name = name
            self.batch_first = batch_first

        def create_model(self):
            return WaveNetVocoder(self)

    def __init__(self, config):
        super().__init__()
        if not config.batch_first:
            raise NotImplementedError("WaveNetVocoder batch_first=False is not implemented: the network takes "
                                      "[B, C, T].")
        if len(config.input_names) != 1 or len(config.output_names) != 1:
            raise ValueError("WaveNetVocoder takes one input name (the conditioning) and one output name, got {} and "
                             "{}.".format(config.input_names, config.output_names))
        self.config = config
        self.input_names, self.output_names = list(config.input_names), list(config.output_names)
        self.target_name, self.name, self.batch_first = config.target_name, config.name, config.batch_first
        self.model = config.wavenet_config.create_model()

    @property
    def use_cond(self):
        return self.model.model.cin_channels > 0

    def init_hidden(self, batch_size=1):
        return None

    def _write(self, data, lengths, max_lengths, output, like):
        name = self.output_names[0]
        data[name] = output
        lengths[name] = lengths[like]
        max_lengths[name] = max_lengths[like] if like in max_lengths else output.shape[2]

    def forward(self, data, lengths, max_lengths, **kwargs):
        target = data.get(self.target_name)
        if target is None:
            return self.inference(data, lengths, max_lengths, **kwargs)
        cond = data[self.input_names[0]] if self.use_cond else None
        output, _ = self.model(cond, target, lengths[self.target_name])
        self._write(data, lengths, max_lengths, output, self.target_name)

    def inference(self, data, lengths, max_lengths, uniforms=None, generator=None):
        first = self.input_names[0]
        cond = data[first] if self.use_cond else None
        output, _ = self.model(cond, None, lengths[first], uniforms=uniforms, generator=generator)
        name = self.output_names[0]
        data[name] = output
        lengths[name] = torch.as_tensor(self.model._lengths(lengths[first]), dtype=torch.long)
        max_lengths[name] = output.shape[2]


# (the adapter's config by the wrapper's name as well: WaveNetWrapper.NamedConfig(wavenet_config, ...))
WaveNetWrapper.NamedConfig = WaveNetVocoder.Config
