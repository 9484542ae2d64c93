"""The frame-rate decoder of an encoder-decoder model behind a fixed attention (the reference's
models/enc_dec_dyn/DecoderModule.py:82-327): the phoneme-rate inputs are merged, turned into one context per decoder
step by the attention matrix of the durations (csrc/fixed_attention.hip), and -- for an autoregressive decoder --
concatenated with the pre-net's view of the previous output frame, run through the rnn_dyn model and projected; a step
emits `n_frames_per_step` frames.

Batched pass: without teacher-forcing names, or with a target and p_teacher_forcing == 1.0.  One attention launch,
the go frame plus the shifted target through the pre-net, the model and the projections on the whole sequence.
Iterative pass: the reference's loop -- one np.random.uniform draw per step after the first and only with a target,
so a seeded run makes the reference's choices; pre-net, model and projections on one frame, the last projected frame
fed back; the recurrent groups step on the states their previous call left (nn/modules.py: _step_forward).  The
contexts of all ceil(T / n) steps come from ONE attention launch in front of the loop, which slices them: the fixed
context does not depend on the decoder's state.

Parameter keys are the reference's: `<name>.model.*`, `<name>.pre_net.*`, `<name>.<name>_<projector name>.model.*`.

Deviations from the reference:
  * the iterative pass with gradients enabled raises NotImplementedError (p_teacher_forcing < 1 needs gradients
    through the feedback loop; run it under torch.no_grad()); the reference trains through it;
  * the last step of the iterative pass over T frames with T % n != 0 takes the mean of the rows the attention
    matrix has left (as the reference); steps beyond the matrix cannot occur (the reference returns NaN for an empty
    slice);
  * without projections the reference's loop fails (torch.cat of an empty list); here the model's output of every
    step is written under output_names[0], as the batched pass does;
  * an autoregressive decoder none of whose projections is fed back raises NotImplementedError in the iterative pass
    (the reference fails on a go frame of width None);
  * a DecoderConfig whose input_names is a plain string reads that one feature (the reference's ModelConfig makes
    a list of it; nothing indexes single letters);
  * an attention matrix that arrives as a Python list (ragged [T, P] matrices: no reader of the reference pads them)
    raises a TypeError naming the collation hook PhonemeDurationLabelGen.unsorted_pad_sequence;
  * a DecoderConfig whose attention_config is not FIXED_ATTENTION (the default None included) raises
    NotImplementedError when it is constructed (the reference builds a decoder without attention, which fails in its
    first forward); a ProjectionConfig given input_names raises NotImplementedError (a TypeError in the reference);
  * the lengths of the one-frame calls inside the loop are kept on the host."""
import logging
import math

import numpy as np
import torch

from idiaptts_amd.nn.functional import padding_rows_identical

from . import ATTENTION_GROUND_TRUTH, FIXED_ATTENTION
from .EncDecDyn import SubModule, _PassThrough
from .attention.FixedAttention import FixedAttention


class ProjectionModule(SubModule):
    """a SubModule without input names: DecoderModule hands it the decoder's output"""

    def __init__(self, config):
        super().__init__(config)
        self.is_autoregressive_input = config.is_autoregressive_input
        self.out_dim = config.out_dim

    def forward_module(self, input_, lengths, max_lengths):
        """the reference's SubModule.forward_module for input_names None: the model sees no lengths"""
        if isinstance(self.model, _PassThrough):
            return input_
        output, _ = self.model(input_, seq_lengths_input=None, max_length_inputs=None)
        return output

    def forward(self, data, lengths, max_lengths, **kwargs):
        raise RuntimeError("Projection {} has no inputs of its own: it runs inside its DecoderModule.".format(self.name))


def _clamp(value, **kwargs):
    return value.clamp(**kwargs) if torch.is_tensor(value) else int(torch.tensor(value).clamp(**kwargs))


class DecoderModule(SubModule):

    def __init__(self, config):
        if config.attention_config != FIXED_ATTENTION:
            raise NotImplementedError("enc_dec_dyn.Config.DecoderConfig(attention_config={!r}): only {!r} is "
                                      "implemented (learned attention is a separate piece of work)."
                                      .format(config.attention_config, FIXED_ATTENTION))
        if ATTENTION_GROUND_TRUTH not in (config.attention_args or {}):
            raise ValueError("DecoderConfig {}: attention_args must name the attention matrix, "
                             "{{enc_dec_dyn.ATTENTION_GROUND_TRUTH: <feature name>}}.".format(config.name))
        super().__init__(config)
        self.attention_args = config.attention_args
        self.attention_config = config.attention_config
        self.attention = FixedAttention.Config(config.attention_args[ATTENTION_GROUND_TRUTH],
                                               config.n_frames_per_step).create_model()
        self.n_frames_per_step = config.n_frames_per_step
        self.p_teacher_forcing = config.p_teacher_forcing
        self.teacher_forcing_input_names = config.teacher_forcing_input_names
        self.has_model = not isinstance(self.model, _PassThrough)

        self.pre_net = config.pre_net_config.create_model() if config.pre_net_config is not None else None
        self.projections = []
        for projection_config in config.projection_configs or ():
            projector = projection_config.create_model()
            projector_id = "{}_{}".format(self.name, projector.name)
            logging.debug("Adding {} to {}".format(projector_id, self.name))
            self.add_module(projector_id, projector)
            self.projections.append(projector)

        # the width of the frame fed back: the autoregressive projections', else the model's (reference :51-67)
        self.decoder_dim = None
        if config.projection_configs is not None:
            dims = [c.out_dim for c in config.projection_configs if c.is_autoregressive_input]
            if len(dims) > 0:
                self.decoder_dim = sum(dims)
        else:
            try:
                self.decoder_dim = self.model[-1].out_dim
            except (AttributeError, TypeError, IndexError):
                if self.is_autoregressive:
                    raise ValueError("Cannot infer decoder output dimension.")
        self.decoder_output_name = getattr(config, "decoder_output_name", None)

    @property
    def is_autoregressive(self):
        return self.teacher_forcing_input_names is not None

    @property
    def extra_input_names(self):
        """what the module reads besides input_names at synthesis time: the attention matrix"""
        return [self.attention.attention_ground_truth]

    def init_hidden(self, batch_size=1):
        super().init_hidden(batch_size)
        if self.pre_net is not None:
            self.pre_net.init_hidden(batch_size)
        for projector in self.projections:
            projector.init_hidden(batch_size)

    def _get_inputs(self, data, names, merge_type):
        """NamedForwardModule._get_inputs, batch_first"""
        inputs = [data[name] for name in names]
        extents = [i.shape[1] for i in inputs if i.dim() > 2]
        longest = max(extents) if extents else 1
        inputs = [self._over_time(i, longest, True) for i in inputs]
        return inputs[0] if len(inputs) == 1 else self.merge(inputs, merge_type, True)

    def forward(self, data, lengths, max_lengths, **kwargs):
        input_ = self._get_inputs(data, self.input_names, self.input_merge_type)
        target = None
        if self.is_autoregressive and all(name in data for name in self.teacher_forcing_input_names):
            target = self._get_inputs(data, self.teacher_forcing_input_names, "cat")
        attention_matrix = data[self.attention.attention_ground_truth]
        if isinstance(attention_matrix, (list, tuple)):
            raise TypeError("The attention matrix {} arrived as a list of per-utterance matrices: its data reader has "
                            "to pad the batch (PhonemeDurationLabelGen.unsorted_pad_sequence, called by the handler's "
                            "prepare_batch).".format(self.attention.attention_ground_truth))
        # (computed tensors: nobody vouches for one common row at the padding positions)
        with padding_rows_identical(False):
            if self.attention.allows_batched_forward() \
                    and (self.teacher_forcing_input_names is None
                         or (target is not None and self.p_teacher_forcing == 1.0)):
                outputs = self._forward_batched(input_, target, lengths, max_lengths, attention_matrix)
            else:
                outputs = self._forward_iterative(input_, target, lengths, max_lengths, attention_matrix)
        output_dict, output_lengths, output_max_lengths = outputs
        lengths.update(output_lengths)
        max_lengths.update(output_max_lengths)
        data.update(output_dict)

    def inference(self, data, lengths, max_lengths, *args, **kwargs):
        """NamedForwardModule.inference (:61-77): the teacher-forcing names are hidden from the module and stay in
        the caller's dictionaries"""
        if not self.is_autoregressive:
            return self.forward(data, lengths, max_lengths, *args, **kwargs)
        hidden = self.teacher_forcing_input_names
        filtered = [{k: v for k, v in d.items() if k not in hidden} for d in (data, lengths, max_lengths)]
        self.forward(*filtered, *args, **kwargs)
        for d, f in zip((data, lengths, max_lengths), filtered):
            d.update(f)

    def _run_model(self, input_, seq_lengths, max_length):
        return self.model(input_, seq_lengths_input=seq_lengths, max_length_inputs=max_length)

    def _forward_batched(self, input_, target, lengths, max_lengths, attention_matrix):
        n = self.n_frames_per_step
        lengths = {k: v // n for k, v in lengths.items()}
        max_lengths = {k: v // n for k, v in max_lengths.items()}
        ground_truth = self.attention.attention_ground_truth
        output_dict, output_lengths_dict, output_max_lengths_dict = {}, {}, {}

        input_, attention = self.attention.forward_batched(input_, attention_matrix)
        output_lengths, output_max_lengths = lengths[ground_truth], max_lengths[ground_truth]
        output_dict["attention"] = attention
        output_lengths_dict["attention"] = lengths[ground_truth]
        output_max_lengths_dict["attention"] = max_lengths[ground_truth]

        if self.is_autoregressive:
            first = self.teacher_forcing_input_names[0]
            teacher_forcing_target = self._get_teacher_forcing_target(target)
            if self.pre_net is not None:
                teacher_forcing_target, _ = self.pre_net(teacher_forcing_target, seq_lengths_input=lengths[first],
                                                         max_length_inputs=max_lengths[first])
            input_ = torch.cat((input_, teacher_forcing_target), dim=2)

        if not self.has_model:
            decoder_output = input_
        else:
            key = self.teacher_forcing_input_names[0] if self.is_autoregressive else ground_truth
            decoder_output, kwargs = self._run_model(input_, lengths[key], max_lengths[key])
            output_lengths, output_max_lengths = kwargs["seq_lengths_input"], kwargs["max_length_inputs"]

        if self.decoder_output_name is not None:
            output_dict[self.decoder_output_name] = decoder_output
            output_lengths_dict[self.decoder_output_name] = output_lengths
            output_max_lengths_dict[self.decoder_output_name] = output_max_lengths

        if len(self.projections) > 0:
            for projector in self.projections:
                name = projector.output_names[0]
                output_dict[name] = self._parse_outputs(projector.forward_module(decoder_output, lengths, max_lengths))
                output_lengths_dict[name] = output_lengths * n
                output_max_lengths_dict[name] = output_max_lengths * n
        else:
            name = self.output_names[0]
            output_dict[name] = decoder_output
            output_lengths_dict[name] = output_lengths * n
            output_max_lengths_dict[name] = output_max_lengths * n
        return output_dict, output_lengths_dict, output_max_lengths_dict

    def _get_teacher_forcing_target(self, target):
        n = self.n_frames_per_step
        shifted_target = target[:, n - 1::n][:, :-1]
        return torch.cat((self._get_go_frame(target), shifted_target), dim=1)

    def _get_go_frame(self, input_):
        return input_.new_zeros(input_.shape[0], 1, self.decoder_dim)

    def _parse_outputs(self, decoder_outputs):
        B, T = decoder_outputs.shape[:2]
        return decoder_outputs.reshape(B, T * self.n_frames_per_step, -1)

    def _forward_iterative(self, input_, target, lengths, max_lengths, attention_matrix):
        if torch.is_grad_enabled() and (input_.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(
                "Decoder {}: the iterative pass (p_teacher_forcing < 1, here {}, or no teacher-forcing input) under "
                "gradients is not implemented; run it inside torch.no_grad(), or train with p_teacher_forcing = 1.0."
                .format(self.name, self.p_teacher_forcing))
        if self.is_autoregressive and self.decoder_dim is None:
            raise NotImplementedError("Decoder {}: no projection is an autoregressive input, there is no frame to feed "
                                      "back.".format(self.name))
        n = self.n_frames_per_step
        B = input_.shape[0]
        ones = torch.ones(B, dtype=torch.long)
        max_steps = target.shape[1] if target is not None else attention_matrix.shape[1]
        steps = math.ceil(max_steps / n)
        if steps > math.ceil(attention_matrix.shape[1] / n):
            raise ValueError("Decoder {}: {} frames to decode, but the attention matrix {} has {}."
                             .format(self.name, max_steps, self.attention.attention_ground_truth,
                                     attention_matrix.shape[1]))
        all_outputs = {}
        # every step's context in one launch: it does not depend on the decoder's state
        contexts, attention = self.attention.forward_all_steps(input_, attention_matrix)
        contexts, attention = contexts[:, :steps], attention[:, :steps]

        decoder_input = self._get_go_frame(input_) if self.is_autoregressive else None
        last_projector_outputs = None
        for i in range(steps):
            step_input = contexts[:, i:i + 1]
            if self.is_autoregressive:
                if i > 0:
                    if target is not None and np.random.uniform(0.0, 1.0) <= self.p_teacher_forcing:
                        decoder_input = target[:, i * n - 1:i * n]          # teacher forcing
                    else:
                        decoder_input = last_projector_outputs[:, -1:]      # auto-regression
                if self.pre_net is not None:
                    decoder_input, _ = self.pre_net(decoder_input, seq_lengths_input=ones, max_length_inputs=1)
                step_input = torch.cat((step_input, decoder_input), dim=-1)
            if self.has_model:
                decoder_output, _ = self._run_model(step_input, ones, 1)
            else:
                decoder_output = step_input
            if self.decoder_output_name is not None:
                all_outputs.setdefault(self.decoder_output_name, []).append(decoder_output)
            fed_back = []
            for projector in self.projections:
                projector_output = self._parse_outputs(projector.forward_module(decoder_output, lengths, max_lengths))
                all_outputs.setdefault(projector.output_names[0], []).append(projector_output)
                if projector.is_autoregressive_input:
                    fed_back.append(projector_output)
            if fed_back:
                last_projector_outputs = torch.cat(fed_back, dim=-1)
            if not self.projections and self.decoder_output_name != self.output_names[0]:
                all_outputs.setdefault(self.output_names[0], []).append(decoder_output)

        outputs = {name: torch.cat(values, dim=1) for name, values in all_outputs.items()}
        outputs["attention"] = attention

        # the lengths of the outputs, clamped as in the reference (:296-325)
        ground_truth = self.attention.attention_ground_truth
        if lengths is not None and self.is_autoregressive and self.teacher_forcing_input_names[0] in lengths:
            first = self.teacher_forcing_input_names[0]
            len_ = _clamp(lengths[first], max=max_steps)
            max_len = _clamp(max_lengths[first], min=max_steps)
        elif ground_truth in lengths:
            len_ = _clamp(lengths[ground_truth], max=max_steps)
            max_len = _clamp(max_lengths[ground_truth], max=max_steps)
        else:
            len_ = max_len = torch.full((B,), max_steps, dtype=torch.long)
        output_lengths, output_max_lengths = {}, {}
        for name in outputs:
            output_lengths[name], output_max_lengths[name] = len_, max_len
        output_lengths["attention"] = len_ // n
        output_max_lengths["attention"] = max_len // n
        return outputs, output_lengths, output_max_lengths
