"""RNNDyn and its layer-group wrappers on the HIP kernels
(reference: rnn_dyn/RNNDyn.py:26-147, FFWrapper.py:37-88, RNNWrapper.py:45-107, CNNWrapper.py,
TransposingWrapper.py).

state_dict() keys and shapes equal the reference's, so its checkpoints load unchanged:
FF group `<i>.module.<k>.weight/bias` with k = index of the Linear (or LayerNorm) inside the nn.Sequential
(non-linearity / dropout modules keep their slots), VAE group `<i>.module.0.linear.weight` (pooling groups have no
parameters), RNN group `<i>.module.weight_ih_l0[_reverse]`, `<i>.h_0`, `<i>.c_0`, Conv1d group `<i>.module.<k>.weight/bias` as FF groups,
TransformerEncoderLayer group `<i>.module.<k>.self_attn.in_proj_weight`, `.self_attn.out_proj.weight`, `.linear1`, `.linear2`,
`.norm1`, `.norm2` with k = index of the block; the group index starts at 1
because `emb_groups` takes slot 0 of the ModuleList.
"""
import copy

import torch
from torch import nn

from idiaptts_amd import ops
from idiaptts_amd.nn.functional import (ChainDropout, DropoutFunction, LinearChainFunction, ValidRows,
                                        default_dropout_stream, padding_is_identical, padding_rows_identical)
from idiaptts_amd.nn.modules import (GRU, LSTM, RNN, Conv1dAct, LayerNormAct, LinearAct, MeanPooling, SelectLastPooling,
                                     TransformerEncoderLayer, VanillaVAE)

# the torch.nn activations a Linear group fuses (default arguments, as the reference's `getattr(nn, nonlin)()`)
LINEAR_NONLINS = tuple(ops.ACT_TORCH_NAME.values())
# the special FFWrapper types built here (reference FFWrapper.py:43-48); their keyword arguments pass through
POOL_TYPES = {"PoolLast": SelectLastPooling, "PoolMean": MeanPooling}
VAE_TYPES = ("VAE", "VanillaVAE")


class FusedActivation(nn.Identity):
    """Keeps the activation's slot (Tanh, ReLU, Sigmoid, ...) of the reference's nn.Sequential; the activation
    itself is applied in the epilogue of the preceding LinearAct / Conv1dAct GEMM, or by the preceding LayerNormAct's
    row kernel."""

    def __init__(self, name):
        super().__init__()
        self.name = name

    def extra_repr(self):
        return "{} (fused into the previous layer)".format(self.name)


class Dropout(nn.Dropout):
    """The nn.Dropout slot of the reference's nn.Sequential (same state-dict layout: no parameters).  In training, on
    float32 device tensors and for 0 < p < 1, the mask comes from the counter rule of csrc/dropout.h -- (seed, salt,
    position) -- instead of torch's generator: the same distribution and scaling, other masks.  `salt` is the index
    in the model of the layer in front (RNNDyn numbers them); the seed of a forward is handed over by the group
    (FFWrapper.forward_dropout) or drawn from the package's stream.  Everything else is torch's module."""

    salt = 0
    seed = None          # of the group's current forward

    def fused(self, x):
        return self.training and 0.0 < self.p < 1.0 and x.is_cuda and x.dtype == torch.float32 and not self.inplace

    def forward(self, x):
        if not self.fused(x) or x.dim() < 2:
            return super().forward(x)
        seed = self.seed if self.seed is not None else default_dropout_stream().next()
        return DropoutFunction.apply(x, self.p, seed, self.salt)


def run_linear_chain(rows, layers, drops=None, seed=0):
    """rows -> the layers' output rows through one autograd node (nn/functional.py: LinearChainFunction); drops: per
    layer (p, salt) of the dropout behind it, with one seed for the call"""
    flat = []
    for m in layers:
        flat += [m.weight, m.bias]
    acts = tuple(m.act for m in layers)
    if drops is not None:
        acts = ChainDropout(acts, tuple(drops), seed)
    return LinearChainFunction.apply(rows, acts, *flat)


class FFWrapper(nn.Module):
    # a padded batch is computed on its valid rows when at least this share of its positions is padding (packing and
    # unpacking are two more passes over the rows; an LJSpeech batch of 32 utterances is one third padding)
    min_padding_share = 1.0 / 16

    def __init__(self, in_dim, layer_config, batch_first=None):
        super().__init__()
        self.batch_first = batch_first
        nonlin = layer_config.nonlin      # a torch.nn class name; older config.json files hold "relu" / "tanh"
        if nonlin is not None:
            nonlin = {"relu": "ReLU", "tanh": "Tanh"}.get(nonlin.lower(), nonlin)
        if layer_config.type in POOL_TYPES or layer_config.type in VAE_TYPES:
            self._create_latent_module(in_dim, layer_config, nonlin)
            return
        if layer_config.type not in ("Linear", "LayerNorm"):
            raise NotImplementedError("Only Linear, LayerNorm, PoolLast / PoolMean and VAE groups are accelerated, "
                                      "got {}.".format(layer_config))
        if nonlin is not None and nonlin not in LINEAR_NONLINS:
            raise NotImplementedError("{} group nonlin={}: not implemented (fused activations: {})."
                                      .format(layer_config.type, layer_config.nonlin, ", ".join(LINEAR_NONLINS)))
        layers = []
        for _ in range(layer_config.num_layers):
            if layer_config.type == "LayerNorm":
                # reference FFWrapper.py: `getattr(torch.nn, "LayerNorm")(**kwargs)`, the width unchanged; a
                # normalized_shape other than the group's input fails there at the first forward, here at once
                layer = LayerNormAct(act=nonlin, **layer_config.kwargs)
                if tuple(layer.normalized_shape) != (in_dim,):
                    raise ValueError("LayerNorm group normalized_shape={} does not match the group's input of {} "
                                     "features.".format(layer.normalized_shape[0], in_dim))
                layers.append(layer)
            else:
                layers.append(LinearAct(in_dim, layer_config.out_dim, act=nonlin,
                                        **layer_config.kwargs))
                in_dim = layer_config.out_dim
            if nonlin is not None:
                layers.append(FusedActivation(nonlin))
            if layer_config.dropout > 0.0:
                layers.append(Dropout(layer_config.dropout))
        self.module = nn.Sequential(*layers)
        self.out_dim = in_dim
        self.number_layers(0)

    def number_layers(self, first):
        """Gives every dropout of the group the index of the layer in front of it as its salt, counting the group's
        layers from `first` (RNNDyn passes the number of layers in the groups before); returns the next index."""
        idx = first - 1
        for m in self.module:
            if isinstance(m, Dropout):
                m.salt = max(idx, 0)
            elif not isinstance(m, FusedActivation):
                idx += 1
        return idx + 1

    def _create_latent_module(self, in_dim, layer_config, nonlin):
        """PoolLast / PoolMean and VAE / VanillaVAE groups.  What fails in the reference at the first forward, with
        an error about tuples or tensors that cannot be unpacked, is refused here by name."""
        if layer_config.type in POOL_TYPES:
            if nonlin is not None:
                raise ValueError("{} group ({}): a pooling group takes no nonlin.".format(layer_config.type,
                                                                                        layer_config))
            if layer_config.num_layers != 1:
                raise ValueError("{} group ({}): a second pooling layer would receive a tensor without its "
                                 "lengths; num_layers must be 1.".format(layer_config.type, layer_config))
            layers = [POOL_TYPES[layer_config.type](**layer_config.kwargs)]
            if layers[0].batch_first != self.batch_first and self.batch_first is not None:
                raise ValueError("{} group batch_first={} in a model with batch_first={}."
                                 .format(layer_config.type, layers[0].batch_first, self.batch_first))
            if layer_config.dropout > 0.0:
                layers.append(Dropout(layer_config.dropout))
            self.out_dim = in_dim
        else:
            if layer_config.num_layers != 1 or nonlin is not None or layer_config.dropout > 0.0:
                raise ValueError("{} group ({}): the layer returns (z, mu, log_var), a tuple no further module "
                                 "takes; num_layers must be 1, without nonlin and without dropout."
                                 .format(layer_config.type, layer_config))
            if layer_config.out_dim is None or layer_config.out_dim < 1:
                raise ValueError("{} group ({}): out_dim is the latent width and must be positive."
                                 .format(layer_config.type, layer_config))
            layers = [VanillaVAE(in_dim, layer_config.out_dim)]
            self.out_dim = layer_config.out_dim          # the width of z (the reference leaves in_dim here)
        self.module = nn.Sequential(*layers)
        self.number_layers(0)

    @property
    def returns_tuple(self):
        return isinstance(self.module[0], VanillaVAE)

    @property
    def takes_padded(self):
        """pool and VAE groups work on the padded tensor, never on the valid rows"""
        return isinstance(self.module[0], (SelectLastPooling, MeanPooling, VanillaVAE))

    def init_hidden(self, batch_size=1):
        pass

    def valid_rows_for(self, input_, kwargs):
        """The ValidRows bookkeeping when this group may run on the valid rows of `input_` (see forward), else None."""
        lengths = kwargs.get("seq_lengths_input")
        if (lengths is None or self.batch_first is None or not padding_is_identical() or input_.dim() != 3
                or not input_.is_cuda or input_.dtype != torch.float32 or not self.runs_on_rows()):
            return None
        T = input_.shape[1 if self.batch_first else 0]
        B = input_.shape[0 if self.batch_first else 1]
        if not torch.is_tensor(lengths) or lengths.numel() != B or int(lengths.max()) > T:
            return None        # (lengths of another time extent: an input merged over time, NamedForwardWrapper "attention")
        vr = ValidRows.get(lengths, T, self.batch_first, input_.device)
        return vr if vr.n_pad >= self.min_padding_share * B * T and vr.N > 0 else None

    def runs_on_rows(self):
        """dropout draws per position: in training the padding positions would not stay identical"""
        return not self.takes_padded and not (self.training and any(isinstance(m, nn.Dropout) for m in self.module))

    def linear_layers(self):
        """The group's LinearAct layers when it is nothing but those (fused activations and, outside training,
        dropout are identities) and all carry a bias, else None: what LinearChainFunction can take as one node."""
        layers = []
        for m in self.module:
            if isinstance(m, LinearAct):
                if m.bias is None:
                    return None
                layers.append(m)
            elif not isinstance(m, (FusedActivation, nn.Dropout)):
                return None
        return layers or None

    def forward_rows(self, rows):
        layers = self.linear_layers()
        if layers is None:
            return self.module(rows)
        return run_linear_chain(rows, layers)

    def chain_dropouts(self):
        """[(p, salt)] per LinearAct of a group that is nothing but Linear (+ activation) (+ dropout), (0, 0) where
        none follows; None when a dropout does not stand behind a layer or cannot be fused (p = 1)"""
        drops, last = [], None
        for m in self.module:
            if isinstance(m, LinearAct):
                drops.append((0.0, 0))
                last = len(drops) - 1
            elif isinstance(m, nn.Dropout):
                if last is None or not isinstance(m, Dropout) or not 0.0 <= m.p < 1.0 or m.inplace:
                    return None
                drops[last], last = (float(m.p), m.salt), None
        return drops

    def forward_dropout(self, input_):
        """Training with dropout (every position of the padded tensor): one seed for the whole group.  A group of
        Linear (+ activation) + dropout layers runs as ONE chain node over the flattened positions, the masks applied
        in the products' epilogues; in any other group the dropout modules take the seed and run the elementwise
        kernel.  (A training step captured into a graph would replay this seed, and with it one mask, on every
        replay; nothing captures training steps.)"""
        seed = default_dropout_stream().next()
        layers = self.linear_layers()
        drops = self.chain_dropouts() if layers is not None else None
        if drops is not None and input_.dim() >= 2:
            rows = input_.reshape(-1, input_.shape[-1])
            out = run_linear_chain(rows, layers, drops, seed)
            return out.reshape(input_.shape[:-1] + (out.shape[-1],))
        mods = [m for m in self.module if isinstance(m, Dropout)]
        for m in mods:
            m.seed = seed
        try:
            return self.module(input_)
        finally:
            for m in mods:
                m.seed = None

    def forward(self, input_, **kwargs):
        """reference FFWrapper.py:63-73: the Sequential on every position of the padded tensor.  Inside a
        `padding_rows_identical()` context (the handler's training / validation loops over stock batches) the
        layers see the valid rows and one representative padding row instead; the padding positions of the
        output receive that row's result, which is what every one of them would have computed.  (RNNDyn.forward
        keeps consecutive Linear groups on the rows without going back to the padded tensor in between.)"""
        first = self.module[0]
        if hasattr(first, "select_inputs"):          # reference CustomWrapper.py:19-23 and FFWrapper.py:150-156
            output = self.module(first.select_inputs(input_, **kwargs))
            for key in ("seq_lengths_input", "max_length_inputs"):
                kwargs[key] = first.get_output_length(kwargs.get(key))
            return output, kwargs
        vr = self.valid_rows_for(input_, kwargs)
        if vr is not None:
            return vr.unpack(self.forward_rows(vr.pack(input_))), kwargs
        if (self.training and input_.is_cuda and input_.dtype == torch.float32
                and any(isinstance(m, Dropout) for m in self.module)):
            return self.forward_dropout(input_), kwargs
        return self.module(input_), kwargs


class RNNWrapper(nn.Module):
    def __init__(self, in_dim, layer_config, batch_first=True, enforce_sorted=True):
        super().__init__()
        if layer_config.nonlin is not None and layer_config.type != 'RNN':
            raise NotImplementedError("Non-linearity is not supported for {}."
                                      .format(layer_config.type))
        if layer_config.type not in ('LSTM', 'GRU', 'RNN'):
            raise NotImplementedError("Unknown recurrent layer type {}.".format(layer_config.type))
        self.batch_first = batch_first
        self.bidirectional = layer_config.kwargs.get("bidirectional", False)
        self.hidden = None
        self.pack = True
        self.unpack = True
        cell = {'LSTM': LSTM, 'GRU': GRU, 'RNN': RNN}[layer_config.type]
        extra = {'nonlinearity': (layer_config.nonlin or 'tanh').lower()} \
            if layer_config.type == 'RNN' else {}
        self.module = cell(input_size=in_dim, hidden_size=layer_config.out_dim,
                           num_layers=layer_config.num_layers, dropout=layer_config.dropout,
                           batch_first=batch_first, bidirectional=self.bidirectional, **extra)
        ndir = 2 if self.bidirectional else 1
        init = layer_config.kwargs.get('hidden_init_value', 0.0)
        h0 = torch.full((layer_config.num_layers * ndir, 1, layer_config.out_dim), float(init))
        c0 = h0.clone()
        if layer_config.kwargs.get('train_hidden_init', False):     # reference RNNWrapper.py:66-71
            self.register_parameter('h_0', nn.Parameter(h0))
            self.register_parameter('c_0', nn.Parameter(c0))
        else:
            self.register_buffer('h_0', h0)
            self.register_buffer('c_0', c0)
        self.out_dim = layer_config.out_dim * ndir

    def init_hidden(self, batch_size=1):
        size = list(self.h_0.size())
        size[1] = batch_size
        # (copies of ONE state per layer and direction, and marked so: the recurrence kernels take a shared initial
        # state only, and nn/modules.py would otherwise compare the rows on the device and wait for the answer --
        # two host synchronisations at the start of every step)
        h_0 = self.h_0.expand(size).contiguous()
        h_0._itts_rows_shared = True
        if isinstance(self.module, LSTM):
            c_0 = self.c_0.expand(size).contiguous()
            c_0._itts_rows_shared = True
            self.hidden = (h_0, c_0)
        else:
            self.hidden = h_0

    def forward(self, input_, seq_lengths_input, max_length_inputs, hidden=None, **kwargs):
        # the kernels take the padded tensor + lengths directly (no PackedSequence round trip)
        output, self.hidden = self.module(input_, self.hidden if hidden is None else hidden,
                                          seq_lengths_input)
        time_dim = 1 if self.batch_first else 0
        total = int(max_length_inputs)
        if output.shape[time_dim] < total:      # pad_packed_sequence(total_length=...)
            pad_shape = list(output.shape)
            pad_shape[time_dim] = total - output.shape[time_dim]
            output = torch.cat((output, output.new_zeros(pad_shape)), dim=time_dim)
        kwargs["hidden"] = self.hidden
        kwargs["seq_lengths_input"] = seq_lengths_input
        kwargs["max_length_inputs"] = max_length_inputs
        return output, kwargs


class CNNWrapper(nn.Module):
    """A Conv1d layer group (reference CNNWrapper.py + TransposingWrapper.py): `num_layers` Conv1d layers, each
    followed by the group's non-linearity, on the padded batch in the model's own layout -- the kernels take
    channels-last rows, so nothing is transposed and the output comes back batch_first or time-major like the
    input.  As in the reference: padding (kernel_size - 1) // 2 is filled in (and written back into
    layer_config.kwargs) when neither padding nor a stride / dilation other than 1 is given, every weight is
    re-initialised with xavier_uniform_(gain=calculate_gain('conv1d')), the non-linearity keeps its slot in the
    nn.Sequential (state-dict keys `module.0.weight`, `module.2.weight`, ...), no dropout is appended, and
    seq_lengths_input / max_length_inputs leave with the output's lengths.  Not an FFWrapper: a convolution
    needs every position of the padded tensor, its padding included, never the valid-rows path."""

    def __init__(self, in_dim, layer_config, batch_first=True):
        super().__init__()
        if layer_config.type != "Conv1d":
            raise NotImplementedError("Layer type {} is outside the accelerated path: only Conv1d groups "
                                      "are implemented.".format(layer_config.type))
        nonlin = layer_config.nonlin
        if nonlin is not None:
            nonlin = {"relu": "ReLU", "tanh": "Tanh"}.get(nonlin.lower(), nonlin)
        if nonlin not in (None, "Tanh", "ReLU"):
            raise NotImplementedError("Conv1d group nonlin={}: only Tanh and ReLU are implemented."
                                      .format(layer_config.nonlin))
        self.batch_first = batch_first
        kwargs = layer_config.kwargs
        layers = []
        for _ in range(layer_config.num_layers):
            if 'padding' not in kwargs and kwargs.get('stride', 1) == 1 and kwargs.get('dilation', 1) == 1:
                kernel = kwargs.get('kernel_size')
                if isinstance(kernel, (tuple, list)):
                    kernel = kernel[0]
                kwargs['padding'] = int((kernel - 1) / 2)       # reference CNNWrapper.py:25-35
            layer = Conv1dAct(in_dim, layer_config.out_dim, act=nonlin, batch_first=batch_first, **kwargs)
            layers.append(layer)
            in_dim = layer_config.out_dim
            nn.init.xavier_uniform_(layer.weight, gain=nn.init.calculate_gain(layer_config.type.lower()))
            if nonlin is not None:
                layers.append(FusedActivation(nonlin))
        self.module = nn.Sequential(*layers)
        self.out_dim = in_dim

    def init_hidden(self, batch_size=1):
        pass

    def get_output_length(self, seq_lengths_input):
        """reference CNNWrapper.py:get_output_length (stride 1)"""
        for layer in self.module:
            if isinstance(layer, Conv1dAct):
                seq_lengths_input = layer.output_length(seq_lengths_input)
        return seq_lengths_input

    def forward(self, input_, **kwargs):
        output = self.module(input_)
        for key in ("seq_lengths_input", "max_length_inputs"):
            if kwargs.get(key) is not None:
                kwargs[key] = self.get_output_length(kwargs[key])
        return output, kwargs


class TransformerWrapper(nn.Module):
    """A self-attention layer group: `LayerConfig("TransformerEncoderLayer", num_layers=n, d_model=.., nhead=..,
    dim_feedforward=.., batch_first=..)`, which the reference's FFWrapper builds as `num_layers` times
    `torch.nn.TransformerEncoderLayer(**kwargs)` in an nn.Sequential named `module` (FFWrapper.py:62-73): the same
    state-dict keys, here on nn.modules.TransformerEncoderLayer.  A `LayerConfig(dropout=p)` puts a Dropout(p) behind
    each block, as FFWrapper does.  The group takes the padded tensor and the lengths, never the valid rows.

    Two keyword arguments are this package's own (the reference would hand them to torch and fail):
    mask_padding (default False): False reproduces the reference, which passes no mask, so padded positions are keys
        and an utterance's output depends on how far its batch is padded; True restricts the keys of every utterance
        to its own length (torch's src_key_padding_mask) and is the recommended setting.
    layer_dropout (default 0.1): the dropout inside the block, in [0, 1).  LayerConfig's own `dropout` never reaches
        torch's constructor in the reference, so its blocks always train with torch's default of 0.1; the default
        here is the same, and 0 turns it off.

    d_model must be the group's input width and a `batch_first` among the kwargs must be the model's (the reference
    silently attends across the batch axis otherwise); without one the model's layout is used.  A `nonlin` is
    refused: the block has its own activation."""

    OWN_KWARGS = ("mask_padding", "layer_dropout")

    def __init__(self, in_dim, layer_config, batch_first=True):
        super().__init__()
        if layer_config.type != "TransformerEncoderLayer":
            raise NotImplementedError("Layer type {} is not a self-attention group.".format(layer_config.type))
        if layer_config.nonlin is not None:
            raise NotImplementedError("TransformerEncoderLayer group nonlin={}: not implemented, the block applies "
                                      "its own activation.".format(layer_config.nonlin))
        kwargs = dict(layer_config.kwargs)
        self.mask_padding = bool(kwargs.pop("mask_padding", False))
        layer_dropout = float(kwargs.pop("layer_dropout", 0.1))
        if not 0.0 <= layer_dropout < 1.0:
            raise ValueError("TransformerEncoderLayer group layer_dropout={} is outside [0, 1).".format(layer_dropout))
        if "d_model" not in kwargs or "nhead" not in kwargs:
            raise ValueError("TransformerEncoderLayer group ({}): d_model and nhead are required.".format(layer_config))
        if kwargs["d_model"] != in_dim:
            raise ValueError("TransformerEncoderLayer group d_model={} does not match the group's input of {} "
                             "features.".format(kwargs["d_model"], in_dim))
        if bool(kwargs.setdefault("batch_first", bool(batch_first))) != bool(batch_first):
            raise ValueError("TransformerEncoderLayer group batch_first={} in a model with batch_first={}: the block "
                             "would attend across the batch axis.".format(kwargs["batch_first"], batch_first))
        self.batch_first = batch_first
        layers = []
        for _ in range(layer_config.num_layers):
            layers.append(TransformerEncoderLayer(dropout=layer_dropout, **kwargs))
            if layer_config.dropout > 0.0:
                layers.append(Dropout(layer_config.dropout))
        self.module = nn.Sequential(*layers)
        self.out_dim = in_dim
        self.number_layers(0)

    def number_layers(self, first):
        """The blocks take the indices first, first + 1, ... as their salts, a dropout behind a block that block's
        index; returns the next index."""
        idx = first - 1
        for m in self.module:
            if isinstance(m, Dropout):
                m.salt = max(idx, 0)
            else:
                idx += 1
                m.salt = idx
        return idx + 1

    def init_hidden(self, batch_size=1):
        pass

    def forward(self, input_, **kwargs):
        lengths = kwargs.get("seq_lengths_input") if self.mask_padding else None
        if lengths is not None:
            lengths = self.module[0].key_lengths(input_, lengths)       # one upload for all blocks
        for m in self.module:
            if isinstance(m, TransformerEncoderLayer):
                input_ = m(input_, lengths=lengths, mask_padding=lengths is not None)
            else:
                input_ = m(input_)
        return input_, kwargs


class RNNDyn(nn.ModuleList):

    def __init__(self, config):
        super().__init__()
        self.config = copy.deepcopy(config)
        self.emb_groups = nn.ModuleDict()      # slot 0 of the ModuleList, like the reference
        for emb_config in config.emb_configs or ():
            emb = nn.Embedding(emb_config.num_embedding, emb_config.embedding_dim)
            emb.affected_layer_group_indices = emb_config.affected_layer_group_indices
            emb.name = emb_config.name
            self.emb_groups[emb_config.name] = emb
        self.layer_groups = []
        n_layers = 0
        in_dim = config.in_dim
        for group_idx, layer_config in enumerate(config.layer_configs):
            in_dim += self._get_embeddings_dim(group_idx)
            if layer_config.needs_packing:
                layer = RNNWrapper(in_dim, layer_config, config.batch_first, enforce_sorted=False)
            elif layer_config.needs_transposing:
                if layer_config.type != "Conv1d":
                    raise NotImplementedError("{} groups are outside the accelerated path (SURVEY.md "
                                              "section 2).".format(layer_config.type))
                layer = CNNWrapper(in_dim, layer_config, config.batch_first)
            elif layer_config.type == "TransformerEncoderLayer":
                layer = TransformerWrapper(in_dim, layer_config, config.batch_first)
            else:
                layer = FFWrapper(in_dim, layer_config, config.batch_first)
            in_dim = layer.out_dim
            if getattr(layer, "returns_tuple", False) and group_idx != len(config.layer_configs) - 1:
                raise ValueError("{} group ({}) is group {} of {}: it returns (z, mu, log_var) and must be the last "
                                 "group.".format(layer_config.type, layer_config, group_idx + 1,
                                                 len(config.layer_configs)))
            self.append(layer)
            self.layer_groups.append(layer)
            # the salt of a dropout is the index in the model of the layer in front of it
            if isinstance(layer, (FFWrapper, TransformerWrapper)):
                n_layers = layer.number_layers(n_layers)
            else:
                n_layers += layer_config.num_layers

    def forward(self, input_, *emb_inputs, **kwargs):
        """reference :88-121.  Embedding indices come as extra arguments (one [T, B, 1] tensor
        per embedding group) or -- deprecated in the reference, but what its wrappers do -- as the
        last columns of the input."""
        embeddings = {}
        if len(self.emb_groups) > 0:
            n = len(self.emb_groups)
            if len(emb_inputs) > 0:
                if len(emb_inputs) != n:
                    raise ValueError("Given number of embedding inputs ({}) does not match number "
                                     "of embedding groups ({}) in model.".format(len(emb_inputs), n))
            else:
                emb_inputs = [input_[:, :, input_.shape[2] - n + i:input_.shape[2] - n + i + 1]
                              for i in range(n)]
                input_ = input_[:, :, :-n]
            for idx, emb in enumerate(self.emb_groups.values()):
                embeddings[emb.name] = emb(emb_inputs[idx][:, :, 0].long())
        last_hidden = None
        rows = None          # (ValidRows, [N (+ 1), F]) while a run of Linear groups works on the valid rows
        chain = []           # .. and the LinearAct layers of that run not applied yet (one autograd node for them all)

        def flush():
            nonlocal rows, chain
            if chain:
                rows, chain = (rows[0], run_linear_chain(rows[1], chain)), []

        # After a Conv1d group the padding positions no longer hold one common row (those just past each length mix
        # in valid frames), and after a self-attention group neither (every position attends its own utterance's
        # keys), so no later group may stand one representative row in for them.
        padding_mixed = False
        for group_idx, module in enumerate(self.layer_groups):
            affected = [emb for emb in self.emb_groups.values() if self._affects(emb, group_idx)]
            if isinstance(module, FFWrapper) and not affected and not padding_mixed:
                if rows is None:
                    vr = module.valid_rows_for(input_, kwargs)
                    if vr is not None:
                        rows = (vr, vr.pack(input_))
                if rows is not None and module.runs_on_rows():
                    layers = module.linear_layers()
                    if layers is not None:
                        chain += layers
                    else:
                        flush()
                        rows = (rows[0], module.module(rows[1]))
                    continue
            if rows is not None:
                flush()
                input_, rows = rows[0].unpack(rows[1]), None
            for emb in affected:
                input_ = torch.cat((input_, embeddings[emb.name]), dim=2)
            padding_mixed = padding_mixed or isinstance(module, (CNNWrapper, TransformerWrapper))
            if padding_mixed and padding_is_identical():
                with padding_rows_identical(False):
                    input_, kwargs = module(input_, **kwargs)
            else:
                input_, kwargs = module(input_, **kwargs)
            # hidden states are not passed from one RNN group to the next (reference :118-121)
            last_hidden = kwargs.pop("hidden", last_hidden)
        if rows is not None:
            flush()
            input_ = rows[0].unpack(rows[1])
        kwargs["hidden"] = last_hidden
        return input_, kwargs

    @staticmethod
    def _affects(emb, group_idx):
        idx = emb.affected_layer_group_indices
        return idx is not None and (-1 in idx or group_idx in idx)

    def _get_embeddings_dim(self, group_idx):
        return sum(emb.embedding_dim for emb in self.emb_groups.values()
                   if self._affects(emb, group_idx))

    def __getitem__(self, item):
        """Zero-based indexing of the layer groups (reference :364-366)."""
        return self.layer_groups[item]

    def get_embeddings(self):
        return self.emb_groups

    def get_group_out_dim(self, group_idx):
        return self.layer_groups[group_idx].out_dim

    def init_hidden(self, batch_size=1):
        for module in self.layer_groups:
            module.init_hidden(batch_size)

    def set_gpu_flag(self, use_gpu):
        self.use_gpu = use_gpu
