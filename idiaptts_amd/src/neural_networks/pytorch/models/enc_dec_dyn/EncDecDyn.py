"""EncDecDyn: named modules run one after the other on one data dictionary (the role of the reference's
models/enc_dec_dyn/EncDecDyn.py and SubModule.py), e.g. a `Conv1d -> GRU -> PoolLast -> VAE` encoder writing
["emb_z", "emb_mu", "emb_logvar"] and a decoder reading ["phoneme_embeddings", "emb_z"] -- the single-frame embedding
is repeated over the decoder's time axis by the wrapper's merge.  Each module is a child under its own name, so
parameter keys are `<name>.model.<rnn_dyn keys>`.  The container also carries what the model handler reads from a
model: `batch_first` (always True here, as in the reference) and `input_names`, the names the data readers provide.

A `Config.DecoderConfig` module is a DecoderModule (DecoderModule.py): the frame-rate decoder behind the fixed attention,
with its pre-net and projections as children (`<name>.pre_net.*`, `<name>.<name>_<projector>.model.*`); `init_hidden`
reaches them through it.

A module that reads a name an earlier module wrote is marked (`reads_module_outputs`): the handler's
`padding_rows_identical()` context speaks for the readers' batches, not for computed tensors, so such a module works on
every position of the padded tensor (NamedForwardWrapper.forward)."""
import copy

from torch import nn

from ..NamedForwardWrapper import NamedForwardWrapper
from .Config import external_input_names


class _PassThrough(nn.Module):
    """stands in for the wrapped model of a SubModule without one"""

    def forward(self, input_, **kwargs):
        return input_, kwargs

    def init_hidden(self, batch_size=1):
        pass


class SubModule(NamedForwardWrapper):
    """A NamedForwardWrapper built from a `Config.ModuleConfig`: around its rnn_dyn model, or around nothing -- with
    `config.config is None` the merged input goes to the output names unchanged, with the first input's lengths."""

    def _create_wrapped_model(self, config):
        model = config.config.create_model() if config.config is not None else _PassThrough()
        if getattr(getattr(model, "config", None), "batch_first", True) is not True:
            raise ValueError("Module {}: enc_dec_dyn modules are batch_first, its rnn_dyn config is not."
                             .format(config.name))
        return model


class EncDecDyn(nn.Module):

    batch_first = True

    def __init__(self, config):
        super().__init__()
        self.config = copy.deepcopy(config)
        self.chain = []              # the modules in the order they run: by process group, then as listed
        written = set()
        for module_config in (m for group in config.process_groups for m in group):
            module = module_config.create_model()
            name = str(module.name)
            if name in self._modules:
                raise ValueError("Two modules of the chain are named {}.".format(name))
            self.add_module(name, module)
            module.reads_module_outputs = any(n in written for n in module.input_names or ())
            written.update(module.output_names or ())
            self.chain.append(module)
        self.input_names = external_input_names([self.chain])

    def init_hidden(self, batch_size=1):
        for module in self.chain:
            module.init_hidden(batch_size)

    def forward(self, data, lengths, max_lengths):
        for module in self.chain:
            module(data, lengths, max_lengths)
        return data

    def inference(self, data, lengths, max_lengths):
        for module in self.chain:
            module.inference(data, lengths, max_lengths)
        return data
