"""enc_dec_dyn.Config with the reference's fields (models/enc_dec_dyn/Config.py), restricted to what runs here:
named modules executed in the order of their `process_group`, each an rnn_dyn model (ModuleConfig), a pass-through
(ModuleConfig with config=None), a NamedForwardWrapper (WrapperConfig) or a fixed-attention decoder with its pre-net
and projections (DecoderConfig, ProjectionConfig; DecoderModule.py); all batch_first, as in the reference.  Combiners
and splitters are separate pieces of work and refuse by name."""
from typing import List

from ..NamedForwardWrapper import NamedForwardWrapper


def external_input_names(process_groups):
    """The names some module reads and no earlier module writes, in the order they are first read: what the data
    readers have to provide."""
    written, names = set(), []
    for group in process_groups:
        for module in group:
            # (a decoder also reads its attention matrix: DecoderConfig.extra_input_names)
            for name in list(module.input_names or ()) + list(getattr(module, "extra_input_names", ())):
                if name not in written and name not in names:
                    names.append(name)
            written.update(module.output_names or ())
    return names


class Config:

    class ModuleConfig:
        def __init__(self, input_names: List[str], config=None, input_merge_type: str = "cat", name: str = None,
                     process_group: int = 0, output_names: List[str] = None, **kwargs):
            self.input_names = input_names
            self.batch_first = True
            self.input_merge_type = input_merge_type
            self.name = name
            self.output_names = output_names
            self.kwargs = kwargs
            self.config = config
            self.process_group = process_group

        def create_model(self):
            from .EncDecDyn import SubModule
            return SubModule(self)

    class WrapperConfig(NamedForwardWrapper.Config):
        """a NamedForwardWrapper as a module of the chain: its Config, batch_first, plus the process group"""

        def __init__(self, wrapped_model_config, input_names: List[str], input_merge_type: str = "cat",
                     name: str = None, output_names: List[str] = None, process_group: int = 0):
            NamedForwardWrapper.Config.__init__(self, wrapped_model_config, input_names, True,
                                                input_merge_type=input_merge_type, name=name,
                                                output_names=output_names)
            self.process_group = process_group

    class ProjectionConfig(ModuleConfig):
        """a projection of a decoder's output (DecoderConfig.projection_configs): it has no input names of its own;
        `is_autoregressive_input`: its last frame is fed back to the decoder, and `out_dim` is that frame's width"""

        def __init__(self, out_dim: int = None, is_autoregressive_input: bool = False, **kwargs):
            if "input_names" in kwargs:
                raise NotImplementedError("enc_dec_dyn.Config.ProjectionConfig(input_names={!r}): a projection with "
                                          "inputs of its own is not implemented, it reads its decoder's output (the "
                                          "reference takes no input_names here either)."
                                          .format(kwargs["input_names"]))
            if out_dim is None:
                raise TypeError("enc_dec_dyn.Config.ProjectionConfig needs out_dim, the width of one projected frame.")
            super().__init__(input_names=None, **kwargs)
            Config._default_output_names(self)
            self.is_autoregressive_input = is_autoregressive_input
            self.out_dim = out_dim

        def create_model(self):
            from .DecoderModule import ProjectionModule
            return ProjectionModule(self)

    class DecoderConfig(ModuleConfig):
        """a frame-rate decoder behind an attention over its phoneme-rate inputs (DecoderModule).  As in the
        reference: `attention_config` names the mechanism (enc_dec_dyn.FIXED_ATTENTION, the only one there is: any other
        value, the default None included, is refused here and not in the first forward) and the legacy `attention_args`
        dict holds its arguments ({enc_dec_dyn.ATTENTION_GROUND_TRUTH: <name of the attention matrix>});
        `teacher_forcing_input_names` makes it autoregressive; a `decoder_output_name` attribute set on the config
        names an extra output for the decoder's own output.  A plain string for input_names / output_names means a
        list of that one name (the reference's ModelConfig._str_to_list)."""

        def __init__(self, attention_config=None, attention_args: dict = {},    # (legacy, as in the reference)
                     teacher_forcing_input_names: List[str] = None, n_frames_per_step: int = 1,
                     p_teacher_forcing: float = 1.0, pre_net_config=None, projection_configs=None, **kwargs):
            from . import FIXED_ATTENTION
            if attention_config != FIXED_ATTENTION:
                # (the reference's DecoderModule has no attention then and fails in its first forward)
                raise NotImplementedError("enc_dec_dyn.Config.DecoderConfig(attention_config={!r}): only {!r} is "
                                          "implemented (learned attention is a separate piece of work)."
                                          .format(attention_config, FIXED_ATTENTION))
            super().__init__(**kwargs)
            self.input_names = Config._str_to_list(self.input_names)
            Config._default_output_names(self)
            self.attention_config = attention_config
            self.attention_args = attention_args
            assert teacher_forcing_input_names is None or len(teacher_forcing_input_names) > 0, \
                "Empty list not allowed for teacher_forcing_input_names, use None instead."
            self.teacher_forcing_input_names = teacher_forcing_input_names
            self.n_frames_per_step = n_frames_per_step
            self.p_teacher_forcing = p_teacher_forcing
            self.pre_net_config = pre_net_config
            self.projection_configs = projection_configs

        @property
        def extra_input_names(self):
            """what the module reads besides input_names at synthesis time: the attention matrix"""
            from . import ATTENTION_GROUND_TRUTH
            name = (self.attention_args or {}).get(ATTENTION_GROUND_TRUTH)
            return [name] if name is not None else []

        def create_model(self):
            from .DecoderModule import DecoderModule
            return DecoderModule(self)

    @staticmethod
    def _str_to_list(str_or_list):
        if str_or_list is None or isinstance(str_or_list, (tuple, list)):
            return str_or_list
        return [str_or_list]

    @staticmethod
    def _default_output_names(config):
        """the reference's ModelConfig: output_names defaults to [name], a string is a list of one"""
        assert config.output_names is not None or config.name is not None, \
            "Default output_names is [name], but both are None for input {}.".format(config.input_names)
        config.output_names = Config._str_to_list(config.output_names) if config.output_names is not None \
            else [config.name]

    class _NotBuilt:
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("enc_dec_dyn.Config.{} is not implemented: only ModuleConfig, WrapperConfig, "
                                      "DecoderConfig and ProjectionConfig modules run here."
                                      .format(type(self).__name__))

    class CombinerConfig(_NotBuilt):
        pass

    class SplitterConfig(_NotBuilt):
        pass

    def __init__(self, modules: List["Config.ModuleConfig"]):
        # process_groups[g]: the modules of process group g in the order given (groups nobody names stay empty)
        self.process_groups = [[m for m in modules if m.process_group == g]
                               for g in range(max(m.process_group for m in modules) + 1)]

    @property
    def input_names(self):
        return external_input_names(self.process_groups)

    def create_model(self):
        from .EncDecDyn import EncDecDyn        # (import here: the two files name each other)
        return EncDecDyn(self)

    def __getattr__(self, item):
        """`config.<module name>` is that module's config, as in the reference; only reached for names that are not
        attributes (never for `process_groups` itself or the dunder look-ups of copy and pickle)."""
        if item != "process_groups" and not item.startswith("__"):
            named = {m.name: m for group in self.__dict__.get("process_groups", ()) for m in group}
            if item in named:
                return named[item]
        raise AttributeError("{} has no attribute or module named {!r}".format(type(self).__name__, item))
