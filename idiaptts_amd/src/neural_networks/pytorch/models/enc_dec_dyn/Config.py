"""enc_dec_dyn.Config with the reference's fields (models/enc_dec_dyn/Config.py), restricted to what runs here:
named modules executed in the order of their `process_group`, each an rnn_dyn model (ModuleConfig), a pass-through
(ModuleConfig with config=None) or a NamedForwardWrapper (WrapperConfig); all batch_first, as in the reference.
Attention decoders, projections, combiners and splitters are separate pieces of work and refuse by name."""
from typing import List

from ..NamedForwardWrapper import NamedForwardWrapper


def external_input_names(process_groups):
    """The names some module reads and no earlier module writes, in the order they are first read: what the data
    readers have to provide."""
    written, names = set(), []
    for group in process_groups:
        for module in group:
            for name in module.input_names or ():
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

    class _NotBuilt:
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("enc_dec_dyn.Config.{} is not implemented: only ModuleConfig and WrapperConfig "
                                      "modules run here.".format(type(self).__name__))

    class ProjectionConfig(_NotBuilt):
        pass

    class DecoderConfig(_NotBuilt):
        pass

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
