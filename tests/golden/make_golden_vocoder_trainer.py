"""Reference capture for WaveNetVocoderTrainer: imports the reference's model_trainers/WaveNetVocoderTrainer.py with
every package that is not installed (wavenet_vocoder, pydub, git, ...) stubbed in sys.modules -- a stub answers any
attribute with a mock; `wavenet_vocoder.util.is_scalar_input` gets its published meaning, as in
make_golden_wavenet.py -- and writes settings only to tests/golden/vocoder_trainer_defaults.json:
  * what create_hparams() adds to or changes in ModularTrainer.create_hparams() (JSON-representable values);
  * the two DataReaderConfigs of legacy_support_init: name, type, directory, features, output names, the length
    attributes and the keyword arguments, with `preprocessing_fn` recorded by its function's name and keywords.
Usage: python tests/golden/make_golden_vocoder_trainer.py (needs the reference checkout; no GPU)."""
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types
from functools import partial
from unittest.mock import MagicMock

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        value = MagicMock(name=self.__name__ + "." + name)
        setattr(self, name, value)
        return value


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """last on sys.meta_path: a package that has been found missing (`roots`), and everything below it, is a stub"""
    roots, stubbed = set(), []

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] not in self.roots:
            return None
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        self.stubbed.append(spec.name)
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def reference_trainer():
    util = _Stub("wavenet_vocoder.util")
    util.is_scalar_input = lambda input_type: input_type == "raw"
    sys.modules["wavenet_vocoder.util"] = util
    _StubFinder.roots.add("wavenet_vocoder")
    sys.meta_path.append(_StubFinder())
    sys.path.insert(0, mg.REF)
    os.environ.setdefault("IDIAPTTS_ROOT", os.path.join(mg.REF, "idiaptts"))
    while True:                              # one missing package per round: stub it, forget the half import, again
        try:
            from idiaptts.src.model_trainers.ModularTrainer import ModularTrainer
            from idiaptts.src.model_trainers.WaveNetVocoderTrainer import WaveNetVocoderTrainer
            return ModularTrainer, WaveNetVocoderTrainer
        except ModuleNotFoundError as e:
            root = e.name.split(".")[0]
            if root == "idiaptts" or root in _StubFinder.roots:
                raise
            _StubFinder.roots.add(root)
            for name in [n for n in sys.modules if n.split(".")[0] == "idiaptts"]:
                del sys.modules[name]


def _plain(value):
    if isinstance(value, partial):
        return {"partial": value.func.__name__,
                "keywords": {k: (v.__name__ if isinstance(v, type) else v) for k, v in sorted(value.keywords.items())}}
    if isinstance(value, tuple):
        return list(value)
    return value


def _representable(value):
    try:
        json.dumps(value)
    except TypeError:
        return False
    return True


def main():
    base_cls, cls = reference_trainer()
    base, hparams = base_cls.create_hparams().values(), cls.create_hparams()
    values = hparams.values()
    additions = {k: v for k, v in values.items() if _representable(v) and (k not in base or base[k] != v)}
    hparams.data_dir, hparams.num_coded_sps = "WAV_DIR", 80
    configs = cls.legacy_support_init("WORLD_DIR", ["id1"], hparams)["data_reader_configs"]
    readers = []
    for c in configs:
        record = {k: _plain(v) for k, v in vars(c).items() if k != "kwargs"}
        record["kwargs"] = {k: _plain(v) for k, v in sorted(c.kwargs.items())}
        readers.append(record)
    out = {"hparams_additions": additions, "reader_configs": readers,
           "legacy_hparams": {"data_dir": "WAV_DIR", "num_coded_sps": 80, "dir_world_features": "WORLD_DIR"}}
    path = os.path.join(HERE, "vocoder_trainer_defaults.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(additions), "hparams,", len(readers), "reader configs; stubbed:",
          sorted(_StubFinder.roots))


if __name__ == "__main__":
    main()
