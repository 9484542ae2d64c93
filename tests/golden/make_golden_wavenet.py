"""Reference capture for the WaveNet wrapper's Config: imports the reference's models/WaveNetWrapper.py by its file
with the `wavenet_vocoder` package (absent everywhere) stubbed in sys.modules, builds `WaveNetWrapper.Config()` and
writes its attributes -- settings only -- to tests/golden/wavenet_config_defaults.json, together with IDENTIFIER and
the two INPUT_TYPE_* names.  The one function of the package the Config's defaults call, util.is_scalar_input, is
stubbed with its published meaning (the input type "raw" is scalar, "mulaw-quantize" is not).
Usage: python tests/golden/make_golden_wavenet.py (needs the reference checkout; no GPU)."""
import importlib.util
import json
import os
import sys
import types
from unittest.mock import MagicMock

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


def reference_wrapper():
    pkg = types.ModuleType("wavenet_vocoder")
    pkg.WaveNet = MagicMock(name="wavenet_vocoder.WaveNet")
    modules = types.ModuleType("wavenet_vocoder.modules")
    modules.Conv1d = type("Conv1d", (), {})
    modules.ConvTranspose2d = type("ConvTranspose2d", (), {})
    util = types.ModuleType("wavenet_vocoder.util")
    util.is_scalar_input = lambda input_type: input_type == "raw"
    sys.modules.update({"wavenet_vocoder": pkg, "wavenet_vocoder.modules": modules, "wavenet_vocoder.util": util})
    path = os.path.join(mg.REF, "idiaptts", "src", "neural_networks", "pytorch", "models", "WaveNetWrapper.py")
    spec = importlib.util.spec_from_file_location("ref_wavenet_wrapper", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.WaveNetWrapper


def main():
    ref = reference_wrapper()
    record = {"IDENTIFIER": ref.IDENTIFIER, "INPUT_TYPE_MULAW": ref.Config.INPUT_TYPE_MULAW,
              "INPUT_TYPE_RAW": ref.Config.INPUT_TYPE_RAW, "defaults": vars(ref.Config())}
    path = os.path.join(HERE, "wavenet_config_defaults.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(record["defaults"]), "fields")


if __name__ == "__main__":
    main()
