"""Reference captures for self-attention layer groups (reference rnn_dyn/FFWrapper.py:62-73 builds
`torch.nn.TransformerEncoderLayer(**kwargs)` by name), run on the CPU against the reference package with the stub
harness of make_golden.py.  Writes tests/golden/attention_fixture.npz, data only:

  <case>/sd/<key>            the state dict of the reference's RNNDyn (built under torch.manual_seed; float32)
  <case>/x, <case>/w         the zero-padded input and the weight tensor of the loss sum(y * w) over every position
  <case>/y, <case>/y32       the output at every padded position in float64 (the model cast with .double()) and the
                             reference's own float32 result beside it
  <case>/grad/<param>, <case>/grad32/<param>   every parameter gradient, likewise
  <case>/seq_lengths_input, <case>/max_length_inputs   as the reference's forward returns them

for the cases of attention_spec.MODEL_CASES: Linear(16, Tanh) -> TransformerEncoderLayer x 2 -> Linear(5) on 6 inputs,
lengths 7, 4 and 1, batch_first and time-major, and norm_first=True.  The model is in eval() (dropout off; train()
with the block's dropout at 0 gives the same numbers) with autograd on, so torch takes its plain path.  The reference
passes no mask: padded positions are keys.

Usage: python tests/golden/make_golden_attention.py (needs the reference checkout)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from attention_spec import MODEL_CASES, MODEL_LENS, model_config, model_inputs  # noqa: E402


def capture(out):
    import torch
    from idiaptts.src.neural_networks.pytorch.models.rnn_dyn.Config import Config
    from idiaptts.src.neural_networks.pytorch.models.rnn_dyn.RNNDyn import RNNDyn
    lens = torch.tensor(MODEL_LENS)
    T, B = max(MODEL_LENS), len(MODEL_LENS)
    for name, bf, norm_first, seed in MODEL_CASES:
        torch.manual_seed(seed)
        model = RNNDyn(model_config(Config, bf, norm_first)).eval()
        x, w = model_inputs(seed, bf)
        p = name + "/"
        for k, v in model.state_dict().items():
            out[p + "sd/" + k] = v.detach().numpy().copy()
        out[p + "x"], out[p + "w"] = x.numpy().copy(), w.numpy().copy()
        for suffix, cast in (("32", lambda t: t), ("", lambda t: t.double())):
            net = cast(model)
            net.zero_grad()
            net.init_hidden(B)
            y, kwargs = net(cast(x), seq_lengths_input=lens, max_length_inputs=torch.tensor(T))
            (y * cast(w)).sum().backward()
            out[p + "y" + suffix] = y.detach().numpy().copy()
            for k, prm in net.named_parameters():
                out[p + "grad" + suffix + "/" + k] = prm.grad.numpy().copy()
            out[p + "seq_lengths_input"] = np.asarray(kwargs["seq_lengths_input"])
            out[p + "max_length_inputs"] = np.asarray(kwargs["max_length_inputs"])
        err = np.abs(out[p + "y32"] - out[p + "y"]).max()
        print(name, tuple(out[p + "y"].shape), "float32 against float64: {:.3g}".format(err),
              [k for k in model.state_dict()][:3])


def _main():
    mg.install_stub_harness()
    out = {}
    capture(out)
    path = os.path.join(HERE, "attention_fixture.npz")
    np.savez_compressed(path, **out)
    print("attention_fixture.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    _main()
