"""The module cases of tests/golden/conv1d_fixture.npz (written by tests/golden/make_golden_conv.py against the
reference, read by tests/test_gpu_conv_model.py and tests/test_conv_config.py): model specs, seeds, lengths, and the
seeded inputs and targets, which the fixture does not store."""

import types

CONV_MODEL = "RNNDYN-1_RELU_32-1_Conv1d_16_3-1_FC_67"


def _newstyle_layers(Config):
    return [Config.LayerConfig("Conv1d", out_dim=24, kernel_size=5, nonlin="ReLU"),
            Config.LayerConfig("Conv1d", out_dim=20, kernel_size=3, dilation=2, padding=2, nonlin="Tanh"),
            Config.LayerConfig("Linear", out_dim=67)]


def _pad0_layers(Config):
    return [Config.LayerConfig("Linear", out_dim=12, nonlin="Tanh"),
            Config.LayerConfig("Conv1d", out_dim=10, kernel_size=5, padding=0, nonlin="ReLU"),
            Config.LayerConfig("Linear", out_dim=7)]


CASES = [   # name, legacy string or layer list, in_dim, batch_first, seed, lengths, out_dim
    ("legacy_bf", CONV_MODEL, 409, True, 11, [13, 7, 10], 67),
    ("legacy_tm", CONV_MODEL, 409, False, 11, [9, 6, 4], 67),
    ("newstyle", _newstyle_layers, 64, True, 13, [16, 11, 5, 14], 67),
    ("pad0", _pad0_layers, 11, False, 14, [12, 8, 6], 7),
]
SD_CASE = {"legacy_tm": "legacy_bf"}     # cases whose state_dict is stored under another case


def case_config(rnn_dyn, Config, case):
    """the rnn_dyn Config of a CASES entry (the reference's package or this one: same names)"""
    name, spec, in_dim, bf = case[:4]
    if isinstance(spec, str):
        return rnn_dyn.convert_legacy_to_config((in_dim,), types.SimpleNamespace(model_type=spec, batch_first=bf,
                                                                                  dropout=0.0))
    return Config(in_dim=in_dim, batch_first=bf, layer_configs=spec(Config))


def case_inputs(torch, index, in_dim, batch_first, lens, out_shape):
    """(x, tgt) of module case `index` on the CPU: a zero-padded batch and a target of shape out_shape, from a
    generator seeded with 100 + index"""
    g = torch.Generator().manual_seed(100 + index)
    T, B = max(lens), len(lens)
    x = torch.randn((B, T, in_dim) if batch_first else (T, B, in_dim), generator=g)
    for b, n in enumerate(lens):
        if batch_first:
            x[b, n:] = 0
        else:
            x[n:, b] = 0
    return x, torch.randn(tuple(out_shape), generator=g)


def masked_mse(torch, y, tgt, lens, batch_first):
    """sum over the valid frames of (y - tgt)^2 / (frames * features)"""
    T = y.shape[1 if batch_first else 0]
    mask = (torch.arange(T, device=y.device)[None, :] < lens[:, None]).to(y.dtype)          # [B, T]
    if not batch_first:
        mask = mask.t()
    return (((y - tgt) ** 2) * mask[..., None]).sum() / (lens.sum() * y.shape[2])
