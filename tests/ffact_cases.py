"""The cases of tests/golden/ffact_fixture.npz (written by tests/golden/make_golden_ffact.py against the reference,
read by tests/test_gpu_ffact.py and tests/test_ffact_config.py): Linear groups with the activations beyond Tanh /
ReLU, their seeds and lengths, and the seeded inputs and targets, which the fixture does not store."""

# every activation a Linear group fuses besides Tanh / ReLU: torch.nn class names
NEW_NONLINS = ("Sigmoid", "LogSigmoid", "Softplus", "Softsign", "LeakyReLU", "ELU", "CELU", "SELU", "Hardtanh",
               "ReLU6", "Hardsigmoid")
# names a Linear group refuses (NotImplementedError naming them)
REFUSED_NONLINS = ("GELU", "SiLU", "Mish", "Hardswish", "Tanhshrink", "PReLU", "RReLU", "Softmax", "LogSoftmax")


def _layers(Config, groups):
    return [Config.LayerConfig("Linear", out_dim=d, num_layers=n, nonlin=a) for d, n, a in groups]


CASES = [   # name, groups (out_dim, num_layers, nonlin), in_dim, batch_first, seed, lengths, input scale
    ("sig_bf", [(24, 2, "Sigmoid"), (20, 1, "LogSigmoid"), (16, 1, "Softplus"), (7, 1, None)], 13, True, 21,
     [13, 7, 10], 1.0),
    ("leaky_tm", [(24, 1, "Softsign"), (20, 2, "LeakyReLU"), (18, 1, "ELU"), (7, 1, None)], 11, False, 22,
     [9, 6, 4, 9], 1.0),
    ("selu_bf", [(20, 1, "CELU"), (24, 1, "SELU"), (16, 1, "Hardtanh"), (5, 1, None)], 9, True, 23,
     [12, 5, 8], 2.0),
    ("clamp_tm", [(24, 1, "ReLU6"), (20, 1, "Hardsigmoid"), (11, 1, "Sigmoid")], 10, False, 24,
     [7, 11, 3], 8.0),
]
# new-style model of the trainer case (409 questions -> 67 acoustic features)
TRAINER_GROUPS = [(32, 1, "ELU"), (32, 1, "Sigmoid"), (32, 1, "Softsign"), (67, 1, None)]


def case_config(Config, case):
    """the rnn_dyn Config of a CASES entry (the reference's package or this one: same names)"""
    name, groups, in_dim, bf = case[:4]
    return Config(in_dim=in_dim, batch_first=bf, layer_configs=_layers(Config, groups))


def trainer_model_config(rnn_dyn, NamedForwardWrapper, name_lists=True):
    """the model_config AcousticModelTrainer.init receives for the trainer case (the reference's own default passes
    the input and output names as plain strings: name_lists=False)"""
    cfg = rnn_dyn.Config(in_dim=409, batch_first=True, layer_configs=_layers(rnn_dyn.Config, TRAINER_GROUPS))
    names = (lambda n: [n]) if name_lists else (lambda n: n)
    return NamedForwardWrapper.Config(wrapped_model_config=cfg, input_names=names("questions"), batch_first=True,
                                      name="AcousticModel", output_names=names("pred_acoustic_features"))


def case_inputs(torch, index, in_dim, batch_first, lens, out_shape, scale=1.0):
    """(x, tgt) of module case `index` on the CPU: a zero-padded batch (randn * scale) and a target of shape
    out_shape, from a generator seeded with 200 + index"""
    g = torch.Generator().manual_seed(200 + index)
    T, B = max(lens), len(lens)
    x = torch.randn((B, T, in_dim) if batch_first else (T, B, in_dim), generator=g) * scale
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
