"""The cases of tests/golden/lnorm_fixture.npz (written by tests/golden/make_golden_lnorm.py against the reference,
read by tests/test_gpu_lnorm_model.py and tests/test_lnorm_config.py): models with LayerNorm layer groups between
Linear, BiLSTM and Conv1d groups, their seeds and lengths, and the seeded inputs and targets, which the fixture does
not store."""


def _layers(Config, groups):
    return [Config.LayerConfig(t, out_dim=d, num_layers=n, nonlin=a, **kw) for t, d, n, a, kw in groups]


def LN(width, num_layers=1, nonlin=None, **kwargs):
    """a LayerNorm group: no out_dim, the width travels as torch.nn.LayerNorm's normalized_shape"""
    return ("LayerNorm", None, num_layers, nonlin, dict(normalized_shape=width, **kwargs))


def LIN(width, nonlin=None):
    return ("Linear", width, 1, nonlin, {})


CASES = [   # name, groups (type, out_dim, num_layers, nonlin, kwargs), in_dim, batch_first, seed, lengths, input scale,
            # LayerNorm groups that run on the valid rows inside padding_rows_identical()
    # after Linear groups, batch_first; an activation of the extended family; bias=False
    ("lin_bf", [LIN(24, "Tanh"), LN(24), LIN(18, "ELU"), LN(18, nonlin="ELU", bias=False), LIN(7)], 13, True, 31,
     [13, 7, 10], 1.0, 2),
    # after a BiLSTM group, time-major; eps 1e-3; the padding rows are the recurrence's zeros (variance 0)
    ("lstm_tm", [("LSTM", 12, 1, None, dict(bidirectional=True)), LN(24, eps=1e-3), LIN(5)], 11, False, 32,
     [9, 6, 4, 9], 1.0, 1),
    # after a Conv1d group, batch_first; normalized_shape given as a list (no valid-rows path behind a convolution)
    ("conv_bf", [("Conv1d", 16, 1, "ReLU", dict(kernel_size=3)), LN([16]), LIN(6)], 9, True, 33, [12, 5, 8], 1.0, 0),
    # first group (rows of 13 columns with a 16-column pitch), two layers with ReLU, unnormalised input with an
    # offset-free scale of 8; elementwise_affine=False; time-major
    ("stack_tm", [LN(13, num_layers=2, nonlin="ReLU"), LIN(20), LN(20, nonlin="Softsign", elementwise_affine=False),
                  LIN(7)], 13, False, 34, [7, 11, 3], 8.0, 2),
]
# new-style model of the trainer case (409 questions -> 67 acoustic features)
TRAINER_GROUPS = [LIN(32, "Tanh"), LN(32), LIN(32, "ELU"), LN(32, nonlin="ReLU"), LIN(67)]


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
    out_shape, from a generator seeded with 400 + index"""
    g = torch.Generator().manual_seed(400 + index)
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


def layer_norm64(torch, x, gamma, beta, eps):
    """torch.nn.LayerNorm over the last extent, written out in float64: (y, mean, rstd)"""
    x = x.double()
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd
    if gamma is not None:
        y = y * gamma.double()
    if beta is not None:
        y = y + beta.double()
    return y, mean[..., 0], rstd[..., 0]


def layer_norm64_bwd(torch, dz, x, gamma, eps):
    """the gradients of layer_norm64 for dL/dz = dz (the gradient at the affine output, i.e. dy * act'(y)), written
    out in float64: (dx, dgamma, dbeta)"""
    _, mean, rstd = layer_norm64(torch, x, None, None, eps)
    dz = dz.double()
    xhat = (x.double() - mean[..., None]) * rstd[..., None]
    g = dz * gamma.double() if gamma is not None else dz
    dx = rstd[..., None] * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    D = x.shape[-1]
    return dx, (dz * xhat).reshape(-1, D).sum(0), dz.reshape(-1, D).sum(0)


# ---- kernel-level cases (tests/test_gpu_lnorm.py; the CPU side of them in tests/test_lnorm_config.py) -----------------
# relative error (2-norm of the difference over the 2-norm of the reference) per product, and the per-element bound
# as a multiple of max(1, max|ref|): the dense layers' bounds
REL_BOUND = {"y": 2e-6, "dx": 2e-6, "dgamma": 3e-6, "dbeta": 3e-6}
ELEM_BOUND = 2e-5
# (N, D) of the shape sweep: every width class of the kernel and its edges (64 lanes x 4 columns x 1, 2, 4, 8, 16),
# odd widths, one and two rows, fewer rows than waves in a workgroup, and 69 rows = two full slabs and a partial one
N_SLABS = 69
SWEEP = [(7, 63), (7, 64), (7, 65), (1, 67), (2, 67), (7, 67), (N_SLABS, 67), (7, 255), (N_SLABS, 256), (7, 257),
         (7, 512), (2, 1024), (7, 1025), (7, 2048), (1, 4096), (N_SLABS, 4096)]
# the ill-conditioned cases: rstd near 1 / sqrt(eps) amplifies rounding.  Only these may use the relaxed bound.
HAZARDS = ("D1", "D3", "constant_row", "offset_1e4")


def sweep_inputs(torch, N, D, seed=0):
    """well-conditioned rows: spread 0.75 .. 1.25 around per-row offsets within +-10; (x, gamma, beta, dy) in float32"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + D)
    x = torch.randn(N, D, generator=g) * (0.75 + 0.5 * torch.rand(N, 1, generator=g)) \
        + (2 * torch.rand(N, 1, generator=g) - 1) * 10
    return x, 1 + 0.5 * torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(N, D, generator=g)


def hazard_inputs(torch, name):
    """(x, gamma, beta, dy, eps) of a HAZARDS case"""
    g = torch.Generator().manual_seed(50 + HAZARDS.index(name))
    N, D = {"D1": (5, 1), "D3": (5, 3), "constant_row": (6, 67), "offset_1e4": (6, 256)}[name]
    x = torch.randn(N, D, generator=g) + 10 * torch.randn(N, 1, generator=g)
    if name == "constant_row":
        x[2] = 2.5            # (sums of 2.5 are exact in float32 in any order: the variance is exactly 0)
        x[4] = -3.7
    if name == "offset_1e4":
        x = torch.randn(N, D, generator=g) + 1e4
    return (x, 1 + 0.5 * torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(N, D, generator=g),
            1e-5)


def errors(got, ref):
    """(relative error in the 2-norm, largest element error over max(1, max|ref|)) of a float64 pair"""
    d = (got.double() - ref).abs()
    return (d.norm().item() / (ref.norm().item() + 1e-30)), d.max().item() / max(1.0, ref.abs().max().item())


def check(product, got, ref, case=None, torch32=None):
    """asserts `got` against the float64 `ref` at the dense layers' bounds; a HAZARDS case passes `case` and torch's
    own float32 result on the same data, and the bound becomes the larger of the dense one and twice torch's error
    (the factor 2: another summation order).  Returns the errors as fractions of their tolerance."""
    tol_rel, tol_el = REL_BOUND[product], ELEM_BOUND
    if torch32 is not None:
        assert case in HAZARDS, "only the named ill-conditioned cases may use the relaxed bound"
        r32, e32 = errors(torch32, ref)
        tol_rel, tol_el = max(tol_rel, 2 * r32), max(tol_el, 2 * e32)
    rel, el = errors(got, ref)
    print("lnorm {} {}: rel {:.3g} ({:.2f} of tol), elem {:.3g} ({:.2f} of tol)".format(
        case or tuple(ref.shape), product, rel, rel / tol_rel, el, el / tol_el))
    assert rel < tol_rel and el < tol_el, (product, case, rel, tol_rel, el, tol_el)
    return rel / tol_rel, el / tol_el


def reference64(torch, x, gamma, beta, dy, eps, act_name=None):
    """float64 forward and backward of LayerNorm + torch.nn.<act_name> on float32 draws:
    dict of y, mean, rstd, dx, dgamma, dbeta"""
    z, mean, rstd = layer_norm64(torch, x, gamma, beta, eps)
    y, dz = z, dy.double()
    if act_name is not None:
        zz = z.detach().clone().requires_grad_(True)
        y = getattr(torch.nn, act_name)()(zz)
        (da,) = torch.autograd.grad(y.sum(), zz)
        y, dz = y.detach(), dz * da
    dx, dgamma, dbeta = layer_norm64_bwd(torch, dz, x, gamma, eps)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)


def torch32(torch, x, gamma, beta, dy, eps, act_name=None):
    """torch's own float32 layer_norm (+ activation) and autograd on the CPU: dict of y, dx, dgamma, dbeta"""
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, gamma, beta)]
    y = torch.nn.functional.layer_norm(leaves[0], (x.shape[-1],), leaves[1], leaves[2], eps)
    if act_name is not None:
        y = getattr(torch.nn, act_name)()(y)
    y.backward(dy)
    return dict(y=y.detach(), dx=leaves[0].grad, dgamma=leaves[1].grad if gamma is not None else None,
                dbeta=leaves[2].grad if beta is not None else None)
