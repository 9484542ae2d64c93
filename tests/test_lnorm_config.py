"""LayerNorm layer groups on the CPU side: every case builds the reference's module layout with its seeded initial
weights (tests/golden/lnorm_fixture.npz), config.json round-trips the kwargs, out-of-scope configurations refuse,
FlatFFModel.from_module leaves such models to the module path, reference-style state dicts load strictly,
LayerNormAct on CPU tensors equals torch, and the float64 restatement the GPU tests compare against
(lnorm_cases.layer_norm64 / layer_norm64_bwd) is pinned to torch's own layer_norm and autograd in float64."""
import os

import numpy as np
import pytest
import torch

from lnorm_cases import (CASES, LIN, LN, SWEEP, _layers, case_config, check, layer_norm64, layer_norm64_bwd, reference64,
                         sweep_inputs, torch32, trainer_model_config)
from idiaptts_amd import lib, ops
from idiaptts_amd.native_ff import FlatFFModel
from idiaptts_amd.nn.modules import Conv1dAct, LayerNormAct, LinearAct
from idiaptts_amd.src.neural_networks.pytorch import config_json
from idiaptts_amd.src.neural_networks.pytorch.models import rnn_dyn
from idiaptts_amd.src.neural_networks.pytorch.models.NamedForwardWrapper import NamedForwardWrapper
from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn import Config, FFWrapper, RNNDyn


@pytest.fixture(scope="module")
def lnorm_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lnorm_fixture.npz"))


_TORCH_NAME = ((LayerNormAct, "LayerNorm"), (LinearAct, "Linear"), (Conv1dAct, "Conv1d"))


def _types(model):
    """'<group>.module.<k>:<torch.nn class>' as the fixture records the reference's modules"""
    out = []
    for k, m in model.named_modules():
        if ".module." in k:
            name = m.name if type(m).__name__ == "FusedActivation" else type(m).__name__
            for cls, torch_name in _TORCH_NAME:
                if isinstance(m, cls):
                    name = torch_name
            out.append("{}:{}".format(k, name))
    return out


def _sd(g, prefix):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_modules_and_seeded_initial_weights_equal_reference(lnorm_golden, case):
    name, seed = case[0], case[4]
    torch.manual_seed(seed)
    model = RNNDyn(case_config(Config, case))
    assert _types(model) == list(lnorm_golden[name + "/modules"])
    sd = model.state_dict()
    ref = _sd(lnorm_golden, name + "/sd/")
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert np.array_equal(sd[k].numpy(), ref[k]), k
    # the group's width is its input's; LayerNorm parameters are torch's ones and zeros
    for group, spec in zip(model.layer_groups, case[1]):
        if spec[0] == "LayerNorm":
            width = spec[4]["normalized_shape"]
            assert group.out_dim == (width[0] if isinstance(width, list) else width)
            assert isinstance(group, FFWrapper) and group.linear_layers() is None and group.runs_on_rows()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_state_dict_loads_strictly(lnorm_golden, case):
    model = RNNDyn(case_config(Config, case))
    sd = {k: torch.from_numpy(v) + 0.25 for k, v in _sd(lnorm_golden, case[0] + "/sd/").items()}
    assert model.load_state_dict(sd, strict=True).missing_keys == []
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_trainer_model_layout_equals_reference(lnorm_golden):
    cfg = trainer_model_config(rnn_dyn, NamedForwardWrapper)
    torch.manual_seed(1234)
    model = cfg.create_model()
    assert _types(model) == list(lnorm_golden["trainer/modules"])
    assert set(model.state_dict().keys()) == set(_sd(lnorm_golden, "trainer/init/"))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(lnorm_golden, "trainer/final/").items()}, strict=True)
    assert FlatFFModel.from_module(model, device="cpu") is None


def test_config_json_round_trips_the_kwargs():
    for case in CASES:
        cfg = case_config(Config, case)
        back = config_json.decode(config_json.encode(cfg))
        assert [(lc.type, lc.out_dim, lc.num_layers, lc.nonlin, lc.kwargs) for lc in back.layer_configs] == \
            [(lc.type, lc.out_dim, lc.num_layers, lc.nonlin, lc.kwargs) for lc in cfg.layer_configs]
        torch.manual_seed(3)
        a = RNNDyn(cfg)
        torch.manual_seed(3)
        b = RNNDyn(back)
        assert _types(a) == _types(b)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        for ma, mb in zip(a.modules(), b.modules()):
            if isinstance(ma, LayerNormAct):
                assert (ma.eps, ma.act, ma.normalized_shape, ma.elementwise_affine) == \
                    (mb.eps, mb.act, mb.normalized_shape, mb.elementwise_affine)


def test_group_layout_with_nonlin_and_dropout():
    lc = Config.LayerConfig("LayerNorm", num_layers=2, nonlin="tanh", dropout=0.1, normalized_shape=6, eps=1e-3)
    group = FFWrapper(6, lc, batch_first=True)
    mods = list(group.module)
    assert [type(m).__name__ for m in mods] == ["LayerNormAct", "FusedActivation", "Dropout"] * 2
    assert all(m.act == ops.ACT_TANH and m.eps == 1e-3 and m.normalized_shape == (6,) for m in mods[::3])
    assert mods[1].name == "Tanh" and group.out_dim == 6
    assert list(group.state_dict()) == ["module.0.weight", "module.0.bias", "module.3.weight", "module.3.bias"]
    assert torch.equal(mods[0].weight, torch.ones(6)) and torch.equal(mods[0].bias, torch.zeros(6))
    group.train()
    assert not group.runs_on_rows()          # dropout draws per position
    group.eval()
    assert group.runs_on_rows()
    # parameter names, shapes and values are torch.nn.LayerNorm's for every option
    for kwargs in (dict(), dict(elementwise_affine=False), dict(bias=False), dict(eps=1e-3)):
        a, b = LayerNormAct(5, act="ELU", **kwargs), torch.nn.LayerNorm(5, **kwargs)
        assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == \
            [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
        assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert LayerNormAct([5]).normalized_shape == LayerNormAct((5,)).normalized_shape == LayerNormAct(5).normalized_shape


def _model(groups, in_dim=8):
    return RNNDyn(Config(in_dim=in_dim, batch_first=True, layer_configs=_layers(Config, groups)))


def test_refusals():
    with pytest.raises(NotImplementedError, match=r"\(4, 8\)"):          # two normalised dimensions
        _model([LN([4, 8])])
    with pytest.raises(NotImplementedError, match=r"\(4, 8\)"):
        LayerNormAct((4, 8))
    with pytest.raises(NotImplementedError, match="4097"):
        _model([LIN(4097), LN(4097)])
    with pytest.raises(NotImplementedError, match="4097"):
        LayerNormAct(4097)
    LayerNormAct(4096)
    with pytest.raises(NotImplementedError, match="GELU"):
        _model([LN(8, nonlin="GELU")])
    with pytest.raises(NotImplementedError, match="GELU"):
        LayerNormAct(8, act="GELU")
    with pytest.raises(ValueError, match=r"(?s)12.*\b8\b"):               # normalized_shape != in_dim
        _model([LN(12)])
    with pytest.raises(ValueError, match=r"(?s)\b8\b.*16"):
        _model([LIN(16), LN(8)])
    with pytest.raises(NotImplementedError, match="GroupNorm"):
        _model([("GroupNorm", None, 1, None, dict(num_groups=2, num_channels=8))])
    with pytest.raises(NotImplementedError, match="BatchNorm1d"):
        _model([("BatchNorm1d", None, 1, None, {})])


def test_the_library_refuses_a_wider_row_before_any_device_work():
    """argument checks come first: no pointer is looked at, nothing is launched (this runs without a GPU)"""
    L = lib.load()
    assert L.itts_layernorm_fwd(None, 4097, None, None, None, 4097, None, None, 4, 4097, 1e-5, 0, None) == -1
    assert b"4097" in L.itts_last_error()
    assert L.itts_layernorm_bwd(None, 4097, None, 4097, None, 0, None, None, None, None, 4097, None, None, 4, 4097, 0,
                                None, None) == -1
    assert b"4097" in L.itts_last_error()
    assert L.itts_layernorm_fwd(None, 8, None, None, None, 8, None, None, 4, 8, 1e-5, 14, None) == -1
    assert b"unknown activation" in L.itts_last_error()
    assert L.itts_layernorm_fwd(None, 4, None, None, None, 8, None, None, 4, 8, 1e-5, 0, None) == -1     # pitch < D
    assert L.itts_layernorm_fwd(None, 8, None, None, None, 8, None, None, 0, 8, 1e-5, 0, None) == 0     # no rows
    # one slab of 2 * D floats per 32 rows up to 1024 slabs, then per 64, 96, ... rows
    for N, slabs in [(1, 1), (32, 1), (33, 2), (69, 3), (32768, 1024), (32769, 513), (51200, 800)]:
        assert L.itts_layernorm_workspace_bytes(N, 67) == slabs * 2 * 67 * 4, N
    assert L.itts_layernorm_workspace_bytes(0, 67) == 0


@pytest.mark.parametrize("act", [None, "ReLU", "Tanh", "ELU", "Softsign"])
@pytest.mark.parametrize("kwargs", [dict(), dict(elementwise_affine=False), dict(bias=False), dict(eps=1e-3)])
def test_layer_norm_act_on_cpu_tensors_equals_torch(act, kwargs):
    torch.manual_seed(4)
    m = LayerNormAct(11, act=act, **kwargs)
    ref = torch.nn.LayerNorm(11, **kwargs)
    with torch.no_grad():
        for p, q in zip(m.parameters(), ref.parameters()):
            p.copy_(torch.randn_like(p))
            q.copy_(p)
    for shape in ((5, 11), (3, 4, 11)):
        x = (torch.randn(shape) * 3 + 2).requires_grad_(True)
        x2 = x.detach().clone().requires_grad_(True)
        y = m(x)
        want = ref(x2)
        if act is not None:
            want = getattr(torch.nn, act)()(want)
        assert torch.equal(y, want)
        y.sum().backward()
        want.sum().backward()
        assert torch.equal(x.grad, x2.grad)


def test_flat_model_leaves_layernorm_models_to_the_module_path():
    assert FlatFFModel.from_module(_model([LIN(8, "Tanh"), LN(8), LIN(3)]), device="cpu") is None
    assert FlatFFModel.from_module(_model([LN(8)]), device="cpu") is None
    assert FlatFFModel.from_module(_model([LIN(8, "Tanh"), LIN(3)]), device="cpu") is not None


@pytest.mark.parametrize("D", [1, 3, 67, 256])
@pytest.mark.parametrize("affine", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_float64_restatement_equals_torch_in_float64(D, affine, eps):
    """what tests/test_gpu_lnorm.py compares the kernels against, pinned to torch.nn.functional.layer_norm and its
    autograd in float64 within 1e-12 (relative to the largest value of each product); float32 draws on both sides"""
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(9, D, generator=g) * 2 + 10).double()
    gamma = (torch.randn(D, generator=g) + 1).double() if affine[0] else None
    beta = torch.randn(D, generator=g).double() if affine[1] else None
    dz = torch.randn(9, D, generator=g).double()
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, gamma, beta)]
    want = torch.nn.functional.layer_norm(leaves[0], (D,), leaves[1], leaves[2], eps)
    want.backward(dz)
    y, mean, rstd = layer_norm64(torch, x, gamma, beta, eps)
    dx, dgamma, dbeta = layer_norm64_bwd(torch, dz, x, gamma, eps)

    def close(a, b):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())

    close(y, want.detach())
    close(dx, leaves[0].grad)
    if gamma is not None:
        close(dgamma, leaves[1].grad)
    if beta is not None:
        close(dbeta, leaves[2].grad)
    close(mean, x.mean(-1))
    close(rstd, 1 / torch.sqrt(x.var(-1, unbiased=False) + eps))


@pytest.mark.parametrize("N,D", SWEEP)
def test_torch_float32_stays_inside_the_dense_bounds_on_the_sweep_inputs(N, D):
    """the bounds tests/test_gpu_lnorm.py holds the kernels to are attainable in float32 on exactly its inputs"""
    x, gamma, beta, dy = sweep_inputs(torch, N, D)
    assert D >= 16
    for act in (None, "Tanh"):
        ref = reference64(torch, x, gamma, beta, dy, 1e-5, act)
        got = torch32(torch, x, gamma, beta, dy, 1e-5, act)
        for product in ("y", "dx", "dgamma", "dbeta"):
            check(product, got[product], ref[product])
