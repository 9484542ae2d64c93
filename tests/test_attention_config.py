"""Self-attention layer groups without a GPU: nn.modules.TransformerEncoderLayer has torch's state-dict keys, shapes
and initial values (the same draws from the same seed), a torch checkpoint loads key for key, the RNNDyn group has the
reference's keys, and everything the group does not take is refused by name at construction."""
import pytest
import torch

from idiaptts_amd import ops
from idiaptts_amd.nn.modules import TransformerEncoderLayer
from idiaptts_amd.native_ff import FlatFFModel
from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn import Config, RNNDyn, TransformerWrapper
from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn.Config import config_from_legacy_string
from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn.RNNDyn import Dropout

LC = Config.LayerConfig


def _group(**kw):
    kwargs = dict(d_model=32, nhead=2, dim_feedforward=48, batch_first=True)
    kwargs.update(kw)
    return LC("TransformerEncoderLayer", **kwargs)


@pytest.mark.parametrize("norm_first", [False, True])
def test_parameters_are_torchs(norm_first):
    torch.manual_seed(11)
    ref = torch.nn.TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=48, batch_first=True,
                                           norm_first=norm_first)
    torch.manual_seed(11)
    own = TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=48, batch_first=True, norm_first=norm_first)
    sd_ref, sd = ref.state_dict(), own.state_dict()
    assert list(sd.keys()) == list(sd_ref.keys())
    for k in sd:
        assert sd[k].shape == sd_ref[k].shape and sd[k].dtype == sd_ref[k].dtype, k
        assert torch.equal(sd[k], sd_ref[k]), k             # the same draws in the same order
    assert set(sd) >= {"self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                       "self_attn.out_proj.bias", "linear1.weight", "linear2.bias", "norm1.weight", "norm2.bias"}
    assert sd["self_attn.in_proj_weight"].shape == (96, 32)
    # initial-value ranges: xavier_uniform on the in-projection, zero biases in the attention, torch.nn.Linear's
    # uniform(-1 / sqrt(fan_in), ..) elsewhere, ones and zeros in the norms
    bound = (6.0 / (96 + 32)) ** 0.5
    assert sd["self_attn.in_proj_weight"].abs().max() <= bound and sd["self_attn.in_proj_weight"].abs().max() > 0.8 * bound
    assert not sd["self_attn.in_proj_bias"].any() and not sd["self_attn.out_proj.bias"].any()
    assert sd["linear1.weight"].abs().max() <= 32 ** -0.5 and sd["linear2.weight"].abs().max() <= 48 ** -0.5
    assert (sd["norm1.weight"] == 1).all() and not sd["norm2.bias"].any()
    own.load_state_dict(ref.state_dict())                   # key for key, strict
    assert own.p == 0.1 and TransformerEncoderLayer(32, 2).dim_feedforward == 2048


def test_group_has_the_reference_keys_and_slots():
    cfg = Config(in_dim=6, batch_first=True, layer_configs=[
        LC("Linear", out_dim=32, nonlin="Tanh"), _group(num_layers=2, dropout=0.25, mask_padding=True, layer_dropout=0.0),
        LC("Linear", out_dim=5)])
    model = RNNDyn(cfg)
    group = model[1]
    assert isinstance(group, TransformerWrapper) and group.out_dim == 32 and group.mask_padding
    assert [type(m).__name__ for m in group.module] == ["TransformerEncoderLayer", "Dropout"] * 2
    assert all(m.p == 0.0 for m in group.module if isinstance(m, TransformerEncoderLayer))
    assert [m.p for m in group.module if isinstance(m, Dropout)] == [0.25, 0.25]
    # salts: the Linear layer is 0, the blocks 1 and 2 (their dropouts share the block's), the last Linear 3
    assert [m.salt for m in group.module] == [1, 1, 2, 2]
    keys = list(model.state_dict().keys())
    torch_group = torch.nn.Sequential(*[torch.nn.TransformerEncoderLayer(32, 2, 48, batch_first=True)
                                        if i % 2 == 0 else torch.nn.Dropout(0.25) for i in range(4)])
    expected = ["2.module." + k for k in torch_group.state_dict().keys()]
    assert [k for k in keys if k.startswith("2.")] == expected
    assert "2.module.2.self_attn.out_proj.weight" in keys and "2.module.0.norm2.bias" in keys
    assert FlatFFModel.from_module(model) is None           # trains on the module path
    # the defaults: the reference's quirks
    plain = TransformerWrapper(32, _group(), batch_first=True)
    assert not plain.mask_padding and plain.module[0].p == 0.1 and len(plain.module) == 1
    # without a batch_first among the kwargs the model's layout is the block's
    assert TransformerWrapper(32, LC("TransformerEncoderLayer", d_model=32, nhead=2), batch_first=True).module[0].batch_first
    assert not TransformerWrapper(32, LC("TransformerEncoderLayer", d_model=32, nhead=2), False).module[0].batch_first


@pytest.mark.parametrize("build,needle", [
    (lambda: TransformerWrapper(24, _group(), True), "d_model=32 does not match the group's input of 24"),
    (lambda: TransformerWrapper(32, _group(batch_first=False), True), "batch_first=False in a model with batch_first=True"),
    (lambda: TransformerWrapper(32, _group(batch_first=True), False), "batch_first=True in a model with batch_first=False"),
    (lambda: TransformerWrapper(32, _group(nhead=3), True), "divisible by nhead = 3"),
    (lambda: TransformerEncoderLayer(32, 5), "divisible by nhead = 5"),
    (lambda: TransformerWrapper(32, _group(layer_dropout=1.0), True), "layer_dropout=1.0"),
    (lambda: TransformerWrapper(32, LC("TransformerEncoderLayer", nhead=2), True), "d_model and nhead are required"),
])
def test_value_errors(build, needle):
    with pytest.raises(ValueError, match=needle):
        build()


@pytest.mark.parametrize("build,needle", [
    (lambda: TransformerWrapper(32, _group(activation="gelu"), True), "activation='gelu'"),
    (lambda: TransformerEncoderLayer(32, 2, activation=torch.nn.functional.relu), "callable activation"),
    (lambda: TransformerWrapper(32, _group(bias=False), True), "bias=False"),
    (lambda: TransformerWrapper(32, _group(nonlin="ReLU"), True), "nonlin=ReLU"),
    (lambda: TransformerWrapper(12, _group(d_model=12, nhead=2), True), "12 / 2"),               # dh 6
    (lambda: TransformerEncoderLayer(20, 2), "20 / 2"),                                          # dh 10
    (lambda: TransformerEncoderLayer(288, 2), "288 / 2"),                                        # dh 144
    (lambda: TransformerEncoderLayer(1040, 65), "d_model = 1040"),
    (lambda: ops.attention_check_envelope(64, 4, T=32769), "T = 32769"),
    (lambda: ops.attention_check_envelope(64, 4, T=5, B=16384), r"B \* nhead = 16384 \* 4"),
])
def test_refusals_by_name(build, needle):
    with pytest.raises(NotImplementedError, match=needle):
        build()


def test_rnndyn_dispatch_and_legacy_string():
    with pytest.raises(ValueError, match="d_model=32"):
        RNNDyn(Config(in_dim=6, layer_configs=[_group()]))
    with pytest.raises(NotImplementedError, match="TransformerEncoderLayer"):
        config_from_legacy_string(6, "RNNDYN-1_TransformerEncoderLayer_32-1_FC_5")
    assert ops.ATTENTION_MAX_HEAD_DIM == 128
