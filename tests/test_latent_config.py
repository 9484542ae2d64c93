"""Utterance embeddings on the CPU side: the PoolLast / PoolMean / VAE groups' layout and state-dict keys against the
reference's (tests/golden/latent_fixture.npz), the configurations refused by name, NamedForwardWrapper's tuple
outputs, VAEKLDLoss's Config and annealing, and the enc_dec_dyn container's bookkeeping.  Nothing here computes."""
import copy

import pytest
import torch

from idiaptts_amd.nn.modules import LinearAct, MeanPooling, SelectLastPooling, VanillaVAE
from idiaptts_amd.src.neural_networks.pytorch import config_json
from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
from idiaptts_amd.src.neural_networks.pytorch.loss.VAEKLDLoss import VAEKLDLoss
from idiaptts_amd.src.neural_networks.pytorch.models import enc_dec_dyn, rnn_dyn
from idiaptts_amd.src.neural_networks.pytorch.models.NamedForwardWrapper import NamedForwardWrapper
from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn import Config, RNNDyn, config_from_legacy_string

import latent_cases as lc

L = Config.LayerConfig


def _model(layers, in_dim=4, batch_first=True):
    return RNNDyn(Config(in_dim=in_dim, batch_first=batch_first, layer_configs=layers))


@pytest.fixture(scope="module")
def fix():
    return lc.load_fixture()


@pytest.mark.parametrize("name", sorted(lc.SINGLE))
@pytest.mark.parametrize("batch_first", [True, False])
def test_state_dict_keys_and_shapes_equal_the_references(fix, name, batch_first):
    model = lc.single_config(rnn_dyn, name, batch_first).create_model()
    ref = lc.sub(fix, name + "/sd/")
    sd = model.state_dict()
    assert list(sd) == list(ref)
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k].shape, k
    model.load_state_dict({k: torch.from_numpy(v) for k, v in ref.items()}, strict=True)


def test_group_layout():
    model = lc.single_config(rnn_dyn, "gru_poollast_vae").create_model()
    pool, vae = model[1], model[2]
    assert isinstance(pool.module[0], SelectLastPooling) and len(pool.module) == 1 and pool.out_dim == 8
    assert isinstance(vae.module[0], VanillaVAE) and len(vae.module) == 1 and vae.out_dim == 4
    lin = vae.module[0].linear
    assert isinstance(lin, LinearAct) and lin.bias is None and tuple(lin.weight.shape) == (8, 8)
    assert pool.module[0].extra_repr() == "batch_first=True"
    assert not pool.runs_on_rows() and not vae.runs_on_rows()
    model = lc.single_config(rnn_dyn, "lin_poolmean_vae", batch_first=False).create_model()
    assert isinstance(model[1].module[0], MeanPooling) and model[1].module[0].time_dim == 0
    assert tuple(model[2].module[0].linear.weight.shape) == (6, 6)
    # the other spelling of the type, and dropout behind a pooling layer as in the reference
    model = _model([L("PoolMean", batch_first=True, dropout=0.5), L("VanillaVAE", out_dim=2)])
    assert isinstance(model[0].module[1], torch.nn.Dropout) and list(model.state_dict()) == ["2.module.0.linear.weight"]
    # such models never take the flat feed-forward step
    from idiaptts_amd.native_ff import FlatFFModel
    assert FlatFFModel.from_module(model) is None
    assert FlatFFModel.from_module(lc.single_config(rnn_dyn, "lin_poolmean_vae").create_model()) is None


def test_output_length_is_ones_without_touching_the_argument():
    pool = SelectLastPooling(batch_first=True)
    lens = torch.tensor([5, 3, 9])
    out = pool.get_output_length(lens)
    assert out.tolist() == [1, 1, 1] and lens.tolist() == [5, 3, 9]        # (the reference's fill_ overwrites lens)
    assert pool.get_output_length(9) == 1 and pool.get_output_length([4, 2]) == [1, 1]
    assert pool.get_output_length(None) is None
    x = torch.zeros(3, 9, 2)
    picked = pool.select_inputs(x, seq_lengths_input=lens, max_length_inputs=9)
    assert picked[0] is x and picked[1] is lens
    assert MeanPooling(False).select_inputs(x)[1] is None


@pytest.mark.parametrize("layers,words", [
    ([L("VAE", out_dim=3), L("Linear", out_dim=4)], ["VAE", "last group"]),
    ([L("Linear", out_dim=4), L("VanillaVAE", out_dim=3), L("PoolLast", batch_first=True)], ["VanillaVAE", "last"]),
    ([L("VAE", out_dim=3, num_layers=2)], ["VAE", "num_layers"]),
    ([L("VAE", out_dim=3, nonlin="Tanh")], ["VAE", "nonlin"]),
    ([L("VAE", out_dim=3, dropout=0.1)], ["VAE", "dropout"]),
    ([L("PoolLast", nonlin="ReLU", batch_first=True)], ["PoolLast", "nonlin"]),
    ([L("PoolMean", nonlin="Tanh", batch_first=True)], ["PoolMean", "nonlin"]),
    ([L("PoolMean", num_layers=2, batch_first=True)], ["PoolMean", "num_layers"]),
])
def test_configurations_that_fail_late_in_the_reference_are_refused_by_name(layers, words):
    with pytest.raises(ValueError) as e:
        _model(layers)
    for word in words:
        assert word in str(e.value), str(e.value)


@pytest.mark.parametrize("layer", [
    L("Mask", mask_value=0.0), L("AlwaysDropout", p=0.5), L("SigmoidNorm"), L("LinearNorm"),
    L("ApplyFunction", fn="exp"), L("Embedding", num_embeddings=4, embedding_dim=3), L("Tanh"), L("ReLU"),
    L("Softmax", dim=2), L("BatchNorm1d", out_dim=4), L("GroupNorm", num_groups=2, num_channels=4), L("GELU"),
], ids=lambda l: l.type)
def test_other_special_types_stay_refused(layer):
    with pytest.raises(NotImplementedError, match=layer.type):
        _model([layer])


def test_legacy_string_has_no_spelling_for_the_new_groups():
    for s in ("RNNDYN-1_PoolLast_8", "RNNDYN-1_PoolMean_8", "RNNDYN-1_VAE_4", "RNNDYN-1_FC_8-1_VanillaVAE_4"):
        with pytest.raises(NotImplementedError):
            config_from_legacy_string(10, s, True)


class _Returns(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.n = n

    def forward(self, input_, **kwargs):
        outs = tuple(input_ + i for i in range(self.n))
        return (outs if self.n != 1 else outs[0]), kwargs


def _wrapper(output_names, n_outputs):
    cfg = NamedForwardWrapper.Config(Config(in_dim=2, layer_configs=[L("Linear", out_dim=2)]), ["x"], True,
                                     name="m", output_names=output_names)
    w = NamedForwardWrapper(cfg)
    w.model = _Returns(n_outputs)
    return w


def test_tuple_outputs_map_one_to_one_onto_the_names():
    x = torch.zeros(2, 3, 2)
    data, lengths, max_lengths = {"x": x}, {"x": torch.tensor([3, 2])}, {"x": 3}
    _wrapper(["z", "mu", "log_var"], 3)(data, lengths, max_lengths)
    assert [float(data[n].mean()) for n in ("z", "mu", "log_var")] == [0.0, 1.0, 2.0]
    for n in ("z", "mu", "log_var"):
        assert lengths[n] is lengths["x"] and max_lengths[n] == 3
    for names, n in ((["z", "mu"], 3), (["a", "b", "c", "d"], 3), (["z"], 2)):
        with pytest.raises(ValueError, match="{} output name".format(len(names))):
            _wrapper(names, n)({"x": x}, dict(lengths), dict(max_lengths))
    # a single tensor goes to every name, as before
    data = {"x": x}
    _wrapper(["a", "b"], 1)(data, dict(lengths), dict(max_lengths))
    assert data["a"] is data["b"]


@pytest.mark.parametrize("step,factor", [
    (0, 0.0),            # not past the first point (step > points[0] is strict)
    (100, 0.0),          # step == annealing_points[0]
    (150, 0.0),          # between the points, but no multiple of annealing_steps
    (200, 100 / 400),    # between the points
    (300, 200 / 400),
    (500, 1.0),          # step == annealing_points[1]: still the linear branch, which reaches 1 there
    (505, 0.0),
    (600, 1.0),          # beyond the second point
    (1000, 1.0),
])
def test_anneal_table(step, factor):
    loss = VAEKLDLoss.Config("kl", ["mu", "lv"], annealing_steps=100, annealing_points=(100, 500)).create_loss()
    assert loss.annealing_factor(step) == factor
    assert float(loss._anneal(torch.tensor(2.0), step)) == 2.0 * factor


def test_anneal_of_the_references_test_recipe():
    loss = VAEKLDLoss.Config("kl", ["mu", "lv"], type_="VAEKLDLoss", start_step=10, annealing_points=(-1, 100),
                             annealing_steps=10, seq_mask="m").create_loss()
    assert loss.annealing_factor(10) == 11 / 101 and loss.annealing_factor(0) == 1 / 101
    assert loss.start_step == 10 and loss.seq_mask == "m" and loss.reduction == "mean_per_frame"
    assert isinstance(loss, VAEKLDLoss) and not isinstance(loss, NamedLoss)


def test_loss_config():
    cfg = VAEKLDLoss.Config("kl", ["mu", "lv"])
    assert (cfg.annealing_steps, cfg.annealing_points, cfg.batch_first, cfg.start_step, cfg.type) == \
        (200, (25000, 150000), True, 0, "VAEKLDLoss")
    # without a mask there are no lengths to divide by: the reference's Config falls back to 'mean'
    assert cfg.reduction == "mean"
    assert VAEKLDLoss.Config("kl", ["mu", "lv"], reduction="mean_per_sample").reduction == "mean"
    assert VAEKLDLoss.Config("kl", ["mu", "lv"], reduction="sum").reduction == "sum"
    assert VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m", reduction="mean_per_sample").reduction == "mean_per_sample"
    with pytest.raises(ValueError):                       # NamedLoss itself keeps its refusal
        NamedLoss(NamedLoss.Config("l", "MSELoss", ["a", "b"]))
    with pytest.raises(NotImplementedError, match="VAEKLDLoss"):      # .. and gains no new type
        NamedLoss(NamedLoss.Config("l", "VAEKLDLoss", ["a", "b"], seq_mask="m"))
    with pytest.raises(ValueError, match=r"\(5, 1\)"):
        VAEKLDLoss.Config("kl", ["mu", "lv"], annealing_points=(5, 1))
    with pytest.raises(ValueError, match="-3"):
        VAEKLDLoss.Config("kl", ["mu", "lv"], annealing_steps=-3)
    with pytest.raises(NotImplementedError, match="median"):
        VAEKLDLoss.Config("kl", ["mu", "lv"], reduction="median").create_loss()
    with pytest.raises(ValueError, match="mu, log_var"):
        VAEKLDLoss.Config("kl", ["mu"]).create_loss()


def test_row_weights_of_a_pooled_embedding_under_a_frame_mask():
    """the reference multiplies [B, 1, 1] KL values by the [B, T, 1] mask: an utterance's weight is its mask summed"""
    mask = torch.tensor([[1., 1, 1, 0], [1, 0, 0, 0]]).unsqueeze(-1)
    mu = torch.zeros(2, 1, 3)
    lens = {"m": torch.tensor([3, 1])}
    w = VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m").create_loss()._row_weight(mu, mask, lens)
    assert torch.equal(w, torch.tensor([3., 1.]) / 4)
    w = VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m", reduction="mean").create_loss()._row_weight(mu, mask, lens)
    assert torch.equal(w, torch.tensor([3., 1.]) / 8)
    w = VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m", reduction="mean_per_sample").create_loss() \
        ._row_weight(mu, mask, lens)
    assert torch.allclose(w, torch.tensor([3. / 3, 1. / 1]) / 2)
    # frame-level latents: the mask itself; no mask: ones
    w = VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m", reduction="sum").create_loss() \
        ._row_weight(torch.zeros(2, 4, 3), mask, lens)
    assert torch.equal(w, mask.reshape(-1))
    w = VAEKLDLoss.Config("kl", ["mu", "lv"]).create_loss()._row_weight(torch.zeros(2, 4, 3), None, lens)
    assert torch.equal(w, torch.full((8,), 1 / 8))
    with pytest.raises(ValueError, match="4 frames"):
        VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m").create_loss()._row_weight(torch.zeros(2, 3, 3), mask, lens)


def test_chain_keys_order_and_input_names(fix):
    config = lc.chain_config(enc_dec_dyn, rnn_dyn)
    assert [[m.name for m in g] for g in config.process_groups] == [["encoder"], ["decoder"]]   # sorted by group
    assert config.encoder.output_names == ["emb_z", "emb_mu", "emb_logvar"]
    with pytest.raises(AttributeError):
        config.nobody
    model = config.create_model()
    ref = lc.sub(fix, "chain/sd/")
    sd = model.state_dict()
    assert list(sd) == list(ref)
    assert all(tuple(v.shape) == ref[k].shape for k, v in sd.items())
    assert model.batch_first is True
    assert model.input_names == ["acoustic_features", "questions"] == config.input_names
    assert model.encoder is model.chain[0] and model.decoder is model.chain[1]
    # the decoder reads emb_z, which the encoder wrote: it never takes the valid-rows path
    assert not model.encoder.reads_module_outputs and model.decoder.reads_module_outputs
    copy.deepcopy(config)


def test_input_names_of_a_three_module_chain():
    M, W = enc_dec_dyn.Config.ModuleConfig, enc_dec_dyn.Config.WrapperConfig
    lin = lambda i, o: Config(in_dim=i, layer_configs=[L("Linear", out_dim=o)])     # noqa: E731
    config = enc_dec_dyn.Config(modules=[
        M(name="post", input_names=["hidden", "speaker", "phonemes"], config=lin(9, 2), process_group=2,
          output_names=["pred"]),
        M(name="pass", input_names=["phonemes"], config=None, process_group=0, output_names=["phonemes_copy"]),
        W(lin(3, 4), ["phonemes_copy", "durations"], name="mid", process_group=1, output_names=["hidden"]),
    ])
    model = config.create_model()
    # read by some module, written by no earlier one, in the order of first use
    assert model.input_names == ["phonemes", "durations", "speaker"]
    assert [m.name for m in model.chain] == ["pass", "mid", "post"]
    assert [m.reads_module_outputs for m in model.chain] == [False, True, True]
    assert sorted(model.state_dict()) == ["mid.model.1.module.0.bias", "mid.model.1.module.0.weight",
                                          "post.model.1.module.0.bias", "post.model.1.module.0.weight"]
    # the pass-through writes its input under the new name with the input's lengths
    x = torch.ones(2, 3, 1)
    data, lengths, max_lengths = {"phonemes": x}, {"phonemes": torch.tensor([3, 2])}, {"phonemes": 3}
    model.chain[0](data, lengths, max_lengths)
    assert data["phonemes_copy"] is x and lengths["phonemes_copy"] is lengths["phonemes"]


def test_duplicate_module_name_and_unbuilt_module_kinds():
    M = enc_dec_dyn.Config.ModuleConfig
    with pytest.raises(ValueError, match="named enc"):
        enc_dec_dyn.Config(modules=[M(["a"], name="enc", output_names=["b"]),
                                    M(["b"], name="enc", output_names=["c"], process_group=1)]).create_model()
    for kind in ("DecoderConfig", "ProjectionConfig", "CombinerConfig", "SplitterConfig"):
        with pytest.raises(NotImplementedError, match=kind):
            getattr(enc_dec_dyn.Config, kind)(input_names=["a"], output_names=["b"])
    with pytest.raises(ValueError, match="batch_first"):
        enc_dec_dyn.Config(modules=[M(["a"], name="tm", output_names=["b"], config=Config(
            in_dim=2, batch_first=False, layer_configs=[L("Linear", out_dim=2)]))]).create_model()


def test_config_json_round_trips_a_chain():
    config = lc.chain_config(enc_dec_dyn, rnn_dyn)
    text = config_json.encode(config)
    assert '"py/object": "idiaptts.src.neural_networks.pytorch.models.enc_dec_dyn.Config.Config.ModuleConfig"' in text
    assert "idiaptts_amd" not in text
    back = config_json.decode(text)
    assert isinstance(back, enc_dec_dyn.Config) and config_json.encode(back) == text
    assert back.input_names == ["acoustic_features", "questions"]
    a, b = config.create_model().state_dict(), back.create_model().state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    enc = back.encoder.config.layer_configs
    assert [(g.type, g.out_dim, g.kwargs) for g in enc] == [("GRU", 8, {}), ("PoolLast", None, {"batch_first": True}),
                                                            ("VAE", 4, {})]
    # a loss config of the family
    kl = VAEKLDLoss.Config("kl", ["emb_mu", "emb_logvar"], seq_mask="m", **lc.KL_ARGS)
    back = config_json.decode(config_json.encode(kl))
    assert isinstance(back, VAEKLDLoss.Config) and list(back.annealing_points) == [-1, 100]
    assert back.create_loss().annealing_factor(10) == 11 / 101
