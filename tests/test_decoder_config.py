"""enc_dec_dyn.Config.DecoderConfig / ProjectionConfig and what hangs on them without a GPU: fields and defaults, the
refusals that remain, the parameter keys of the reference, the names a model asks its data readers for, and the
collation hook with which PhonemeDurationLabelGen(load_as_matrix=True) pads a batch of ragged attention matrices."""
import numpy as np
import pytest
import torch

import decoder_cases as dc
import encdec_spec as spec
from idiaptts_amd.src.data_preparation.phonemes.PhonemeDurationLabelGen import PhonemeDurationLabelGen
from idiaptts_amd.src.neural_networks.pytorch.ModularModelHandlerPyTorch import ModularModelHandlerPyTorch
from idiaptts_amd.src.neural_networks.pytorch.models import enc_dec_dyn, rnn_dyn

FIX = spec.load_fixture()
C = enc_dec_dyn.Config


def test_constants_and_exports():
    assert enc_dec_dyn.FIXED_ATTENTION == "FixedAttention"
    assert enc_dec_dyn.ATTENTION_GROUND_TRUTH == "ground_truth_durations"
    att = enc_dec_dyn.FixedAttention.Config("attention_matrix", 5).create_model()
    assert isinstance(att, enc_dec_dyn.FixedAttention) and att.allows_batched_forward()
    assert att.attention_ground_truth == "attention_matrix" and att.n_frames_per_step == 5
    assert len(list(att.parameters())) == 0


def test_decoder_config_fields_and_defaults():
    c = C.DecoderConfig(input_names=["a"], name="dec", attention_config=enc_dec_dyn.FIXED_ATTENTION)
    assert (c.attention_config, c.attention_args, c.teacher_forcing_input_names) == ("FixedAttention", {}, None)
    assert (c.n_frames_per_step, c.p_teacher_forcing, c.pre_net_config, c.projection_configs) == (1, 1.0, None, None)
    assert (c.input_names, c.output_names, c.batch_first, c.input_merge_type, c.process_group, c.config) == \
        (["a"], ["dec"], True, "cat", 0, None)
    c = dc.attention_only(enc_dec_dyn)            # plain strings mean lists of one name, as in the reference
    assert c.input_names == [str(n) for n in FIX["quirk/str_input_names"]] == ["phoneme_embeddings"]
    assert c.output_names == ["upsampled_phoneme_embeddings"]
    assert c.extra_input_names == ["attention_matrix"]
    p = C.ProjectionConfig(out_dim=3, name="proj")
    assert (p.input_names, p.output_names, p.is_autoregressive_input, p.out_dim) == (None, ["proj"], False, 3)
    with pytest.raises(AssertionError, match="output_names"):
        C.DecoderConfig(input_names=["a"], attention_config=enc_dec_dyn.FIXED_ATTENTION)    # no name, no output names
    with pytest.raises(TypeError, match="out_dim"):
        C.ProjectionConfig(name="proj")


def test_empty_teacher_forcing_list_is_refused():
    with pytest.raises(AssertionError, match="Empty list not allowed for teacher_forcing_input_names"):
        C.DecoderConfig(input_names=["a"], name="dec", attention_config=enc_dec_dyn.FIXED_ATTENTION,
                        teacher_forcing_input_names=[])


def test_refusals_that_remain():
    for kind in ("CombinerConfig", "SplitterConfig"):
        with pytest.raises(NotImplementedError, match=kind):
            getattr(C, kind)(input_names=["a"], output_names=["b"])
    with pytest.raises(NotImplementedError, match=r"DecoderConfig\(attention_config=None\)"):
        C.DecoderConfig(input_names=["a"], name="dec")            # a decoder without attention: the default
    with pytest.raises(NotImplementedError, match="DotProductAttention"):
        C.DecoderConfig(input_names=["a"], name="dec", attention_config="DotProductAttention")
    with pytest.raises(NotImplementedError, match="ProjectionConfig.*inputs of its own"):
        C.ProjectionConfig(out_dim=3, name="proj", input_names=["a"])
    with pytest.raises(ValueError, match="attention_args"):
        C.DecoderConfig(input_names=["a"], name="dec", attention_config=enc_dec_dyn.FIXED_ATTENTION).create_model()


def test_parameter_keys_are_the_references_and_its_state_dict_loads():
    for case, config in (("case1", dc.case1_config(enc_dec_dyn, rnn_dyn)), ("case2", dc.case2_config(enc_dec_dyn, rnn_dyn))):
        model = config.create_model()
        ref = spec.sub(FIX, case + "/sd/")
        assert list(model.state_dict()) == list(ref)
        model.load_state_dict({k: torch.as_tensor(v).float() for k, v in ref.items()})
    assert [n for n, _ in model.named_parameters()] == [str(n) for n in FIX["case2/param_names"]]
    decoder = model.Decoder
    assert decoder.is_autoregressive and decoder.decoder_dim == dc.A and decoder.decoder_output_name is None
    assert config.input_names == ["phonemes", "attention_matrix"] == model.input_names
    assert decoder.reads_module_outputs


def test_config_json_round_trips_a_decoder():
    from idiaptts_amd.src.neural_networks.pytorch import config_json
    config = dc.case2_config(enc_dec_dyn, rnn_dyn, 0.5)
    text = config_json.encode(config)
    assert '"py/object": "idiaptts.src.neural_networks.pytorch.models.enc_dec_dyn.Config.Config.DecoderConfig"' in text
    assert "ProjectionConfig" in text and "idiaptts_amd" not in text
    back = config_json.decode(text)
    assert config_json.encode(back) == text and back.Decoder.p_teacher_forcing == 0.5
    assert list(back.create_model().state_dict()) == list(config.create_model().state_dict())


def test_decoder_output_name_is_read_from_the_config_with_getattr():
    config = dc.decoder(enc_dec_dyn, rnn_dyn, 1.0)
    config.decoder_output_name = "decoder_states"
    assert config.create_model().decoder_output_name == "decoder_states"


def test_init_hidden_reaches_pre_net_and_projections():
    model = dc.case2_config(enc_dec_dyn, rnn_dyn).create_model()
    calls = []
    for name, module in (("pre_net", model.Decoder.pre_net), ("projection", model.Decoder.projections[0])):
        module.init_hidden = (lambda n: lambda batch_size=1: calls.append((n, batch_size)))(name)
    model.init_hidden(3)
    assert calls == [("pre_net", 3), ("projection", 3)]
    assert model.Decoder.model[1].hidden[0].shape == (1, 3, 4)


# ---- the collation hook ---------------------------------------------------------------------------------------------
class _Dataset:
    def __init__(self, readers):
        self.readers = readers

    def get_datareader_by_output_name(self, key):
        return self.readers[key]


class _PlainReader:
    min_frames = None
    other_pad_dims = None
    requires_seq_mask = False


def _matrices():
    return [PhonemeDurationLabelGen.durations_to_hard_attention_matrix(d) for d in ((2, 1, 3), (1, 1, 1, 4), (5,))]


def test_matrix_reader_pads_both_axes():
    reader = PhonemeDurationLabelGen(load_as_matrix=True)
    assert not hasattr(PhonemeDurationLabelGen(load_as_matrix=False), "unsorted_pad_sequence")
    mats = _matrices()
    shapes = torch.tensor([m.shape for m in mats])
    out = reader.unsorted_pad_sequence(mats, True, shapes)
    assert out.shape == (3, 7, 4) and out.dtype == np.float32
    for i, m in enumerate(mats):
        assert (out[i, :m.shape[0], :m.shape[1]] == m).all()
        assert out[i].sum() == m.sum()                      # zeros everywhere else
    tm = reader.unsorted_pad_sequence(mats, False, shapes)
    assert tm.shape == (7, 3, 4) and (tm.transpose(1, 0, 2) == out).all()


def test_prepare_batch_calls_the_hook_and_leaves_other_readers_bit_identical():
    rng = np.random.RandomState(3)
    mats = _matrices()
    feats = [rng.randn(m.shape[0], 5).astype(np.float32) for m in mats]
    dataset = _Dataset({"attention_matrix": PhonemeDurationLabelGen(load_as_matrix=True), "feats": _PlainReader()})
    batch = [({"attention_matrix": m, "feats": f, "_id_list": str(i)}, dataset)
             for i, (m, f) in enumerate(zip(mats, feats))]
    for batch_first in (True, False):
        data, lengths = ModularModelHandlerPyTorch.prepare_batch(batch, batch_first=batch_first)
        A = data["attention_matrix"]
        assert torch.is_tensor(A) and A.dtype == torch.float32
        assert tuple(A.shape) == ((3, 7, 4) if batch_first else (7, 3, 4))
        assert lengths["attention_matrix"].tolist() == [6, 7, 5] == lengths["feats"].tolist()
        # a reader without the hook: the bits of the stock padding, with and without a hooked reader in the batch
        stock = ModularModelHandlerPyTorch.unsorted_pad_sequence(list(feats), batch_first)
        assert data["feats"].dtype == stock.dtype and torch.equal(data["feats"], stock)
        alone, _ = ModularModelHandlerPyTorch.prepare_batch(
            [({"feats": f}, _Dataset({"feats": _PlainReader()})) for f in feats], batch_first=batch_first)
        assert torch.equal(alone["feats"], stock)
        bare, _ = ModularModelHandlerPyTorch.prepare_batch([{"feats": f} for f in feats], batch_first=batch_first)
        assert torch.equal(bare["feats"], stock)
