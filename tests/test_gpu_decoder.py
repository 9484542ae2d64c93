"""The fixed-attention decoder of enc_dec_dyn on the GPU against the reference's float64 outputs in
tests/golden/decoder_fixture.npz (cases 1 - 4 of tests/golden/make_golden_decoder.py), and the recurrent layers stepped
one frame at a time on per-row states.

The bound of every comparison is the larger of the dense layers' (2e-6 relative in the 2-norm, 2e-5 * max(1, max|ref|)
per element) and twice the error of the same flow in torch float32 on the CPU (tests/encdec_spec.py, or torch.nn's
recurrent layers), both taken against float64 -- the rule of tests/test_gpu_mol.py and tests/test_gpu_wavenet.py.  The
float32 error is computed here, never taken from the code under test.  Cases 3 and 4 run a feedback loop of four
steps; every comparison prints the fraction of its tolerance it used."""
import numpy as np
import pytest
import torch

import decoder_cases as dc
import encdec_spec as spec
from idiaptts_amd.nn.modules import GRU, LSTM, RNN
from idiaptts_amd.src.neural_networks.pytorch.models import enc_dec_dyn, rnn_dyn

pytestmark = pytest.mark.gpu

FIX = spec.load_fixture()
F32, F64 = torch.float32, torch.float64
GIVEN = ("phonemes", "attention_matrix", "acoustic_features")


def _model(config, case, gpu):
    model = config.create_model()
    ref = spec.sub(FIX, case + "/sd/")
    assert list(model.state_dict()) == list(ref)                         # the reference's keys ..
    assert len(list(model.parameters())) == sum(1 for k in ref if not k.endswith(("h_0", "c_0")))
    model.load_state_dict({k: torch.as_tensor(v).float() for k, v in ref.items()})     # .. and its state dict loads
    return model.to(gpu)


def _dicts(gpu, with_target):
    names = [n for n in GIVEN if with_target or n != "acoustic_features"]
    data = {n: torch.as_tensor(FIX["in/" + n]).to(gpu) for n in names}
    lens = {"phonemes": torch.as_tensor(FIX["in/phoneme_lens"]), "attention_matrix": torch.as_tensor(FIX["in/frame_lens"]),
            "acoustic_features": torch.as_tensor(FIX["in/frame_lens"])}
    maxs = {"phonemes": torch.tensor(5), "attention_matrix": torch.tensor(20), "acoustic_features": torch.tensor(20)}
    return data, {n: lens[n].clone() for n in names}, {n: maxs[n].clone() for n in names}


def _spec_inputs(dtype):
    return spec.tensors(spec.sub(FIX, "in/"), dtype), torch.as_tensor(FIX["in/frame_lens"])


def _check_outputs(case, data, lens, maxs, out32):
    ref = spec.sub(FIX, case + "/out/")
    assert sorted(k for k in data if k not in GIVEN) == sorted(ref)
    used = [spec.check("{} {}".format(case, k), data[k].detach(), torch.as_tensor(ref[k]), out32[k].detach())
            for k in sorted(ref)]
    for k, v in spec.sub(FIX, case + "/len/").items():
        assert torch.as_tensor(lens[k]).tolist() == v.tolist(), (case, "length of", k)
    for k, v in spec.sub(FIX, case + "/maxlen/").items():
        assert int(maxs[k]) == int(v), (case, "max length of", k)
    return max(used)


def test_case1_attention_feeding_a_parallel_decoder(gpu):
    model = _model(dc.case1_config(enc_dec_dyn, rnn_dyn), "case1", gpu)
    data, lens, maxs = _dicts(gpu, False)
    model.init_hidden(2)
    with torch.no_grad():
        model(data, lens, maxs)
    out32 = spec.case1(spec.tensors(spec.sub(FIX, "case1/sd/"), F32), *_spec_inputs(F32))
    _check_outputs("case1", data, lens, maxs, out32)


def test_case2_batched_pass_loss_and_every_parameter_gradient(gpu):
    model = _model(dc.case2_config(enc_dec_dyn, rnn_dyn), "case2", gpu)
    data, lens, maxs = _dicts(gpu, True)
    model.init_hidden(2)
    model(data, lens, maxs)
    sd32 = spec.tensors(spec.sub(FIX, "case2/sd/"), F32)
    names = [str(n) for n in FIX["case2/param_names"]]
    for n in names:
        sd32[n].requires_grad_(True)
    inputs32, frame_lens = _spec_inputs(F32)
    out32 = spec.decoder_batched(sd32, inputs32, frame_lens)
    _check_outputs("case2", data, lens, maxs, out32)
    mask = torch.as_tensor(FIX["in/mask"]).to(gpu)
    loss = spec.mse(data["pred_acoustic_features"], data["acoustic_features"], mask)
    loss32 = spec.mse(out32["pred_acoustic_features"], inputs32["acoustic_features"], inputs32["mask"])
    spec.check("case2 mse", loss.detach().reshape(1), torch.as_tensor(FIX["case2/mse"]).reshape(1),
               loss32.detach().reshape(1))
    loss.backward()
    loss32.backward()
    params = dict(model.named_parameters())
    assert list(params) == names
    for n in names:
        assert params[n].grad is not None, n
        spec.check("case2 grad " + n, params[n].grad, torch.as_tensor(FIX["case2/grad/" + n]), sd32[n].grad)


class _RecordUniform:
    def __enter__(self):
        self.orig, self.draws = np.random.uniform, []

        def uniform(*args, **kwargs):
            self.draws.append(self.orig(*args, **kwargs))
            return self.draws[-1]
        np.random.uniform = uniform
        return self

    def __exit__(self, *exc):
        np.random.uniform = self.orig


def test_case3_inference_runs_the_loop_without_the_teacher_forcing_input(gpu):
    model = _model(dc.case2_config(enc_dec_dyn, rnn_dyn), "case2", gpu)
    data, lens, maxs = _dicts(gpu, True)             # the caller's dictionaries hold the target ..
    target = data["acoustic_features"]
    model.init_hidden(2)
    with torch.no_grad(), _RecordUniform() as rec:
        model.inference(data, lens, maxs)
    assert rec.draws == []                           # .. the module does not see it: no draw, pure auto-regression
    assert data["acoustic_features"] is target and "acoustic_features" in lens and "acoustic_features" in maxs
    out32 = spec.decoder_iterative(spec.tensors(spec.sub(FIX, "case2/sd/"), F32), _spec_inputs(F32)[0], False)
    used = _check_outputs("case3", data, lens, maxs, out32)
    print("case3: four feedback steps used {:.2f} of the tolerance".format(used))


def test_case4_scheduled_sampling_makes_the_references_choices(gpu):
    model = _model(dc.case2_config(enc_dec_dyn, rnn_dyn, p_teacher_forcing=0.5), "case2", gpu)
    data, lens, maxs = _dicts(gpu, True)
    model.init_hidden(2)
    np.random.seed(1234)
    with torch.no_grad(), _RecordUniform() as rec:
        model(data, lens, maxs)
    assert len(rec.draws) == -(-20 // dc.N_STEP) - 1 == 3          # one per step after the first
    assert rec.draws == [float(d) for d in FIX["case4/draws"]]
    out32 = spec.decoder_iterative(spec.tensors(spec.sub(FIX, "case2/sd/"), F32), _spec_inputs(F32)[0], True, 0.5,
                                   rec.draws)
    used = _check_outputs("case4", data, lens, maxs, out32)
    print("case4: four feedback steps used {:.2f} of the tolerance".format(used))


def test_the_iterative_pass_under_gradients_is_refused_by_name(gpu):
    model = _model(dc.case2_config(enc_dec_dyn, rnn_dyn, p_teacher_forcing=0.5), "case2", gpu)
    data, lens, maxs = _dicts(gpu, True)
    model.init_hidden(2)
    with pytest.raises(NotImplementedError, match="p_teacher_forcing < 1"):
        model(data, lens, maxs)
    with pytest.raises(TypeError, match="unsorted_pad_sequence"):
        data["attention_matrix"] = [a for a in data["attention_matrix"]]
        model(data, lens, maxs)


# ---- stepping a recurrent layer on per-row states ------------------------------------------------------------------
B, T, D, H = 3, 6, 7, 20
LAYERS = {
    "lstm": (LSTM, torch.nn.LSTM, {}),
    "gru": (GRU, torch.nn.GRU, {}),
    "rnn_tanh": (RNN, torch.nn.RNN, {"nonlinearity": "tanh"}),
    "rnn_relu": (RNN, torch.nn.RNN, {"nonlinearity": "relu"}),
    "lstm_2layer": (LSTM, torch.nn.LSTM, {"num_layers": 2}),
    "gru_2layer": (GRU, torch.nn.GRU, {"num_layers": 2}),
    "lstm_bidirectional": (LSTM, torch.nn.LSTM, {"bidirectional": True}),
    "gru_bidirectional": (GRU, torch.nn.GRU, {"bidirectional": True}),
}


def _stepped(layer, x, h0):
    """one call per frame, carrying the state: -> outputs [B, T, .]"""
    outs, state = [], h0
    for t in range(x.shape[1]):
        out, state = layer(x[:, t:t + 1], state)
        outs.append(out)
    return torch.cat(outs, dim=1), state


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_stepping_on_per_row_states_matches_one_call(gpu, name):
    ours, theirs, kw = LAYERS[name]
    torch.manual_seed(sorted(LAYERS).index(name))
    ref32 = theirs(D, H, batch_first=True, **kw)
    for p in ref32.parameters():
        p.data.mul_(1.5)
    ref64 = theirs(D, H, batch_first=True, **kw).double()
    ref64.load_state_dict({k: v.double() for k, v in ref32.state_dict().items()})
    layer = ours(D, H, batch_first=True, **kw)
    layer.load_state_dict(ref32.state_dict())
    layer = layer.to(gpu)
    x = torch.randn(B, T, D)                               # unequal rows: their states differ from the first step on
    n_states = kw.get("num_layers", 1) * (2 if kw.get("bidirectional") else 1)
    shared = torch.randn(n_states, 1, H).expand(n_states, B, H).contiguous()
    lstm = ours is LSTM

    def state(t, dev=None):
        t = t if dev is None else t.to(dev)
        return (t, t.clone()) if lstm else t

    def ours_stepped(xd, h):
        outs = []
        for t in range(T):
            out, h = layer(xd[:, t:t + 1], h, torch.ones(B, dtype=torch.long))
            outs.append(out)
        return torch.cat(outs, dim=1), h

    with torch.no_grad():
        want, _ = _stepped(ref64, x.double(), state(shared.double()))
        want32, _ = _stepped(ref32, x, state(shared))
        got, hn = ours_stepped(x.to(gpu), state(shared, gpu))
        spec.check(name + " stepped", got, want, want32)
        hn = hn[0] if lstm else hn
        assert hn.shape == (n_states, B, H) and not bool((hn == hn[:, :1]).all())
        if not kw.get("bidirectional"):                     # .. which is one T-frame call from the shared state
            whole, _ = layer(x.to(gpu), state(shared, gpu), torch.full((B,), T, dtype=torch.long))
            spec.check(name + " stepped against one call", got, whole.double().cpu(), want32)
            spec.check(name + " one call", whole, ref64(x.double(), state(shared.double()))[0], want32)
        # a first step from states that differ per row
        own = torch.randn(n_states, B, H)
        want1, _ = ref64(x[:, :1].double(), state(own.double()))
        got1, _ = layer(x[:, :1].to(gpu), state(own, gpu), torch.ones(B, dtype=torch.long))
        spec.check(name + " own states", got1, want1, ref32(x[:, :1], state(own))[0])


def test_per_row_states_over_two_frames_or_under_grad_are_refused(gpu):
    for ours in (LSTM, GRU, RNN):
        layer = ours(D, H, batch_first=True).to(gpu)
        own = torch.randn(1, B, H, device=gpu)
        hx = (own, own.clone()) if ours is LSTM else own
        x = torch.randn(B, 2, D, device=gpu)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="Per-sequence initial states"):
            layer(x, hx, torch.full((B,), 2, dtype=torch.long))
        with pytest.raises(NotImplementedError, match="Scheduled-sampling training is the follow-up"):
            layer(x[:, :1], hx, torch.ones(B, dtype=torch.long))          # gradients enabled, parameters want them
        with torch.no_grad():
            assert layer(x[:, :1], hx, torch.ones(B, dtype=torch.long))[0].shape == (B, 1, H)
