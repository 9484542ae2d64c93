"""Reference capture for the fixed-attention decoder of enc_dec_dyn: the reference's EncDecDyn with a DecoderModule,
run on the CPU against the reference package with the stub harness of make_golden.py.  The reference's modules run in
float64 (`model.double()` works for every module used here: Linear, LSTM, the attention); parameters and inputs are
drawn in float32 first, so a float32 model can load them exactly.  Writes tests/golden/decoder_fixture.npz (data only).

Shapes: B 2, frames T (20, 15) padded to 20, phonemes P (4, 5) padded to 5, phoneme features 3, encoder width 6,
acoustic width A 3, pre-net width 4, decoder Linear 8 + LSTM 4.

  in/phonemes [B, 5, 3], in/attention_matrix [B, 20, 5] (hard, from durations; zero rows behind an utterance's frames,
  zero columns behind its phonemes), in/acoustic_features [B, 20, 3], in/frame_lens, in/phoneme_lens, in/mask [B, 20, 1]
  case1/  encoder (Linear 6, Tanh) -> DecoderConfig "FixedAttention" (n 1, no model, input_names a plain str) ->
          "ParallelDecoder" ModuleConfig (Linear 8 ReLU + LSTM 4):  sd/<key>, out/<name>, len/<name>, maxlen/<name>
  case2/  encoder -> DecoderConfig "Decoder" (n 5, pre-net 2 x Linear 4 ReLU, Linear 8 ReLU + LSTM 4, one autoregressive
          projection Linear 3 * 5, teacher forcing on acoustic_features): batched, p_teacher_forcing 1.
          sd/<key>, out/<name> ("attention" included), len/, maxlen/, mse = mean over the valid frames and the 3
          features of (pred - target)^2, grad/<key> of mse
  case3/  case 2's model and parameters through inference(): acoustic_features absent -> the iterative pass.
  case4/  the same model with p_teacher_forcing 0.5, a target, np.random.seed(1234): draws = what np.random.uniform
          returned, in order.  Run under torch.no_grad().
  quirk/  what the reference does at its edges (recorded as flags and values, see capture_quirks)
Usage: python tests/golden/make_golden_decoder.py (needs the reference checkout)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

B, T, P, F, E, A, PRE, N_STEP = 2, 20, 5, 3, 6, 3, 4, 5
FRAME_LENS, PHONEME_LENS = (20, 15), (4, 5)
DURATIONS = ((6, 3, 7, 4), (2, 5, 1, 4, 3))


class RecordUniform:
    """records what np.random.uniform returns while active"""

    def __enter__(self):
        self.orig, self.draws = np.random.uniform, []

        def uniform(*args, **kwargs):
            out = self.orig(*args, **kwargs)
            self.draws.append(out)
            return out
        np.random.uniform = uniform
        return self

    def __exit__(self, *exc):
        np.random.uniform = self.orig


def _inputs():
    import torch
    torch.manual_seed(11)
    frame_lens = torch.tensor(FRAME_LENS, dtype=torch.int64)
    attention = torch.zeros(B, T, P)
    for b, durs in enumerate(DURATIONS):
        t = 0
        for p, d in enumerate(durs):
            attention[b, t:t + d, p] = 1.0
            t += d
        assert t == FRAME_LENS[b]
    mask = (torch.arange(T)[None, :] < frame_lens[:, None]).float().unsqueeze(-1)
    pmask = (torch.arange(P)[None, :] < torch.tensor(PHONEME_LENS)[:, None]).float().unsqueeze(-1)
    phonemes = torch.randn(B, P, F) * pmask
    acoustic = (torch.randn(B, T, A) * 0.7 + 0.2) * mask
    return {"phonemes": phonemes, "attention_matrix": attention, "acoustic_features": acoustic, "mask": mask}


def _dicts(inputs, with_target):
    import torch
    names = ["phonemes", "attention_matrix"] + (["acoustic_features"] if with_target else [])
    data = {k: inputs[k].double() for k in names}
    lens = {"phonemes": torch.tensor(PHONEME_LENS), "attention_matrix": torch.tensor(FRAME_LENS),
            "acoustic_features": torch.tensor(FRAME_LENS)}
    maxs = {"phonemes": torch.tensor(P), "attention_matrix": torch.tensor(T), "acoustic_features": torch.tensor(T)}
    return data, {k: lens[k].clone() for k in names}, {k: maxs[k].clone() for k in names}


def _encoder(enc_dec_dyn, rnn_dyn):
    LC = rnn_dyn.Config.LayerConfig
    return enc_dec_dyn.Config.ModuleConfig(
        name="Encoder", input_names=["phonemes"], output_names=["phoneme_embeddings"], process_group=0,
        config=rnn_dyn.Config(in_dim=F, batch_first=True, layer_configs=[LC("Linear", out_dim=E, nonlin="Tanh")]))


def _decoder(enc_dec_dyn, rnn_dyn, p_teacher_forcing):
    LC = rnn_dyn.Config.LayerConfig
    return enc_dec_dyn.Config.DecoderConfig(
        attention_args={enc_dec_dyn.ATTENTION_GROUND_TRUTH: "attention_matrix"},
        attention_config=enc_dec_dyn.FIXED_ATTENTION, teacher_forcing_input_names=["acoustic_features"],
        config=rnn_dyn.Config(in_dim=E + PRE, batch_first=True, layer_configs=[
            LC("Linear", out_dim=8, nonlin="ReLU"), LC("LSTM", out_dim=4)]),
        input_names=["phoneme_embeddings"], name="Decoder", n_frames_per_step=N_STEP,
        p_teacher_forcing=p_teacher_forcing,
        pre_net_config=rnn_dyn.Config(in_dim=A, batch_first=True, layer_configs=[
            LC("Linear", out_dim=PRE, nonlin="ReLU", num_layers=2)]),
        process_group=1,
        projection_configs=[enc_dec_dyn.Config.ProjectionConfig(
            config=rnn_dyn.Config(in_dim=4, batch_first=True, layer_configs=[LC("Linear", out_dim=A * N_STEP)]),
            name="AcousticFeaturesProjector", output_names=["pred_acoustic_features"], out_dim=A,
            is_autoregressive_input=True)])


def _record(out, prefix, data, lens, maxs, given):
    for k, v in data.items():
        if k not in given:
            out[prefix + "out/" + k] = v.detach().numpy()
    for k, v in lens.items():
        if k not in given:
            out[prefix + "len/" + k] = np.asarray(v)
    for k, v in maxs.items():
        if k not in given:
            out[prefix + "maxlen/" + k] = np.asarray(v)


def _new_model(config, seed):
    import torch
    torch.manual_seed(seed)
    model = config.create_model()
    for p in model.parameters():            # away from the small default initialisation
        p.data.mul_(2.0)
    return model.double()


def capture(out):
    import torch
    from idiaptts.src.neural_networks.pytorch.models import enc_dec_dyn, rnn_dyn
    LC = rnn_dyn.Config.LayerConfig
    inputs = _inputs()
    for k, v in inputs.items():
        out["in/" + k] = v.numpy()
    out["in/frame_lens"], out["in/phoneme_lens"] = np.asarray(FRAME_LENS), np.asarray(PHONEME_LENS)

    # case 1: attention only, feeding a parallel decoder
    config = enc_dec_dyn.Config(modules=[
        _encoder(enc_dec_dyn, rnn_dyn),
        enc_dec_dyn.Config.DecoderConfig(
            attention_args={enc_dec_dyn.ATTENTION_GROUND_TRUTH: "attention_matrix"},
            attention_config=enc_dec_dyn.FIXED_ATTENTION, input_names="phoneme_embeddings", name="FixedAttention",
            output_names="upsampled_phoneme_embeddings", process_group=1, n_frames_per_step=1),
        enc_dec_dyn.Config.ModuleConfig(
            config=rnn_dyn.Config(in_dim=E, batch_first=True, layer_configs=[
                LC("Linear", out_dim=8, nonlin="ReLU"), LC("LSTM", out_dim=4)]),
            input_names=["upsampled_phoneme_embeddings"], name="ParallelDecoder", process_group=2,
            output_names=["pred_acoustic_features"])])
    model = _new_model(config, 21)
    for k, v in model.state_dict().items():
        out["case1/sd/" + k] = np.array(v.numpy(), copy=True)
    data, lens, maxs = _dicts(inputs, False)
    given = set(data)
    model.init_hidden(B)
    with torch.no_grad():
        model(data, lens, maxs)
    _record(out, "case1/", data, lens, maxs, given)
    print("case1 keys", list(model.state_dict()), "outputs", [k for k in data if k not in given])

    # case 2: the autoregressive decoder, batched under teacher forcing
    model = _new_model(enc_dec_dyn.Config(modules=[_encoder(enc_dec_dyn, rnn_dyn),
                                                   _decoder(enc_dec_dyn, rnn_dyn, 1.0)]), 22)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k, v in sd.items():
        out["case2/sd/" + k] = np.array(v.numpy(), copy=True)
    out["case2/param_names"] = np.asarray([k for k, _ in model.named_parameters()])
    data, lens, maxs = _dicts(inputs, True)
    given = set(data)
    model.init_hidden(B)
    model(data, lens, maxs)
    _record(out, "case2/", data, lens, maxs, given)
    mask = inputs["mask"].double()
    mse = (((data["pred_acoustic_features"] - data["acoustic_features"]) ** 2) * mask).sum() / (mask.sum() * A)
    out["case2/mse"] = np.asarray(float(mse))
    mse.backward()
    for k, v in model.named_parameters():
        out["case2/grad/" + k] = v.grad.numpy()
    print("case2 keys", list(sd), "mse", float(mse), "lens", {k: v for k, v in lens.items() if k not in given})

    # case 3: inference() without the teacher-forcing input
    data, lens, maxs = _dicts(inputs, False)
    given = set(data)
    model.init_hidden(B)
    with torch.no_grad(), RecordUniform() as rec:
        model.inference(data, lens, maxs)
    assert len(rec.draws) == 0
    _record(out, "case3/", data, lens, maxs, given)
    print("case3 outputs", {k: tuple(v.shape) for k, v in data.items() if k not in given})

    # case 4: the iterative pass with a target and p_teacher_forcing 0.5
    model4 = _new_model(enc_dec_dyn.Config(modules=[_encoder(enc_dec_dyn, rnn_dyn),
                                                    _decoder(enc_dec_dyn, rnn_dyn, 0.5)]), 22)
    model4.load_state_dict(sd)
    data, lens, maxs = _dicts(inputs, True)
    given = set(data)
    model4.init_hidden(B)
    np.random.seed(1234)
    with torch.no_grad(), RecordUniform() as rec:
        model4(data, lens, maxs)
    out["case4/draws"] = np.asarray(rec.draws, dtype=np.float64)
    _record(out, "case4/", data, lens, maxs, given)
    print("case4 draws", rec.draws, "lens", {k: v for k, v in lens.items() if k not in given},
          "maxs", {k: v for k, v in maxs.items() if k not in given})
    capture_quirks(out, inputs)


def capture_quirks(out, inputs):
    """The reference at its edges.
    quirk/str_input_names: DecoderConfig(input_names="phoneme_embeddings") -> the module's input_names.
    quirk/partial/: FixedAttention.forward_incremental on T = 7, n = 5 at idx 5 (a slice of 2 rows: their mean) and at
    idx 10 (an empty slice: NaN weights and context)."""
    import torch
    from idiaptts.src.neural_networks.pytorch.models import enc_dec_dyn
    config = enc_dec_dyn.Config.DecoderConfig(
        attention_args={enc_dec_dyn.ATTENTION_GROUND_TRUTH: "attention_matrix"},
        attention_config=enc_dec_dyn.FIXED_ATTENTION, input_names="phoneme_embeddings", name="FixedAttention",
        output_names="upsampled", n_frames_per_step=1)
    out["quirk/str_input_names"] = np.asarray(list(config.create_model().input_names))
    attention = enc_dec_dyn.FixedAttention.Config("attention_matrix", 5).create_model()
    A_ = inputs["attention_matrix"][:, :7].double()
    enc = torch.arange(B * P * 2, dtype=torch.float64).reshape(B, P, 2) / 7.0
    c5, w5, _ = attention.forward_incremental(5, enc, None, A_)
    c10, w10, _ = attention.forward_incremental(10, enc, None, A_)
    out["quirk/partial/A"], out["quirk/partial/enc"] = A_.numpy(), enc.numpy()
    out["quirk/partial/ctx5"], out["quirk/partial/w5"] = c5.numpy(), w5.numpy()
    out["quirk/partial/empty_is_nan"] = np.asarray(bool(torch.isnan(w10).all() and torch.isnan(c10).all()))
    print("quirks: input_names", out["quirk/str_input_names"], "empty slice NaN", out["quirk/partial/empty_is_nan"])


def _main():
    mg.install_stub_harness()
    out = {}
    capture(out)
    path = os.path.join(HERE, "decoder_fixture.npz")
    np.savez_compressed(path, **out)
    print("decoder_fixture.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    _main()
