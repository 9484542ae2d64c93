"""The configs that rebuild the models of tests/golden/decoder_fixture.npz here (the generator's, name for name), shared
by tests/test_decoder_config.py and tests/test_gpu_decoder.py."""
F, E, A, PRE, N_STEP = 3, 6, 3, 4, 5         # phoneme features, encoder width, acoustic width, pre-net width, frames a step


def encoder(enc_dec_dyn, rnn_dyn):
    LC = rnn_dyn.Config.LayerConfig
    return enc_dec_dyn.Config.ModuleConfig(
        name="Encoder", input_names=["phonemes"], output_names=["phoneme_embeddings"], process_group=0,
        config=rnn_dyn.Config(in_dim=F, batch_first=True, layer_configs=[LC("Linear", out_dim=E, nonlin="Tanh")]))


def attention_only(enc_dec_dyn):
    return enc_dec_dyn.Config.DecoderConfig(
        attention_args={enc_dec_dyn.ATTENTION_GROUND_TRUTH: "attention_matrix"},
        attention_config=enc_dec_dyn.FIXED_ATTENTION, input_names="phoneme_embeddings", name="FixedAttention",
        output_names="upsampled_phoneme_embeddings", process_group=1, n_frames_per_step=1)


def case1_config(enc_dec_dyn, rnn_dyn):
    LC = rnn_dyn.Config.LayerConfig
    return enc_dec_dyn.Config(modules=[
        encoder(enc_dec_dyn, rnn_dyn), attention_only(enc_dec_dyn),
        enc_dec_dyn.Config.ModuleConfig(
            config=rnn_dyn.Config(in_dim=E, batch_first=True, layer_configs=[
                LC("Linear", out_dim=8, nonlin="ReLU"), LC("LSTM", out_dim=4)]),
            input_names=["upsampled_phoneme_embeddings"], name="ParallelDecoder", process_group=2,
            output_names=["pred_acoustic_features"])])


def decoder(enc_dec_dyn, rnn_dyn, p_teacher_forcing, width=None, n=N_STEP):
    """the fixture's autoregressive decoder; `width`: every hidden width (the bench script's 512) instead of the
    fixture's 4 / 8 / 4"""
    LC = rnn_dyn.Config.LayerConfig
    pre, lin, rec = (PRE, 8, 4) if width is None else (width, width, width)
    enc_width = E if width is None else width
    return enc_dec_dyn.Config.DecoderConfig(
        attention_args={enc_dec_dyn.ATTENTION_GROUND_TRUTH: "attention_matrix"},
        attention_config=enc_dec_dyn.FIXED_ATTENTION, teacher_forcing_input_names=["acoustic_features"],
        config=rnn_dyn.Config(in_dim=enc_width + pre, batch_first=True, layer_configs=[
            LC("Linear", out_dim=lin, nonlin="ReLU"), LC("LSTM", out_dim=rec)]),
        input_names=["phoneme_embeddings"], name="Decoder", n_frames_per_step=n, p_teacher_forcing=p_teacher_forcing,
        pre_net_config=rnn_dyn.Config(in_dim=A, batch_first=True, layer_configs=[
            LC("Linear", out_dim=pre, nonlin="ReLU", num_layers=2)]),
        process_group=1,
        projection_configs=[enc_dec_dyn.Config.ProjectionConfig(
            config=rnn_dyn.Config(in_dim=rec, batch_first=True, layer_configs=[LC("Linear", out_dim=A * n)]),
            name="AcousticFeaturesProjector", output_names=["pred_acoustic_features"], out_dim=A,
            is_autoregressive_input=True)])


def case2_config(enc_dec_dyn, rnn_dyn, p_teacher_forcing=1.0):
    return enc_dec_dyn.Config(modules=[encoder(enc_dec_dyn, rnn_dyn), decoder(enc_dec_dyn, rnn_dyn, p_teacher_forcing)])
