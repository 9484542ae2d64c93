"""WaveNetVocoderTrainer: trains the sample-level vocoder (WaveNetWrapper) from spectral conditioning at the frame
rate to raw audio, with the reference's names and defaults (idiaptts/src/model_trainers/WaveNetVocoderTrainer.py:
__init__ :45-92, legacy_support_init :124-177, create_hparams :179-243).

The reference's class is not a working recipe -- it reads hparams.max_input_train_sec, which nothing defines, assigns
dataset_val twice (:111, :119) and never the training set, calls ModelTrainer.split_batch (:276), which does not exist,
and matches the conditioning's length to a "questions" reader it does not have -- so where it is broken this class
decides:
  * max_input_train_sec = 0.5, max_input_test_sec = 1.0 and num_mixtures = 10 are defaults here; a window has
    W = int(1000 / frame_size_ms * sec) * m samples, m = int(frame_rate_output_Hz / (1000 / frame_size_ms));
  * the corpus lives on the device (data_preparation/VocoderCorpus.py) and one kernel launch assembles a batch of
    windows, conditioning up-sampled in the same launch: the "mfbanks" reader has no preprocessing_fn and no
    match_length, and there is no collate / decollate function;
  * the silence trim cuts samples and conditioning together (VocoderCorpus);
  * the mask handed to the loss is the sequence mask without its first column (prepare_batch :263-264), and its
    lengths count the scored columns, len - 1;
  * synth generates whole utterances in batches (the reference's wrapper refuses batches), seeded by hparams.seed;
  * train / test / checkpoints are ModularTrainer's; figures, save_for_vocoding (a pickle of the whole model),
    upsample_conditional_features, other dataset types and more than one rank are refused or not built."""
import copy
import logging
import os
from typing import List

import numpy as np

from idiaptts_amd.src.data_preparation.audio.RawWaveformLabelGen import RawWaveformLabelGen
from idiaptts_amd.src.data_preparation.DataReaderConfig import DataReaderConfig
from idiaptts_amd.src.data_preparation.VocoderCorpus import (VocoderCorpus, VocoderWindowSampler,
                                                             in_to_out_multiplier, window_length)
from idiaptts_amd.src.ExtendedHParams import ExtendedHParams
from idiaptts_amd.src.model_trainers.ModularTrainer import ModularTrainer
from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
from idiaptts_amd.src.neural_networks.pytorch.models.WaveNetWrapper import WaveNetWrapper
from idiaptts_amd.src.Synthesiser import Synthesiser


class WaveNetVocoderTrainer(ModularTrainer):
    logger = logging.getLogger(__name__)

    def __init__(self, hparams: ExtendedHParams, id_list: List[str],
                 data_reader_configs: List[DataReaderConfig] = None):
        if hparams is None:
            hparams = self.create_hparams()
            hparams.out_dir = os.path.curdir
        self._refuse(hparams)
        super().__init__(data_reader_configs=data_reader_configs, id_list=id_list, hparams=hparams)
        if hparams.scheduler_type == "default":
            hparams.scheduler_type = "Noam"
            hparams.scheduler_args['wormup_steps'] = 4000       # (the reference's spelling; the handler reads it)
        self.corpus = None
        self._prepared_readers = None

    @staticmethod
    def _refuse(hparams):
        if hparams.has_value("upsample_conditional_features") and hparams.upsample_conditional_features:
            raise NotImplementedError("upsample_conditional_features = {} is not implemented: the conditioning is "
                                      "up-sampled linearly while a batch is assembled."
                                      .format(hparams.upsample_conditional_features))
        if hparams.dataset_type != "PyTorchDatareadersDataset":
            raise NotImplementedError("dataset_type = {} is not implemented: the vocoder trains from its "
                                      "device-resident corpus.".format(hparams.dataset_type))
        from idiaptts_amd import parallel
        world = parallel.dp_rank_world()[1]
        if world > 1:
            raise NotImplementedError("torch.distributed with {} ranks is not implemented for the vocoder: its window "
                                      "sampler is single-process.".format(world))

    @staticmethod
    def legacy_support_init(dir_world_features: os.PathLike, id_list: List[str], hparams: ExtendedHParams):
        mu = hparams.mu if hparams.input_type == WaveNetWrapper.Config.INPUT_TYPE_MULAW else None
        data_reader_configs = [
            DataReaderConfig(
                name="mfbanks",
                directory=dir_world_features,
                feature_type="WorldFeatLabelGen",
                features=[hparams.sp_type + str(hparams.num_coded_sps)],
                output_names=["conditioning"],
                requires_seq_mask=True,
                random_select=True,
                load_sp=hparams.load_sp,
                load_lf0=hparams.load_lf0,
                load_vuv=hparams.load_vuv,
                load_bap=hparams.load_bap,
                add_deltas=False,
                num_coded_sps=hparams.num_coded_sps,
                num_bap=hparams.num_bap,
                sp_type=hparams.sp_type,
            ),
            DataReaderConfig(
                name="target",
                feature_type="RawWaveformLabelGen",
                directory=hparams.data_dir,
                frame_rate_output_Hz=hparams.frame_rate_output_Hz,
                frame_size_ms=hparams.frame_size_ms,
                mu=mu,
                silence_threshold_quantized=hparams.silence_threshold_quantized,
                requires_seq_mask=True,
            ),
        ]
        return dict(data_reader_configs=data_reader_configs, hparams=hparams, id_list=id_list)

    @staticmethod
    def create_hparams(hparams_string=None, verbose=False):
        """Create model hyper-parameters. Parse non-default from given string."""
        hparams = ModularTrainer.create_hparams(hparams_string, verbose=False)
        hparams.synth_vocoder = "raw"
        hparams.add_hparams(
            batch_first=True,
            frame_rate_output_Hz=16000,
            bit_depth=16,
            silence_threshold_quantized=None,  # Beginning and end of audio below the threshold are trimmed.
            teacher_forcing_in_test=True,
            ema_decay=0.9999,
            mu=255,
            input_type=WaveNetWrapper.Config.INPUT_TYPE_MULAW,
            use_cond=True,  # Determines if conditioning is used.
            len_in_out_multiplier=1,
            sp_type="mfbanks",
            load_sp=True,
            load_lf0=False,
            load_vuv=False,
            load_bap=False,
            # read by the reference, defined nowhere in it:
            max_input_train_sec=0.5,
            max_input_test_sec=1.0,
            num_mixtures=10)
        if hparams_string:           # (the string wins over this class's defaults as well)
            hparams.parse(hparams_string)
        if verbose:
            logging.info(hparams.get_debug_string())
        return hparams

    # ------------------------------------------------------------------------------ data
    @staticmethod
    def window_lengths(hparams):
        """(W_train, W_test) in samples"""
        m = in_to_out_multiplier(hparams.frame_rate_output_Hz, hparams.frame_size_ms)
        return (window_length(hparams.max_input_train_sec, hparams.frame_size_ms, m),
                window_length(hparams.max_input_test_sec, hparams.frame_size_ms, m))

    def _setup_datareaders(self, data_reader_configs, hparams):
        if self._prepared_readers is not None:           # init() has set them up for its defaults
            self.datareaders.update(self._prepared_readers)
            self._prepared_readers = None
            return
        self._refuse(hparams)
        readers = [config.create_reader() for config in data_reader_configs]
        for reader in readers:
            for out_name in reader.output_names:
                self.datareaders[out_name] = reader
        self._readers = readers
        wave = [r for r in readers if isinstance(r, RawWaveformLabelGen)]
        cond = [r for r in readers if r not in wave]
        if len(wave) != 1 or len(cond) > 1 or (hparams.use_cond and len(cond) != 1):
            raise ValueError("The vocoder takes one RawWaveformLabelGen and one conditioning reader, got {}.".format(
                [type(r).__name__ for r in readers]))
        self.wave_reader, self.cond_reader = wave[0], (cond[0] if hparams.use_cond else None)
        W_train, W_test = self.window_lengths(hparams)
        splits = [("train", self.id_list_train), ("val", self.id_list_val), ("test", self.id_list_test)]
        for name, ids in splits[1:]:
            overlap = [i for i in (ids or []) if i in self.id_list_train]
            assert len(overlap) == 0, "Found same ids in train and {} set: ".format(name) + ", ".join(overlap)
        all_ids = [i for _, ids in splits for i in (ids or [])]
        self.corpus = VocoderCorpus(self.wave_reader, self.cond_reader, all_ids)
        index = {id_name: n for n, id_name in enumerate(all_ids)}

        def sampler(ids, W, training):
            if ids is None:
                return None
            return VocoderWindowSampler(self.corpus, [index[i] for i in ids], W, seed=hparams.seed, training=training)
        self.dataset_train = sampler(self.id_list_train, W_train, True)
        self.dataset_val = sampler(self.id_list_val, W_test, False)
        self.dataset_test = sampler(self.id_list_test, W_test, False)

    # ------------------------------------------------------------------------------ init
    def init(self, hparams, model_config=None, loss_configs=None, data_reader_configs=None):
        self._refuse(hparams)
        if model_config is None or loss_configs is None:
            # the defaults need the conditioning's width, which the corpus knows: the readers come first, and
            # ModularTrainer.init finds them ready
            configs = data_reader_configs if data_reader_configs is not None else self._data_reader_configs
            if configs is None:
                raise ValueError("Parameter data_reader_configs is required.")
            self.datareaders = dict()
            self._setup_datareaders(copy.deepcopy(configs), hparams)
            self._prepared_readers = dict(self.datareaders)
            wavenet_config = self.default_wavenet_config(hparams, self.corpus.cin)
            if model_config is None:
                model_config = WaveNetWrapper.NamedConfig(wavenet_config, input_names=["conditioning"],
                                                          target_name="target", output_names=["pred_target"],
                                                          name="WaveNetVocoder", batch_first=True)
            if loss_configs is None:
                loss_configs = [self.default_loss_config(hparams, getattr(model_config, "wavenet_config",
                                                                          wavenet_config))]
        super().init(hparams, model_config=model_config, loss_configs=loss_configs,
                     data_reader_configs=data_reader_configs)

    @staticmethod
    def default_wavenet_config(hparams, cin_channels):
        if hparams.input_type == WaveNetWrapper.Config.INPUT_TYPE_MULAW:
            return WaveNetWrapper.Config(cin_channels=cin_channels, out_channels=hparams.mu + 1, scalar_input=False)
        if hparams.input_type == WaveNetWrapper.Config.INPUT_TYPE_RAW:
            return WaveNetWrapper.Config(cin_channels=cin_channels, out_channels=3 * hparams.num_mixtures,
                                         scalar_input=True)
        raise NotImplementedError("input_type = {} is not implemented ({}, {}).".format(
            hparams.input_type, WaveNetWrapper.Config.INPUT_TYPE_MULAW, WaveNetWrapper.Config.INPUT_TYPE_RAW))

    @staticmethod
    def default_loss_config(hparams, wavenet_config, pred_name="pred_target", target_name="target"):
        common = dict(input_names=[pred_name, target_name], seq_mask=target_name + "_mask", batch_first=True,
                      reduction="mean_per_frame", shift=1)
        if hparams.input_type == WaveNetWrapper.Config.INPUT_TYPE_MULAW:
            return NamedLoss.Config(name="OneHotCrossEntropyLoss", type_="OneHotCrossEntropyLoss", **common)
        return NamedLoss.Config(name="DiscretizedMixturelogisticLoss", type_="DiscretizedMixturelogisticLoss",
                                num_classes=2 ** hparams.bit_depth, log_scale_min=wavenet_config.log_scale_min,
                                hinge_loss=wavenet_config.hinge_regularizer, **common)

    def train(self, hparams):
        # (the sampler's epoch follows the trainer's: a run continued from a checkpoint draws the next epoch's windows)
        self.dataset_train.epoch = self.total_epoch
        return super().train(hparams)

    # ------------------------------------------------------------------------------ synthesis
    @staticmethod
    def draw_uniforms(generator, n_rows, n_samples, scalar_input, device):
        """the numbers WaveNet.generate draws with, from `generator`: [B, T] for classes, [B, T, 2] in (1e-5,
        1 - 1e-5) for the mixture of logistics (choice, logistic)"""
        import torch
        shape = (n_rows, n_samples, 2) if scalar_input else (n_rows, n_samples)
        u = torch.rand(shape, generator=generator, device=device, dtype=torch.float32)
        return u * (1.0 - 2e-5) + 1e-5 if scalar_input else u

    def synth(self, hparams, ids_input, post_processing_mapping=None, plotter_configs=None, load_target=True):
        """One wav per id through Synthesiser.run_raw_synth: the conditioning from the reader, up-sampled with
        sample_linearly_batch, T * m samples generated in batches of hparams.batch_size_synth.  With hparams.seed the
        uniforms come from a generator seeded with it (one generator over the batches, in the order of the ids), so
        two calls write the same bytes.  Returns {id: waveform float64}."""
        import torch
        from idiaptts_amd.misc.utils import sample_linearly_batch
        if hparams.synth_gen_figure:
            raise NotImplementedError("Figure generation is outside the accelerated path.")
        id_list = self._input_to_str_list(ids_input)
        self.logger.info("Start synthesising [{0}]".format(", ".join(str(i) for i in id_list)))
        model = self.model_handler.model
        model.eval()
        wrapper = model.model
        device = next(model.parameters()).device
        m = in_to_out_multiplier(hparams.frame_rate_output_Hz, hparams.frame_size_ms)
        generator = None
        if hparams.seed is not None:
            generator = torch.Generator(device=device)
            generator.manual_seed(int(hparams.seed))
        scalar_input = wrapper.model.scalar_input
        output = {}
        for first in range(0, len(id_list), hparams.batch_size_synth):
            ids = id_list[first:first + hparams.batch_size_synth]
            cond, frames = None, None
            if model.use_cond:
                feats = [np.asarray(self.cond_reader[i][self.cond_reader.output_names[0]], dtype=np.float32)
                         for i in ids]
                frames = [len(f) for f in feats]
                up = sample_linearly_batch(feats, m)                               # device tensors [T m, cin]
                cond = torch.nn.utils.rnn.pad_sequence(up, batch_first=True).transpose(1, 2).contiguous()
            else:
                frames = [len(self.wave_reader.load(i)) // m for i in ids]
            lengths = [T * m for T in frames]
            uniforms = self.draw_uniforms(generator, len(ids), max(lengths), scalar_input, device)
            waves = wrapper.generate_waveform(cond, lengths, uniforms=uniforms)
            for id_name, wave in zip(ids, waves):
                output[id_name] = wave.cpu().numpy()
        Synthesiser.run_raw_synth(output, hparams, epoch=self.total_epoch, step=self.total_steps)
        return output

    def gen_figure_from_output(self, id_name, labels, hidden, hparams):
        raise NotImplementedError("gen_figure_from_output: figure generation is outside the accelerated path.")
