"""Synthesiser.run_world_synth, run_griffin_lim and run_raw_synth with the reference's interface
(idiaptts/src/Synthesiser.py:38-106, :155-179, :320-351).

The reference walks the utterances one by one (decode_sp -> world_features_to_raw -> write);
here all utterances of the call are decoded (mgc2sp, or the mel inversion kernel for sp_type "mfbanks"),
aperiodicity-decoded and synthesised by single batched GPU launches, then written. `synth_world_features` is the name BASELINE.json's
north-star uses for this entry point; it is provided as an alias.
"""
import logging
import math
import os
from typing import Dict

import numpy as np
import scipy.io.wavfile

from .. import world as _world
from .data_preparation.audio.AudioProcessing import AudioProcessing
from .data_preparation.audio.audio_batch import write_pcm16
from .data_preparation.world.WorldFeatLabelGen import WorldFeatLabelGen


def _has(hparams, name):
    if hasattr(hparams, "has_value"):
        return hparams.has_value(name)
    return getattr(hparams, name, None) is not None


def _get(hparams, name, default):
    return getattr(hparams, name) if _has(hparams, name) else default


class Synthesiser(object):
    SYNTH_SUB_DIR = "synth"
    # Amplitude floor of spectra decoded from mel filter banks before WORLD synthesis: the NNLS inversion leaves
    # bins at exactly 0, where WORLD's aperiodic response takes log(0) and the waveform turns NaN (the reference
    # passes them on unchanged).  1e-6 is WORLD's own safe-guard minimum of the power spectrum, 1e-12, as an
    # amplitude.
    MFBANKS_AMP_FLOOR = 1e-6

    @staticmethod
    def run_world_synth(synth_output: Dict[str, np.ndarray], hparams, epoch: int = None,
                        step: int = None, use_model_name: bool = True,
                        has_deltas: bool = False, return_waveforms: bool = False):
        """Run the WORLD synthesize method on every entry of synth_output (id -> features).  sp_type "mfbanks":
        the mel filter banks of all utterances are inverted in one launch (AudioProcessing.mfbanks_to_amp_sp_batch)
        and floored at MFBANKS_AMP_FLOOR, a departure from the reference that keeps the waveforms finite."""
        fs = hparams.synth_fs
        fft_size = AudioProcessing.fs_to_frame_length(fs)
        save_dir = Synthesiser._get_synth_dir(hparams, use_model_name, epoch=epoch, step=step)
        ids, amp_sps, lf0s, vuvs, baps = [], [], [], [], []
        post_filtering = getattr(hparams, "do_post_filtering", False)
        mfbanks = []
        for id_name, output in synth_output.items():
            coded_sp, lf0, vuv, bap = WorldFeatLabelGen.convert_to_world_features(
                output, contains_deltas=has_deltas, num_coded_sps=hparams.num_coded_sps,
                num_bap=hparams.num_bap)
            if hparams.sp_type == "mfbanks":
                mfbanks.append(coded_sp)    # decoded below, all utterances in one launch
                amp_sp = None
            else:
                amp_sp = AudioProcessing.decode_sp(coded_sp, hparams.sp_type, fs,
                                                   post_filtering=post_filtering).astype(np.double, copy=False)
            ids.append(id_name)
            amp_sps.append(amp_sp)
            lf0s.append(lf0)
            vuvs.append(vuv)
            baps.append(bap)
        if mfbanks:
            if post_filtering:
                logging.warning("Post-filtering only implemented for cepstrum features.")
            amp_sps = [np.maximum(a.astype(np.double, copy=False), Synthesiser.MFBANKS_AMP_FLOOR)
                       for a in AudioProcessing.mfbanks_to_amp_sp_batch(mfbanks, fs)]
        args = dict()
        for attr in "preemphasis", "f0_silence_threshold", "lf0_zero":
            if hasattr(hparams, attr):
                args[attr] = getattr(hparams, attr)
        waveforms = WorldFeatLabelGen.world_features_to_raw_batch(amp_sps, lf0s, vuvs, baps, fs=fs,
                                                                  n_fft=fft_size, **args)
        for id_name, waveform in zip(ids, waveforms):
            logging.info("Synthesise {} with the WORLD vocoder.".format(id_name))
            file_name = (os.path.basename(id_name) + getattr(hparams, "synth_file_suffix", "")
                         + '_' + str(hparams.num_coded_sps) + hparams.sp_type + "_WORLD")
            file_path = os.path.join(save_dir, file_name)
            # soundfile.write(float) default subtype for .wav is PCM_16
            write_pcm16(file_path + ".wav", waveform, fs)
            if getattr(hparams, "synth_ext", "wav").lower() != 'wav':
                raise NotImplementedError("Only wav output is supported (pydub is out of scope).")
        if return_waveforms:
            return dict(zip(ids, waveforms))

    synth_world_features = run_world_synth

    @staticmethod
    def run_griffin_lim_on_log(synth_output: Dict[str, np.ndarray], *args, **kwargs):
        """reference :320-322: Griffin-Lim of dB amplitude spectra (db_to_amp first)."""
        synth_output = {k: AudioProcessing.db_to_amp(v) for k, v in synth_output.items()}
        return Synthesiser.run_griffin_lim(synth_output, *args, **kwargs)

    @staticmethod
    def run_griffin_lim(synth_output: Dict[str, np.ndarray], hparams, epoch: int = None, step: int = None,
                        use_model_name: bool = True, return_waveforms: bool = False):
        """Griffin-Lim of every amplitude spectrum [T, K] in synth_output (id -> spectrum), written to
        <basename>[_<model_name>]<synth_file_suffix>.<synth_ext> (reference :324-351).  The reference runs
        librosa.griffinlim(output.T ** griffin_lim_power, n_iter=griffin_lim_iters, hop_length, win_length) per
        utterance; here all utterances of the call run as one batch on the Griffin-Lim kernel (the random initial
        phases are drawn from np.random in the same order).  Samples are written as raw_to_file does -- times
        2 ** (bit_depth - 1), truncated to int16 -- but clipped to the int16 range first, where the reference's
        cast is undefined.  Only wav output is supported."""
        if getattr(hparams, "synth_ext", "wav").lower() != "wav":
            raise NotImplementedError("Only wav output is supported (pydub is out of scope).")
        fs = hparams.synth_fs
        hop_length = int(hparams.hop_size_ms / 1000. * fs)
        win_length_ms = getattr(hparams, "win_length_ms", None)
        win_length = None if win_length_ms is None else int(win_length_ms / 1000. * fs)
        power = _get(hparams, "griffin_lim_power", 1.2)
        ids = list(synth_output.keys())
        spectra = [np.asarray(synth_output[i]) ** power for i in ids]
        waveforms = _world.griffinlim_batch(spectra, n_iter=_get(hparams, "griffin_lim_iters", 60),
                                            hop_length=hop_length, win_length=win_length)
        preemphasis = _get(hparams, "preemphasis", 0.0)
        if preemphasis != 0:
            waveforms = [AudioProcessing.depreemphasis(raw, preemphasis) for raw in waveforms]
        save_dir = Synthesiser._get_synth_dir(hparams, use_model_name, epoch=epoch, step=step)
        bit_depth = _get(hparams, "bit_depth", 16)
        for id_name, raw in zip(ids, waveforms):
            file_name = "{}{}{}.{}".format(os.path.basename(id_name).rsplit('.', 1)[0],
                                           "_" + hparams.model_name if use_model_name else "",
                                           getattr(hparams, "synth_file_suffix", ""), hparams.synth_ext)
            Synthesiser.raw_to_file(os.path.join(save_dir, file_name), raw, fs, bit_depth)
        if return_waveforms:
            return dict(zip(ids, waveforms))

    @staticmethod
    def copy_synth(hparams, file_id_list, epoch=None, step=None, feature_dir=None):
        """Reference audio of synth_vocoder "raw" (reference :155-165): every file of file_id_list (paths of wav
        files) is loaded with RawWaveformLabelGen.load_sample(id_name, hparams.frame_rate_output_Hz) and written
        back with the suffix "_ref", without the model name; the suffix of hparams is restored afterwards.  The other
        vocoders copy-synthesise from a trainer's data readers (ModularTrainer.copy_synth)."""
        if hparams.synth_vocoder != "raw":
            raise NotImplementedError("Synthesiser.copy_synth is implemented for synth_vocoder \"raw\", not {}: use "
                                      "the trainer's copy_synth.".format(hparams.synth_vocoder))
        from .data_preparation.audio.RawWaveformLabelGen import RawWaveformLabelGen
        logging.info("Copy synthesis with {} for [{}].".format(hparams.synth_vocoder, ", ".join(file_id_list)))
        synth_dict = {id_name: RawWaveformLabelGen.load_sample(id_name, _get(hparams, "frame_rate_output_Hz", None))
                      for id_name in file_id_list}
        old_synth_file_suffix = getattr(hparams, "synth_file_suffix", "")
        hparams.synth_file_suffix = "_ref"
        try:
            Synthesiser.run_raw_synth(synth_dict, hparams, epoch=epoch, step=step, use_model_name=False)
        finally:
            hparams.synth_file_suffix = old_synth_file_suffix

    @staticmethod
    def raw_file_name(id_name, hparams, use_model_name=True):
        """<basename>[_<model_name>]<synth_file_suffix>.<synth_ext>"""
        return "{}{}{}.{}".format(os.path.basename(id_name).rsplit('.', 1)[0],
                                  "_" + hparams.model_name if use_model_name else "",
                                  getattr(hparams, "synth_file_suffix", ""), hparams.synth_ext)

    @staticmethod
    def run_raw_synth(synth_output: Dict[str, np.ndarray], hparams, epoch: int = None, step: int = None,
                      use_model_name: bool = True):
        """Write the raw waveforms in synth_output (id -> samples in [-1, 1]) with raw_to_file (reference :167-179),
        to <basename>[_<model_name>]<synth_file_suffix>.<synth_ext>.  That is the name the reference intends: its
        expression at :174-177 has a precedence slip (the conditional swallows everything after "_" + model_name, so
        with use_model_name the suffix is lost and without it the basename is) and a stray comma that makes the name
        a tuple, which os.path.join refuses.  Only wav output is supported."""
        if getattr(hparams, "synth_ext", "wav").lower() != "wav":
            raise NotImplementedError("Only wav output is supported (pydub is out of scope).")
        save_dir = Synthesiser._get_synth_dir(hparams, use_model_name, epoch=epoch, step=step)
        bit_depth = _get(hparams, "bit_depth", 16)
        for id_name, raw in synth_output.items():
            file_name = Synthesiser.raw_file_name(id_name, hparams, use_model_name)
            Synthesiser.raw_to_file(os.path.join(save_dir, file_name), np.asarray(raw).reshape(-1), hparams.synth_fs,
                                    bit_depth)

    @staticmethod
    def raw_to_file(file_path, raw, fs, bit_depth=16):
        """reference :181-201 for wav: raw * 2 ** (bit_depth - 1) truncated to int16 (clipped to its range first)."""
        logging.info("Save {} from raw waveform.".format(file_path))
        pcm = np.clip(np.asarray(raw) * math.pow(2, bit_depth - 1), -32768, 32767).astype(np.int16)
        scipy.io.wavfile.write(file_path, fs, pcm)

    @staticmethod
    def _get_synth_dir(hparams, use_model_name: bool = True, epoch: int = None, step: int = None):
        """reference :82-106"""
        if _has(hparams, "synth_dir"):
            save_dir = hparams.synth_dir
        else:
            parts = [hparams.out_dir] if _has(hparams, "out_dir") else [os.path.curdir]
            if use_model_name and _has(hparams, "model_name"):
                parts.append(hparams.model_name)
            parts.append(Synthesiser.SYNTH_SUB_DIR)
            if epoch is not None:
                parts.append("e" + str(epoch))
            elif step is not None:
                parts.append("s" + str(step))
            save_dir = os.path.join(*parts)
        os.makedirs(save_dir, exist_ok=True)
        logging.info("Selected {} as synthesis directory.".format(save_dir))
        return save_dir
