"""Cuts leading and trailing silence of every given audio file down to min_silence_ms (the reference's
src/data_preparation/audio/silence_remove.py); shorter silences stay as they are, none is added.  The files are named
by an id list; results go to the output directory under the same names.

librosa.effects.trim is restated: the frame RMS comes from the kernel of csrc/audio_prep.hip
(librosa.feature.rms, center=True), the threshold scan over the few dozen values per file runs in numpy."""
import logging
import os

import numpy as np

from .... import ops
from . import audio_batch
from .AudioProcessing import AudioProcessing


def trim_indices(rms, n_samples, hop_length, top_db):
    """librosa.effects.trim's index pair from the frame RMS of a signal (ref=np.max): a frame is non-silent where
    10 log10(max(1e-10, rms^2)) minus the same of the loudest frame exceeds -top_db; (0, 0) when none is."""
    power = np.maximum(1e-10, np.square(np.asarray(rms, dtype=np.float64)))
    db = 10.0 * np.log10(power) - 10.0 * np.log10(power.max())
    nonzero = np.flatnonzero(db > -top_db)
    if nonzero.size == 0:
        return 0, 0
    start = int(nonzero[0]) * hop_length
    end = min(n_samples, (int(nonzero[-1]) + 1) * hop_length)
    return start, end


class SilenceRemover(object):
    logger = logging.getLogger(__name__)
    # the padding of librosa.feature.rms: "constant" is librosa >= 0.10, "reflect" librosa 0.8 / 0.9
    pad_mode = "constant"

    def __init__(self, min_silence_ms=200):
        self.min_silence_ms = min_silence_ms

    def keep_slice(self, file, n_samples, fs, indices):
        """(start_frame, end_frame) of raw[start_frame:end_frame] from librosa's index pair, with the reference's
        arithmetic (:81-107): the silence on either side in milliseconds, cut down to min_silence_ms or, when shorter,
        kept whole with a warning; end_frame = int(-excess * fs / 1000 - 1), so the last sample always goes."""
        silences_ms = ((indices[0] / fs * 1000, "beginning"), ((n_samples - indices[1]) / fs * 1000, "end"))
        excess_ms = []
        for silence_ms, where in silences_ms:
            if silence_ms < self.min_silence_ms:
                logging.warning("File {} has only {} ms of silence in the {}.".format(file, silence_ms, where))
                excess_ms.append(0)
            else:
                excess_ms.append(silence_ms - self.min_silence_ms)
        return int(excess_ms[0] * fs / 1000), int(-excess_ms[1] * fs / 1000 - 1)

    def trim_slices(self, samples, offsets, fs, names, silence_threshold_db=-50, hop_size_ms=None):
        """(start_frame, end_frame) for every signal of a batch at one sampling rate."""
        frame_length = AudioProcessing.fs_to_frame_length(fs)
        if hop_size_ms is None:
            hop_size_ms = min(self.min_silence_ms, 32)
        hop_length = int(fs / 1000 * hop_size_ms)
        rms, f_off = ops.frame_rms(audio_batch.to_device(samples), offsets, frame_length, hop_length, self.pad_mode)
        rms = rms.cpu().numpy()
        slices = []
        for i, name in enumerate(names):
            n = int(offsets[i + 1] - offsets[i])
            indices = trim_indices(rms[f_off[i]:f_off[i + 1]], n, hop_length, abs(silence_threshold_db))
            slices.append(self.keep_slice(name, n, fs, indices))
        return slices

    def _step(self, silence_threshold_db, hop_size_ms):
        def step(samples, offsets, fs, paths):
            slices = self.trim_slices(samples, offsets, fs, [os.path.basename(p) for p in paths],
                                      silence_threshold_db, hop_size_ms)
            return [raw[start:end] for raw, (start, end) in zip(audio_batch.split(samples, offsets), slices)]
        return step

    def process_list(self, id_list, dir_audio, dir_out, format="wav", silence_threshold_db=-50, chunk_size_ms=10):
        audio_batch.process_list([file_id + "." + format for file_id in id_list], dir_audio, dir_out,
                                 self._step(silence_threshold_db, chunk_size_ms))

    def process_file(self, file, dir_audio, dir_out, silence_threshold_db=-50, hop_size_ms=None):
        return audio_batch.process_list([file], dir_audio, dir_out, self._step(silence_threshold_db, hop_size_ms))[0]


def main():
    parser = audio_batch.list_parser(__doc__)
    parser.add_argument("--silence_db", type=int, dest="silence_threshold_db", required=False, default=-50,
                        help="frames this many dB below the loudest frame count as silence")
    parser.add_argument("--chunk_size", type=int, dest="chunk_size_ms", required=False, default=10,
                        help="hop between the frames whose level is measured, in ms")
    parser.add_argument("--min_silence_ms", type=int, dest="min_silence_ms", required=False, default=200,
                        help="silence kept in front of and behind the audio, in ms")
    audio_batch.run_command_line(parser, lambda args: SilenceRemover(args.min_silence_ms),
                                 ("silence_threshold_db", "chunk_size_ms"))


if __name__ == "__main__":
    main()
