"""Raw waveforms from .wav files as network targets, with the reference's constructor and methods
(data_preparation/audio/RawWaveformLabelGen.py): samples in [-1, 1), mu-law companded to mu + 1 classes and returned
as the [T, mu + 1] one-hot target OneHotCrossEntropyLoss consumes, or as [T, 1] float32 for
DiscretizedMixturelogisticLoss when mu is None.

The companding runs on the device in float64 (itts_mulaw_encode_f64 / itts_mulaw_decode, csrc/mol.hip);
`preprocess_batch` writes the one-hot targets of a whole list from one launch (itts_mulaw_onehot) and leaves them
there: the one-hot array, 256 to 65536 floats a sample, is never built on the host.  Files are read through
AudioProcessing.read_wav (the reference reads with pydub); changing the frame rate while loading is refused, because
pydub's audioop resampler is not reproduced here: resample the corpus first with down_sampling.downsample_list.
The reference's command line (a debugging print of three samples) is not built."""
import logging
import os

import numpy as np

from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
from idiaptts_amd.src.data_preparation.DataReaders import ReaderBase


def _device():
    import torch
    from idiaptts_amd import lib
    lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


class RawWaveformLabelGen(ReaderBase):
    """Load raw waveform from .wav files."""

    logger = logging.getLogger(__name__)

    def __init__(self, dir_labels=None, norm_params=None, frame_rate_output_Hz=None, frame_size_ms=5, mu=None,
                 silence_threshold_quantized=None):
        self.dir_labels = dir_labels
        self.frame_rate_output_Hz = frame_rate_output_Hz
        self.frame_size_ms = frame_size_ms
        self.mu = mu
        self.silence_threshold_quantized = silence_threshold_quantized
        self.norm_params = norm_params
        self._configure("raw")

    def _file_path(self, file_path):
        candidates = [file_path, file_path + ".wav"]
        if self.dir_labels is not None:
            candidates += [os.path.join(self.dir_labels, file_path), os.path.join(self.dir_labels, file_path + ".wav")]
        for path in candidates:
            if os.path.isfile(path):
                return path
        raise FileNotFoundError("Cannot find file {}.".format(" or ".join(candidates)))

    def load(self, file_path):
        return self.load_sample(self._file_path(file_path), self.frame_rate_output_Hz)

    @staticmethod
    def trim_end_sample(sample, length, reverse=False):
        """Trim the end (with reverse the front) of a preprocessed sample by `length` frames."""
        if length == 0:
            return sample
        return sample[length:, ...] if reverse else sample[:-length, ...]

    @staticmethod
    def load_sample(file_path, frame_rate_output_Hz=None):
        """The file's samples as float64 in [-1, 1): integers divided by 2 ** (bit_depth - 1), as the reference."""
        raw, fs = AudioProcessing.read_wav(file_path)
        if raw.ndim != 1:
            raise ValueError("{} has {} channels: RawWaveformLabelGen takes mono files.".format(file_path,
                                                                                              raw.shape[1]))
        if frame_rate_output_Hz is not None and frame_rate_output_Hz != fs:
            raise NotImplementedError(
                "{} has a frame rate of {} Hz and frame_rate_output_Hz is {} Hz: changing the rate while loading is "
                "not implemented (pydub's resampler is not reproduced); resample the files first with "
                "down_sampling.downsample_list.".format(file_path, fs, frame_rate_output_Hz))
        return raw

    @staticmethod
    def mu_law_companding(raw, mu=255):
        """int64 class indices in [0, mu]: ((sign(x) log(1 + mu |x|) / log(1 + mu)) + 1) mu / 2, truncated."""
        import torch
        from idiaptts_amd import ops
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        x = torch.from_numpy(raw.reshape(-1)).to(_device())
        return ops.mulaw_encode(x, [0, x.numel()], mu).cpu().numpy().reshape(raw.shape)

    @staticmethod
    def mu_law_companding_reversed(raw, mu=255):
        """float64 samples of class indices: r = i / (mu / 2) - 1, sign(r) / mu ((1 + mu) ** |r| - 1)."""
        import torch
        from idiaptts_amd import ops
        raw = np.ascontiguousarray(raw)
        if not np.issubdtype(raw.dtype, np.integer):
            raise TypeError("mu_law_companding_reversed takes class indices (integers), got {}.".format(raw.dtype))
        i = torch.from_numpy(raw.astype(np.int64).reshape(-1)).to(_device())
        return ops.mulaw_decode(i, [0, i.numel()], mu).cpu().numpy().reshape(raw.shape)

    @staticmethod
    def start_and_end_indices(quantized, silence_threshold=20):
        """(start, end) of the reference's silence trim on mu-law indices: the first sample further than the
        threshold from the centre 127 (fixed, whatever mu is), and the last such sample at an index above 1 (its
        backward scan is range(size - 1, 1, -1)).  The caller keeps [start, end): the sample at `end` is dropped, as
        there.  A signal without such samples fails the reference's assertions, and fails here."""
        quantized = np.asarray(quantized)
        loud = np.abs(quantized.astype(np.int64) - 127) > silence_threshold
        front, back = np.flatnonzero(loud), np.flatnonzero(loud[2:])
        assert front.size > 0, "no sample is further than {} from 127".format(silence_threshold)
        assert back.size > 0, "no sample after the first two is further than {} from 127".format(silence_threshold)
        return int(front[0]), int(back[-1]) + 2

    def preprocess_batch(self, samples):
        """`preprocess_sample` of a list of float64 signals, on the device: a list of float32 tensors [T_s, mu + 1]
        (views of one buffer written by one launch) or [T_s, 1] without mu."""
        import torch
        from idiaptts_amd import ops
        dev = _device()
        if self.mu is None:
            return [torch.from_numpy(np.asarray(s, dtype=np.float64).reshape(-1)).to(dev).float().unsqueeze(-1)
                    for s in samples]
        signals = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1) for s in samples]
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
        x = torch.from_numpy(np.concatenate(signals) if signals else np.zeros(0)).to(dev)
        begins, lengths = list(offsets[:-1]), [len(s) for s in signals]
        if self.silence_threshold_quantized is not None:
            index = ops.mulaw_encode(x, offsets, self.mu).cpu().numpy()
            for n in range(len(signals)):
                start, end = self.start_and_end_indices(index[offsets[n]:offsets[n + 1]],
                                                        self.silence_threshold_quantized)
                begins[n], lengths[n] = offsets[n] + start, max(end - start, 0)
        onehot, out_off = ops.mulaw_onehot(x, begins, lengths, self.mu)
        return [onehot[out_off[n]:out_off[n + 1]] for n in range(len(signals))]

    def preprocess_sample(self, sample):
        if self.mu is None:
            return np.expand_dims(sample, -1).astype(np.float32)
        return self.preprocess_batch([sample])[0].cpu().numpy()

    def postprocess_sample(self, sample, norm_params=None):
        """Network output [T, C] back to a waveform: arg-max and inverse companding with mu, then times
        norm_params."""
        if self.mu is not None:
            sample = self.mu_law_companding_reversed(np.asarray(sample).argmax(axis=1), self.mu)
        if norm_params is not None:
            sample *= norm_params
        elif self.norm_params is not None:
            sample *= self.norm_params
        return sample

    def set_normalisation_params(self, norm_params):
        self.norm_params = norm_params
        return self.norm_params

    def gen_data(self, *args, **kwargs):
        raise NotImplementedError()
