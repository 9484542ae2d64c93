"""Zero-phase high-pass filtering of every given audio file (the reference's
src/data_preparation/audio/high_pass_filter.py): a least-squares FIR design, applied forwards and backwards
(scipy.signal.filtfilt) by the unit-rate FIR kernel of csrc/audio_prep.hip.  The files are named by an id list; results
go to the output directory under the same names."""
import logging

import numpy as np
import scipy.signal

from .... import ops
from . import audio_batch


class HighPassFilter(object):
    logger = logging.getLogger(__name__)

    def __init__(self, stop_freq_Hz=70, pass_freq_Hz=100, filter_order=1001):
        self.stop_freq_Hz = stop_freq_Hz
        self.pass_freq_Hz = pass_freq_Hz
        self.filter_order = filter_order
        self._taps = {}

    def filter_coefs(self, fs):
        """signal.firls(filter_order, (0, stop, pass, fs / 2), (0, 0, 1, 1)) -- the reference passes nyq=fs / 2, which
        scipy has since removed; fs=fs is the same design.  Cached per rate."""
        if fs not in self._taps:
            bands = (0, self.stop_freq_Hz, self.pass_freq_Hz, fs / 2.)
            self._taps[fs] = np.ascontiguousarray(
                scipy.signal.firls(self.filter_order, bands, (0, 0, 1, 1), fs=fs), dtype=np.float64)
        return self._taps[fs]

    def _padlen_text(self):
        # scipy.signal.filtfilt's refusal (padlen = 3 * max(len(a), len(b)))
        return "The length of the input vector x must be greater than padlen, which is {}.".format(
            3 * self.filter_order)

    def _step(self, samples, offsets, fs, paths):
        taps = audio_batch.to_device(self.filter_coefs(fs))
        y = ops.fir_filtfilt(audio_batch.to_device(samples), offsets, taps).cpu().numpy()
        return audio_batch.split(y, offsets)

    def process_list(self, id_list, dir_audio, dir_out, format="wav"):
        audio_batch.process_list([file_id + "." + format for file_id in id_list], dir_audio, dir_out, self._step,
                                 min_samples=3 * self.filter_order, min_samples_text=self._padlen_text())

    def process_file(self, file, dir_audio, dir_out):
        return audio_batch.process_list([file], dir_audio, dir_out, self._step, min_samples=3 * self.filter_order,
                                        min_samples_text=self._padlen_text())[0]

    def highpass_filter(self, raw, fs):
        raw = np.asarray(raw, dtype=np.float64)
        if raw.ndim != 1:
            raise ValueError("highpass_filter takes one mono signal, got shape {}".format(raw.shape))
        if len(raw) <= 3 * self.filter_order:
            raise ValueError(self._padlen_text())
        return self._step(raw, np.array([0, len(raw)], dtype=np.int64), fs, None)[0]


def main():
    parser = audio_batch.list_parser(__doc__)
    parser.add_argument("--stop_freq_Hz", type=float, dest="stop_freq_Hz", required=False, default=70,
                        help="upper edge of the stop band: nothing below it passes")
    parser.add_argument("--pass_freq_Hz", type=float, dest="pass_freq_Hz", required=False, default=100,
                        help="lower edge of the pass band; the gain rises from 0 to 1 between the two edges")
    parser.add_argument("--filter_order", type=int, dest="filter_order", required=False, default=1001,
                        help="number of filter taps (odd)")
    audio_batch.run_command_line(
        parser, lambda args: HighPassFilter(args.stop_freq_Hz, args.pass_freq_Hz, args.filter_order))


if __name__ == "__main__":
    main()
