"""Scales every given audio file to one root-mean-square level after removing its mean (the reference's
src/data_preparation/audio/normalize_loudness.py), on the loudness kernels of csrc/audio_prep.hip.  The files are
named by an id list; results go to the output directory under the same names."""
import logging

from .... import ops
from . import audio_batch


class LoudnessNormalizer(object):
    logger = logging.getLogger(__name__)

    def __init__(self, ref_rms=0.1):
        self.ref_rms = ref_rms

    @staticmethod
    def _refuse_silence(samples, offsets, paths):
        # the reference divides by a zero sum of squares and writes NaNs; here nothing of the list is written
        for path, signal in zip(paths, audio_batch.split(samples, offsets)):
            if not signal.any():
                raise ValueError("{} holds only zeros: its loudness cannot be normalised".format(path))

    def _step(self, samples, offsets, fs, paths):
        y = ops.loudness_normalise(audio_batch.to_device(samples), offsets, self.ref_rms).cpu().numpy()
        return audio_batch.split(y, offsets)

    def process_list(self, id_list, dir_audio, dir_out, format="wav"):
        audio_batch.process_list([file_id + "." + format for file_id in id_list], dir_audio, dir_out, self._step,
                                 precheck=self._refuse_silence)

    def process_file(self, file, dir_audio, dir_out):
        return audio_batch.process_list([file], dir_audio, dir_out, self._step, precheck=self._refuse_silence)[0]


def main():
    parser = audio_batch.list_parser(__doc__)
    parser.add_argument("--ref_rms", type=float, dest="ref_rms", required=False, default=0.1,
                        help="root-mean-square level every file is brought to")
    audio_batch.run_command_line(parser, lambda args: LoudnessNormalizer(args.ref_rms))


if __name__ == "__main__":
    main()
