"""Function that down-samples a list of audio files (the reference's src/data_preparation/audio/down_sampling.py).

python down_sampling.py <dir_audio> <dir_out> <file_id_list> <target_sampling_rate>

The reference resamples with librosa.load(sr=target), i.e. resampy or soxr; here the polyphase kernel of
csrc/audio_prep.hip computes scipy.signal.resample_poly(x, target, rate) with scipy's default Kaiser filter.
Importing this module runs nothing (the reference's runs at import)."""
import os
import sys
from math import gcd
from shutil import copy

import numpy as np
import scipy.signal

from .... import ops
from . import audio_batch


def resample_filter(up, down):
    """scipy.signal.resample_poly's default filter for the reduced ratio up / down, times up."""
    max_rate = max(up, down)
    half_len = 10 * max_rate
    return scipy.signal.firwin(2 * half_len + 1, 1. / max_rate, window=("kaiser", 5.0)) * up


def resample_ratio(current_sampling_rate, target_sampling_rate):
    g = gcd(int(current_sampling_rate), int(target_sampling_rate))
    up, down = int(target_sampling_rate) // g, int(current_sampling_rate) // g
    if max(up, down) > ops.RESAMPLE_MAX_RATE:
        raise ValueError("Resampling from {} to {} Hz needs the ratio {}/{}: max(up, down) > {} is not implemented."
                         .format(current_sampling_rate, target_sampling_rate, up, down, ops.RESAMPLE_MAX_RATE))
    return up, down


def resample(samples, offsets, current_sampling_rate, target_sampling_rate):
    """The signals behind `offsets` at the target rate: (samples, offsets)."""
    up, down = resample_ratio(current_sampling_rate, target_sampling_rate)
    taps = audio_batch.to_device(resample_filter(up, down))
    y, out_off = ops.resample_poly(audio_batch.to_device(samples), offsets, up, down, taps)
    return y.cpu().numpy(), np.asarray(out_off, dtype=np.int64)


def downsample_list(id_list, dir_audio, dir_out, target_sampling_rate):
    target_sampling_rate = int(target_sampling_rate)
    files = [file_id + ".wav" for file_id in id_list]
    for names, fs in audio_batch.plan_batches(files, dir_audio, average_channels=True):
        if fs == target_sampling_rate:
            for name in names:
                full_path_in, full_path_out = os.path.join(dir_audio, name), os.path.join(dir_out, name)
                print("{} is at {} Hz already: copied.".format(full_path_in, fs))
                audio_batch.make_parent_dir(full_path_out)
                copy(full_path_in, full_path_out)
            continue
        resample_ratio(fs, target_sampling_rate)                 # (refuses before anything is read)
        for name in names:
            print("{}: {} -> {} Hz.".format(os.path.join(dir_audio, name), fs, target_sampling_rate))
        samples, offsets = audio_batch.read_batch(names, dir_audio, average_channels=True)
        y, out_off = resample(samples, offsets, fs, target_sampling_rate)
        for name, raw in zip(names, audio_batch.split(y, out_off)):
            audio_batch.make_parent_dir(os.path.join(dir_out, name))
            audio_batch.write_pcm16(os.path.join(dir_out, name), raw, target_sampling_rate)


def main(argv=None):
    argv = sys.argv if argv is None else argv
    dir_audio = argv[1]
    dir_out = argv[2]
    file_id_list = argv[3]
    target_sampling_rate = int(argv[4])
    downsample_list(audio_batch.read_id_list(file_id_list), dir_audio, dir_out, target_sampling_rate)


if __name__ == "__main__":
    main()
